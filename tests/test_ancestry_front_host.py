"""The Python side of the ancestry-specific ops (gnomix_amd/ancestry_ops.py), without a GPU: the one copy of each helper (window span,
verdict, labels check), the host front's row preparation, and that each of them is written in one place."""
import ast
import glob
import itertools
import os

import numpy as np
import pytest

from gnomix_amd import _lib, ancestry_ops as ops, assoc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = _lib.GNX_OK, _lib.GNX_EINVAL, _lib.GNX_EUNSUPPORTED


@pytest.mark.parametrize("C,M,W", [(37, 9, 4), (10, 10, 1)])
def test_window_span_is_the_number_of_windows_a_range_touches(C, M, W):
    for c0 in range(C):
        for c1 in range(c0 + 1, C + 1):
            assert assoc.window_span(c0, c1, M, W) == len({min(c // M, W - 1) for c in range(c0, c1)}), (c0, c1)
    for c0, c1 in ((5, 5), (9, 3), (C, C), (-1, 4), (-3, -1), (-2, C)):
        assert assoc.window_span(c0, c1, M, W) == 1, (c0, c1)
    # the buffers of the three association ops are cut with it
    assert assoc.stats_buffers(3, 2, 5, 30, M, W)[2].shape[0] == assoc.window_span(5, 30, M, W)
    assert assoc.trait_buffers(3, 2, 3, 5, 30, M, W)[1].shape[0] == assoc.window_span(5, 30, M, W)
    assert assoc.logit_buffers(3, 2, 5, 30, M, W)[3].shape[0] == assoc.window_span(5, 30, M, W)


class _Ctx:
    """Context.check: raises for a code that is not GNX_OK; records what it was given"""
    h = 1234

    def __init__(self):
        self.seen = []

    def check(self, rc):
        self.seen.append(rc)
        if rc != OK:
            raise _lib.GnxError(rc, "stub")


# (rc, n_bad, check) in this order; True = the call raises GnxError(rc), False = the outputs are handed over
CASES = [(rc, n_bad, check) for rc in (OK, EINVAL, EUNSUPPORTED) for n_bad in (0, 3) for check in (True, False)]
RAISES = {
    # linear, traits: `if check or (rc != GNX_OK and not n_bad.value): ctx.check(rc)`
    "linear": [False, False, False, False,   True, True, True, False,   True, True, True, False],
    # logit: `if check or rc not in (GNX_OK, GNX_EINVAL) or (rc != GNX_OK and not n_bad.value): ctx.check(rc)`
    "logit": [False, False, False, False,   True, True, True, False,   True, True, True, True],
    # pairs, LD (host form): `if check or not n_bad.value: ctx.check(rc)`
    "pairs": [False, False, False, False,   True, True, True, False,   True, True, True, False],
}
HANDED = {"linear": None, "logit": (EINVAL,), "pairs": None}


@pytest.mark.parametrize("rule", sorted(RAISES))
def test_verdict_table(rule):
    assert len(CASES) == 12
    for (rc, n_bad, check), raises in zip(CASES, RAISES[rule]):
        ctx = _Ctx()
        if raises:
            with pytest.raises(_lib.GnxError) as err:
                ops.verdict(ctx, rc, n_bad, check, HANDED[rule])
            assert err.value.code == rc and ctx.seen == [rc], (rule, rc, n_bad, check)
        else:
            ops.verdict(ctx, rc, n_bad, check, HANDED[rule])
            assert ctx.seen in ([], [OK]), (rule, rc, n_bad, check)     # nothing a Context would raise for was passed on
    # the forms without `check` always raise on a code that is not GNX_OK
    for rc, n_bad in itertools.product((EINVAL, EUNSUPPORTED), (0, 3)):
        with pytest.raises(_lib.GnxError):
            ops.verdict(_Ctx(), rc, n_bad)


def test_host_front_rows():
    N, C, M, W, A = 8, 37, 9, 4, 3
    rng = np.random.default_rng(0)
    lab = rng.integers(0, A, size=(N, W)).astype(np.int32)
    wide = np.zeros((N, C + 7), np.int8)
    wide[:, :C] = rng.integers(0, 3, size=(N, C))
    X = wide[:, :C]
    assert X.strides == (C + 7, 1)
    # the association ops' front: int8 rows with a row stride go through as they are
    f = ops.host_front(_Ctx(), X, lab, M, A, strided=True)
    assert f.suffix == "" and (f.N, f.C, f.M, f.W, f.A) == (N, C, M, W, A)
    assert f.head == (1234, X.ctypes.data, _lib.GNX_ROWS_INT8, C + 7, f.keep[1].ctypes.data, W, N, C, M, W, A)
    assert f.keep[0] is X
    # ... the other ops' front makes them contiguous
    f = ops.host_front(_Ctx(), X, lab, M, A)
    assert f.head[1] != X.ctypes.data and f.head[3] == C and f.keep[0].flags.c_contiguous and np.array_equal(f.keep[0], X)
    # another integer dtype is re-coded: whatever is not 0 / 1 is the missing code 2
    X16 = X.astype(np.int16)
    X16[2, 5], X16[3, 6], X16[4, 7] = 3, -1, 256
    for strided in (False, True):
        f = ops.host_front(_Ctx(), X16, lab, M, A, strided=strided)
        rows = f.keep[0]
        assert rows.dtype == np.int8 and rows.flags.c_contiguous and (rows[2, 5], rows[3, 6], rows[4, 7]) == (2, 2, 2)
        keep = np.ones((N, C), bool)
        keep[[2, 3, 4], [5, 6, 7]] = False
        assert np.array_equal(rows[keep], np.where(X[keep] > 1, 2, X[keep]))
    # packed rows: C is needed, and a row holds at least ceil(C / 4) bytes
    P = np.zeros((N, (C + 3) // 4 + 3), np.uint8)
    with pytest.raises(ValueError, match="pass C"):
        ops.host_front(_Ctx(), P, lab, M, A, packed=True)
    with pytest.raises(ValueError, match=r"ceil\(C / 4\) = 10"):
        ops.host_front(_Ctx(), P[:, :(C + 3) // 4 - 1], lab, M, A, packed=True, C=C)
    f = ops.host_front(_Ctx(), P, lab, M, A, packed=True, C=C)
    assert f.head[2:4] == (_lib.GNX_ROWS_PACKED2, (C + 3) // 4 + 3) and f.C == C
    # one row: the row width stands in for the stride
    for strided in (False, True):
        f = ops.host_front(_Ctx(), X[:1], lab[:1], M, A, strided=strided)
        assert f.N == 1 and f.head[3] == C
    # the outputs: numpy arrays, zeroed unless asked otherwise; addresses; None stays None
    z = f.alloc((3, 2), np.int32)
    assert isinstance(z, np.ndarray) and z.dtype == np.int32 and not z.any() and f.alloc((3, 2), np.float64, False).shape == (3, 2)
    assert f.ptr(z) == z.ctypes.data and f.ptr(None) is None and f.host(z) is z and f.put(z) is z
    # rows, then an even N, then the labels
    with pytest.raises(ValueError, match="N must be even"):
        ops.host_front(_Ctx(), X[:7], lab[:5], M, A, even=True)
    with pytest.raises(ValueError, match=r"X has 37 columns, C = 36"):
        ops.host_front(_Ctx(), X[:7], lab[:5], M, A, C=36, even=True)


def test_labels_check():
    N, W = 6, 4
    lab64 = np.arange(N * W * 2, dtype=np.int64).reshape(N, 2 * W)[:, ::2]
    assert not lab64.flags.c_contiguous
    out = ops.check_labels(lab64, N, W)
    assert out.dtype == np.int32 and out.flags.c_contiguous and np.array_equal(out, lab64)
    assert ops.check_labels(lab64, N).shape == (N, W)                     # no model: W is the labels' own
    with pytest.raises(ValueError, match=r"labels must be \(N=5, W=4\), got \(6, 4\)"):
        ops.check_labels(lab64, N - 1, W)                                 # wrong N
    with pytest.raises(ValueError, match=r"labels must be \(N=5, W\), got \(6, 4\)"):
        ops.check_labels(lab64, N - 1)
    with pytest.raises(ValueError, match=r"labels must be \(N=6, W=5\), got \(6, 4\)"):
        ops.check_labels(lab64, N, W + 1)                                 # wrong W under a model
    with pytest.raises(ValueError, match=r"labels must be \(N=6, W\), got \(24,\)"):
        ops.check_labels(np.zeros(N * W), N)


def _code_only(path):
    """the module's code with comments and docstrings gone"""
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and ast.get_docstring(node, clean=False) is not None:
            node.body = node.body[1:] or [ast.Pass()]
    return ast.unparse(tree)


def test_front_helpers_have_one_definition():
    """The checks and the chunk loop every ancestry-specific op shares are written once in the Python layer (DESIGN.md names
    ancestry_ops.py as their home): a pasted copy is where the forms of an op start to differ."""
    text = {os.path.basename(p): _code_only(p) for p in glob.glob(os.path.join(ROOT, "gnomix_amd", "*.py"))}
    assert len(text) > 20 and "ancestry_ops.py" in text

    def homes(needle):
        return sorted((name, src.count(needle)) for name, src in text.items() if needle in src)

    assert homes("N must be even") == [("ancestry_ops.py", 1)]
    assert homes("labels must be (N=") == [("ancestry_ops.py", 1)]
    assert homes("(c1 - 1) //") == [("assoc.py", 1)]
    assert homes("def score_chunks(") == [("postprocess.py", 1)]
    calls = [(name, n - (name == "postprocess.py")) for name, n in homes("score_chunks(")]
    assert [c for c in calls if c[1]] == [("ancestry_ops.py", 1)]
    # DeviceModel keeps no ancestry-specific method of its own
    assert "def ancestry_" not in text["model.py"] and "class DeviceModel(AncestryOps)" in text["model.py"]
