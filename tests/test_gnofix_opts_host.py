"""Gnofix search options, host side (no GPU): the numpy restatement against the reference's recorded outputs and against
oracle.gnofix at the defaults; the C struct against the header; the Python-side refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import load_golden, trees_from_npz
from gnofix_opts_exact import DEFAULTS, candidates, gnofix_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "G24_gnofix_opts.npz"


def fixture_cases():
    g = load_golden(FIXTURE)
    return [(str(name), k) for name in g["geoms"] for k in range(len(g[str(name) + "_cases"]))]


def case_options(g, name, k):
    opt = json.loads(str(g[name + "_cases"][k]))
    return opt.pop("max_it"), opt


@pytest.mark.parametrize("name,k", fixture_cases())
def test_restatement_equals_the_reference(oracle, name, k):
    g = load_golden(FIXTURE)
    T = trees_from_npz(oracle, g, name + "_t_")
    S, X, B = int(g[name + "_S"]), g[name + "_X"], g[name + "_B"]
    max_it, opt = case_options(g, name, k)
    rows = lambda r: oracle.xgb_predict_proba(T, np.asarray(r, dtype=np.float32))
    labs = lambda b: oracle.smooth_xgb(T, b, S)[1]
    oX, oY, trk, nh = (g["%s_%d_%s" % (name, k, f)] for f in ("oX", "oY", "trk", "nhist"))
    for i in range(X.shape[0] // 2):
        Xm, Xp, Ym, Yp, t, ns = gnofix_opts(X[2 * i], X[2 * i + 1], B[2 * i:2 * i + 2], S, rows, labs, max_it=max_it, **opt)
        assert np.array_equal(Xm, oX[2 * i]) and np.array_equal(Xp, oX[2 * i + 1]), i
        assert np.array_equal(Ym, oY[2 * i]) and np.array_equal(Yp, oY[2 * i + 1]), i
        assert np.array_equal(t, trk[i]) and ns == int(nh[i]) - 2, i


def test_fixture_shows_every_option():
    """every option set differs from the defaults on some individual (what the generator asserts when it writes the file)"""
    g = load_golden(FIXTURE)
    for name in map(str, g["geoms"]):
        for k in range(1, len(g[name + "_cases"])):
            same = all(np.array_equal(g["%s_%d_%s" % (name, k, f)], g["%s_0_%s" % (name, f)]) for f in ("oX", "oY", "trk", "nhist"))
            assert not same, (name, k)
        assert case_options(g, name, 0)[1] == {}


@pytest.mark.parametrize("name", ["one", "two", "edges", "many", "rand"])
def test_restatement_at_the_defaults_equals_oracle_gnofix(oracle, name):
    g = load_golden("G5_gnofix.npz")
    T = trees_from_npz(oracle, g, "r_" if name == "rand" else "t_")
    S = int(g["S"])
    rows = lambda r: oracle.xgb_predict_proba(T, np.asarray(r, dtype=np.float32))
    labs = lambda b: oracle.smooth_xgb(T, b, S)[1]
    max_it = 4 if name == "rand" else 50
    ref = oracle.gnofix(g[name + "_Xm"], g[name + "_Xp"], g[name + "_B"], S, rows, labs, max_it=max_it)
    got = gnofix_opts(g[name + "_Xm"], g[name + "_Xp"], g[name + "_B"], S, rows, labs, max_it=max_it, **DEFAULTS)
    for a, b in zip(ref[:5], got[:5]):
        assert np.array_equal(a, b)
    assert ref[5] == got[5]
    assert np.array_equal(got[0], g[name + "_oXm"]) and np.array_equal(got[2], g[name + "_oYm"])  # and the reference itself


def test_candidate_order():
    assert candidates(7, 0, 0) == [(7, None)]
    assert candidates(7, 2, 0) == [(5, None), (6, None), (7, None), (8, None), (9, None)]
    assert candidates(7, 0, 1) == [(7, None), (7, 8)]
    assert candidates(7, 1, 3) == [(6, None), (7, None), (8, None), (6, 7), (5, 7), (7, 8), (7, 9), (7, 10)]


def _header():
    return open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()


def test_struct_layout_matches_the_header():
    from gnomix_amd import _lib
    body = re.search(r"typedef struct gnx_gnofix_opts \{(.*?)\} gnx_gnofix_opts;", _header(), re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.GnofixOpts._fields_)
    off = 0
    for t, n in fields:  # natural alignment, as the C compiler lays it out
        sz = 4 if t == "int32_t" else 8
        off = (off + sz - 1) // sz * sz
        assert getattr(_lib.GnofixOpts, n).offset == off, n
        off += sz
    assert C.sizeof(_lib.GnofixOpts) == (off + 7) // 8 * 8 == 40
    enums = dict(re.findall(r"(GNX_GNOFIX_(?:CHECK|PROB)_\w+) = (\d+)", _header()))
    assert {k: int(v) for k, v in enums.items()} == {
        "GNX_GNOFIX_CHECK_DISC_SMOOTH": 0, "GNX_GNOFIX_CHECK_ALL": 1, "GNX_GNOFIX_CHECK_DISC_BASE": 2, "GNX_GNOFIX_CHECK_DISC_EITHER": 3,
        "GNX_GNOFIX_PROB_MAX": 0, "GNX_GNOFIX_PROB_PROD": 1}
    assert _lib.GNOFIX_CHECKS == {"disc_smooth": 0, "all": 1, "disc_base": 2, "disc_either": 3}
    assert _lib.GNOFIX_PROB_COMPS == {"max": 0, "prod": 1}
    for sym in ("gnx_gnofix_ex", "gnx_gnofix_ex_dev"):
        assert sym in _lib.SYMBOLS and re.search(r"\bint %s\(" % sym, _header())


def test_abi_version_is_still_16():
    from gnomix_amd import _lib
    assert re.search(r"#define GNX_ABI_VERSION (\d+)", _header()).group(1) == "16"
    assert _lib.GNX_ABI_VERSION == 16


def test_python_side_refusals():
    from gnomix_amd import _lib
    o = _lib.gnofix_opts(7, check_criterion="disc_either", max_center_offset=2, non_lin_s=1, prob_comp="prod", prior_switch_prob=0.3,
                         padding=False)
    assert (o.struct_bytes, o.max_it, o.check_criterion, o.max_center_offset, o.non_lin_s, o.prob_comp, o.padding, o.prior_switch_prob) == \
        (40, 7, 3, 2, 1, 1, 0, 0.3)
    d = _lib.gnofix_opts()
    assert (d.max_it, d.check_criterion, d.max_center_offset, d.non_lin_s, d.prob_comp, d.padding, d.prior_switch_prob) == (50, 0, 0, 0, 0, 1, 0.5)
    for name in ("naive_switch", "end_naive_switch", "d"):
        with pytest.raises(NotImplementedError, match=name):
            _lib.gnofix_opts(**{name: 3})
        _lib.gnofix_opts(**{name: None})  # the reference's own default
    with pytest.raises(ValueError, match="check_criterion"):
        _lib.gnofix_opts(check_criterion="disc_everything")
    with pytest.raises(ValueError, match="prob_comp"):
        _lib.gnofix_opts(prob_comp="sum")
    with pytest.raises(TypeError, match="mode_filter"):
        _lib.gnofix_opts(mode_filter=3)


def test_python_entry_points_take_the_options():
    import inspect
    from gnomix_amd import gnomix, model
    for fn in (model.DeviceModel.gnofix, model.DeviceModel.gnofix_device, gnomix.HipGnomix.phase):
        kinds = [p.kind for p in inspect.signature(fn).parameters.values()]
        assert inspect.Parameter.VAR_KEYWORD in kinds, fn


def test_gpu_fuzz_inputs_cover_what_the_fuzz_is_for(oracle):
    """the 40 fuzz seeds of tests/test_gpu_gnofix_opts.py, through the restatement alone: some individuals end at the iteration cap,
    some at the convergence stop; accepted double switches and accepted switches at window 0 occur; every criterion, both prob_comp
    values, both padding values and a window size C // W != M are drawn"""
    import test_gpu_gnofix_opts as F
    capped = converged = doubles = at_zero = switches = 0
    seen, ws_differs = set(), 0
    for seed in range(F.FUZZ_SEEDS):
        (S, W, A, M, Cn), _, opt, max_it, _, _ = F.fuzz_case(seed)
        ev, st = [], []
        res = F.fuzz_reference(oracle, seed, events=ev, stats=st)
        capped += sum(s["capped"] for s in st)
        converged += sum(not s["capped"] for s in st)
        switches += sum(r[5] for r in res)
        doubles += sum(j2 is not None for (_, _, j2) in ev)
        at_zero += sum(j2 is None and j1 == 0 for (_, j1, j2) in ev)
        seen |= {opt["check_criterion"], opt["prob_comp"], "padding=%s" % opt["padding"]}
        ws_differs += Cn // W != M
    assert capped >= 10 and converged >= 10, (capped, converged)
    assert doubles >= 10 and at_zero >= 1 and switches >= 200, (doubles, at_zero, switches)
    assert seen == {"disc_smooth", "all", "disc_base", "disc_either", "max", "prod", "padding=True", "padding=False"}
    assert ws_differs >= 4
