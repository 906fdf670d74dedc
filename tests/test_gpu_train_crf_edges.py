"""gnx_train_crf (csrc/k_train_crf.hip) across its dispatch table, chain and block edges, entry by entry of the gradient.

tests/test_train_crf.py holds the trainer to the oracle at four shapes, through the objective and the gradient's NORM.  Here:
  the grid   every k_crf_eval<KP> instantiation and its boundaries (A = 8 | 9, 16 | 17, 32), W = 1, 2, 3 (no edge, the t - 2
             prefetches), W = 64 | 65 (the lane stride), N = 1, 3, 4, 5 (dead waves), N = 32 | 33 (the reduction's chunk), float32 B;
  the gradient, ENTRY BY ENTRY, read through the ABI: with no stored pair the first L-BFGS direction is d = -g / |g| and the line
             search only scales it, so after max_iterations = 1 the displacement w0 - w1 is a positive multiple of g(w0).  Its unit
             vector is compared with the oracle's; a transposed state or transition block, or exchanged halves, move that vector by
             > 1e-3 (asserted on the oracle's side, tests/crf_cases.py) against a bar of ~1e-9;
  labels and inputs at their edges, c2 != 1 (k_crf_reduce2's regulariser no longer hides in a relative bar), weights of scale 5 and
             20 over 400 windows (the rescaled forward pass far from zero), fits at <16>, the host L-BFGS's controls, refusals.
The bars are the project's: 1e-10 |f| on the objective, 1e-9 |g| on the gradient (norm and direction).  The oracle's own error on the
far-weight cases, measured against a longdouble restatement (tests/test_train_crf_cases_host.py), is ~1e-11: no bar is widened."""
import ctypes as C

import numpy as np
import pytest

import crf_cases as CC

pytestmark = pytest.mark.gpu


def _norm(*a):
    return float(np.sqrt(sum(np.sum(np.square(x, dtype=np.float64)) for x in a)))


def _check_point(oracle, B, y, st0, tr0, c2=1.0):
    """the two checks at one point (state0, trans0): objective and gradient norm after zero iterations, the gradient's direction
    after one -> (state1, trans1, the zero-iteration info)"""
    from gnomix_amd.train import train_crf_arrays
    A = B.shape[2]
    f, gs, gt = oracle.crf_objective(B, y, st0, tr0, c2)
    gn = _norm(gs, gt)
    assert np.isfinite(f) and np.all(np.isfinite(gs)) and np.all(np.isfinite(gt)) and gn > 0
    v = CC.unit(gs, gt)
    if A > 2 and np.any(st0):       # the check below can fail: each indexing slip moves the oracle's own direction by far more than the bar
        for name, m in CC.mutations(gs, gt).items():
            assert np.max(np.abs(m - v)) > 1e-3, name

    s_, t_, info0 = train_crf_arrays(B, y, c2=c2, max_iterations=0, state0=st0, trans0=tr0)
    print("f dev %.17g oracle %.17g rel %.3g | |g| dev %.17g oracle %.17g rel %.3g" % (
        info0["objective"], f, abs(info0["objective"] - f) / abs(f), info0["grad_norm"], gn, abs(info0["grad_norm"] - gn) / gn))
    assert info0["evaluations"] == 1 and info0["iterations"] == 0
    assert np.array_equal(s_, st0) and np.array_equal(t_, tr0)
    assert abs(info0["objective"] - f) <= 1e-10 * abs(f)
    assert abs(info0["grad_norm"] - gn) <= 1e-9 * gn

    st1, tr1, info1 = train_crf_arrays(B, y, c2=c2, max_iterations=1, state0=st0, trans0=tr0)
    w0 = np.concatenate([np.asarray(st0, np.float64).ravel(), np.asarray(tr0, np.float64).ravel()])
    w1 = np.concatenate([st1.ravel(), tr1.ravel()])
    assert info1["iterations"] == 1 and not np.array_equal(w1, w0)
    u = (w0 - w1) / _norm(w0 - w1)
    bound = CC.direction_bound(w0, w1)
    at = int(np.argmax(np.abs(u - v)))
    print("direction: max|u - v| %.3g at entry %d of %d, bar %.3g, step length %.3g" % (np.max(np.abs(u - v)), at, u.size, bound, _norm(w0 - w1)))
    assert np.max(np.abs(u - v)) <= bound, ("state" if at < A * A else "trans", divmod(at % (A * A), A))
    return st1, tr1, info0


def _starts(A, st0, tr0):
    return {"zero": (np.zeros((A, A)), np.zeros((A, A))), "normal": (st0, tr0)}


def _assert_no_edge_term(tr0, tr1, info0, c2=1.0):
    """W = 1: the data term of g_trans is exactly 0, the device's g_trans is 2 c2 trans0, and trans1 is the host's own arithmetic on it:
    trans0 + step * -(g_trans * h0), h0 = 1 / |g| (no pair stored yet), step one of the line search's powers of two.  Bit for bit —
    the displacement of the transition block is parallel to trans0"""
    if not np.any(tr0):
        assert np.array_equal(tr1, np.zeros_like(tr0))
        return
    h0 = 1.0 / max(1e-300, info0["grad_norm"])
    d = -((0.0 + 2.0 * c2 * tr0) * h0)
    steps = [2.0 ** k for k in range(-30, 31) if np.array_equal(tr0 + 2.0 ** k * d, tr1)]
    assert len(steps) == 1, steps


@pytest.mark.parametrize("start", ["zero", "normal"])
@pytest.mark.parametrize("N,W,A", CC.GRID)
def test_objective_and_gradient_entries_on_the_dispatch_grid(oracle, N, W, A, start):
    B, y, st0, tr0 = CC.case(N, W, A)
    st0, tr0 = _starts(A, st0, tr0)[start]
    st1, tr1, info0 = _check_point(oracle, B, y, st0, tr0)
    if W == 1:
        _assert_no_edge_term(tr0, tr1, info0)


@pytest.mark.parametrize("start", ["zero", "normal"])
@pytest.mark.parametrize("N,W,A", CC.F32_CASES)
def test_float32_base_probabilities(oracle, N, W, A, start):
    B, y, st0, tr0 = CC.case(N, W, A, dtype=np.float32)
    assert B.dtype == np.float32
    st0, tr0 = _starts(A, st0, tr0)[start]
    st1, tr1, info0 = _check_point(oracle, B, y, st0, tr0)       # the oracle widens the same float32 values
    if W == 1:
        _assert_no_edge_term(tr0, tr1, info0)


@pytest.mark.parametrize("start", ["zero", "normal"])
@pytest.mark.parametrize("kind", CC.LABEL_KINDS)
@pytest.mark.parametrize("N,W,A", CC.LABEL_CASES)
def test_labels_and_inputs_at_their_edges(oracle, N, W, A, kind, start):
    B, y, st0, tr0 = CC.case(N, W, A, kind=kind)
    if kind == "label_absent":
        assert not np.any(y == 2)
    if kind == "b_onehot":
        assert set(np.unique(B)) == {0.0, 1.0}
    st0, tr0 = _starts(A, st0, tr0)[start]
    _check_point(oracle, B, y, st0, tr0)


@pytest.mark.parametrize("start", ["zero", "normal"])
def test_two_labels_of_which_only_one_occurs(oracle, start):
    B, y, st0, tr0 = CC.case(5, 6, 2, kind="constant_set")
    assert np.all(y == 1)
    st0, tr0 = _starts(2, st0, tr0)[start]
    _check_point(oracle, B, y, st0, tr0)


@pytest.mark.parametrize("start", ["zero", "normal"])
@pytest.mark.parametrize("c2", CC.C2S)
@pytest.mark.parametrize("N,W,A", CC.C2_CASES)
def test_regulariser_weight_other_than_one(oracle, N, W, A, c2, start):
    B, y, st0, tr0 = CC.case(N, W, A)
    st0, tr0 = _starts(A, st0, tr0)[start]
    _check_point(oracle, B, y, st0, tr0, c2=c2)


@pytest.mark.parametrize("s", CC.FAR_SCALES)
@pytest.mark.parametrize("N,W,A", CC.FAR_CASES)
def test_weights_far_beyond_a_trained_model(oracle, N, W, A, s):
    """c2 = 1e-6 leaves f and g to the data term; weights of scale s make every window's rescaling and the running log Z large"""
    B, y, _, _ = CC.case(N, W, A)
    st0, tr0 = CC.far_start(N, W, A, s)
    _check_point(oracle, B, y, st0, tr0, c2=1e-6)


# ---- fits ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_case(oracle):
    """(N, W, A, c2) -> B, y, the oracle's fit (state, trans, f): computed once per shape and regulariser, shared, never written to"""
    cache = {}

    def get(N, W, A, c2):
        if (N, W, A, c2) not in cache:
            B, y, _, _ = CC.case(N, W, A)
            so, to, fo = oracle.crf_fit(B, y, c2=c2)
            for a in (B, y, so, to):
                a.setflags(write=False)
            cache[(N, W, A, c2)] = (B, y, so, to, fo)
        return cache[(N, W, A, c2)]
    return get


def _assert_same_optimum(oracle, B, y, c2, st, tr, info, so, to, fo):
    assert info["converged"]
    print("f dev %.17g oracle %.17g rel %.3g" % (info["objective"], fo, abs(info["objective"] - fo) / abs(fo)))
    assert abs(info["objective"] - fo) <= 1e-10 * abs(fo)
    _, gs, gt = oracle.crf_objective(B, y, st, tr, c2)          # the oracle's gradient at the device's answer
    assert max(np.abs(gs).max(), np.abs(gt).max()) < 1e-6
    # f - c2 |w|^2 is convex, so f is 2 c2-strongly convex: |g(a) - g(b)| >= 2 c2 |a - b|
    _, gso, gto = oracle.crf_objective(B, y, so, to, c2)
    dist, bound = _norm(st - so, tr - to), (_norm(gs, gt) + _norm(gso, gto)) / (2.0 * c2)
    print("|w_dev - w_or| %.3g, bound %.3g" % (dist, bound))
    assert dist <= bound


@pytest.mark.parametrize("N,W,A,c2", [(24, 12, 17, 1.0), (24, 12, 32, 1.0), (40, 30, 4, 0.01), (40, 30, 4, 10.0)])
def test_fit_from_zeros_reaches_the_oracles_optimum(oracle, fit_case, N, W, A, c2):
    from gnomix_amd.train import train_crf_arrays
    B, y, so, to, fo = fit_case(N, W, A, c2)
    st, tr, info = train_crf_arrays(B, y, c2=c2)
    _assert_same_optimum(oracle, B, y, c2, st, tr, info, so, to, fo)


@pytest.mark.parametrize("memory", [1, 64])
def test_lbfgs_memory_at_its_limits(oracle, fit_case, memory):
    from gnomix_amd.train import train_crf_arrays
    B, y, so, to, fo = fit_case(40, 30, 4, 1.0)
    st, tr, info = train_crf_arrays(B, y, memory=memory)
    _assert_same_optimum(oracle, B, y, 1.0, st, tr, info, so, to, fo)


def test_iteration_cap(oracle, fit_case):
    from gnomix_amd.train import train_crf_arrays
    B, y, _, _, _ = fit_case(40, 30, 4, 1.0)
    f0 = oracle.crf_objective(B, y, np.zeros((4, 4)), np.zeros((4, 4)))[0]
    st, tr, info = train_crf_arrays(B, y, max_iterations=3)
    assert info["iterations"] == 3 and not info["converged"] and info["objective"] < f0
    assert info["evaluations"] >= 4
    f3 = oracle.crf_objective(B, y, st, tr)[0]                  # the weights returned are the ones the objective belongs to
    assert abs(info["objective"] - f3) <= 1e-10 * abs(f3)


def test_warm_start_at_the_optimum_and_run_to_run_bits(fit_case):
    from gnomix_amd.train import train_crf_arrays
    B, y, _, _, _ = fit_case(40, 30, 4, 1.0)
    st, tr, info = train_crf_arrays(B, y)
    st2, tr2, info2 = train_crf_arrays(B, y)
    assert info["converged"]
    assert st.tobytes() == st2.tobytes() and tr.tobytes() == tr2.tobytes()        # fixed-order sums, no atomics: the same bits
    assert np.float64(info["objective"]).tobytes() == np.float64(info2["objective"]).tobytes()
    assert np.float64(info["grad_norm"]).tobytes() == np.float64(info2["grad_norm"]).tobytes()
    assert info["iterations"] == info2["iterations"] and info["evaluations"] == info2["evaluations"]
    st3, tr3, info3 = train_crf_arrays(B, y, state0=st, trans0=tr)
    assert info3["iterations"] == 0 and info3["evaluations"] == 1 and info3["converged"]
    assert st3.tobytes() == st.tobytes() and tr3.tobytes() == tr.tobytes()
    assert np.float64(info3["objective"]).tobytes() == np.float64(info["objective"]).tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------------
_GOOD = dict(N=4, W=10, A=3, c1=0.0, c2=1.0, epsilon=1e-8, max_iterations=10, memory=10)
_REFUSED = {
    "A=1": dict(A=1), "A=33": dict(A=33), "W=0": dict(W=0), "N=0": dict(N=0), "epsilon=0": dict(epsilon=0.0),
    "max_iterations=-1": dict(max_iterations=-1), "memory=0": dict(memory=0), "memory=65": dict(memory=65),
    "B=NULL": dict(null="B"), "y=NULL": dict(null="y"), "params=NULL": dict(null="P"), "state=NULL": dict(null="state"),
    "trans=NULL": dict(null="trans"),
}


@pytest.mark.parametrize("what", list(_REFUSED))
def test_refusals_leave_the_weights_alone(what):
    from gnomix_amd import _lib
    k = dict(_GOOD, null=None)
    k.update(_REFUSED[what])
    ctx = _lib.default_context(0)
    A = k["A"]
    B = np.full((4, 10, 33), 1.0 / 33)                          # as large as any (N, W, A) below would read
    y = np.zeros((4, 10), np.int32)
    P = _lib.CrfParams(k["c1"], k["c2"], k["epsilon"], k["max_iterations"], k["memory"])
    poison = -1234.5
    st, tr = np.full((33, 33), poison), np.full((33, 33), poison)
    info = _lib.CrfInfo()
    ptr = {"B": B.ctypes.data, "y": y.ctypes.data, "P": C.byref(P), "state": st.ctypes.data, "trans": tr.ctypes.data}
    if k["null"]:
        ptr[k["null"]] = None
    rc = ctx.lib.gnx_train_crf(ctx.h, ptr["B"], 1, ptr["y"], k["N"], k["W"], A, ptr["P"], ptr["state"], ptr["trans"], C.byref(info))
    assert rc != 0
    assert b"train_crf" in ctx.lib.gnx_last_error(ctx.h)
    assert np.all(st == poison) and np.all(tr == poison)


def test_the_accepted_call_beside_the_refusals():
    """the arguments the refusals start from are themselves accepted: each refusal is down to the one argument it changes"""
    from gnomix_amd import _lib
    ctx = _lib.default_context(0)
    k = _GOOD
    B = np.full((k["N"], k["W"], k["A"]), 1.0 / 3)
    y = np.zeros((k["N"], k["W"]), np.int32)
    P = _lib.CrfParams(k["c1"], k["c2"], k["epsilon"], k["max_iterations"], k["memory"])
    st, tr = np.zeros((3, 3)), np.zeros((3, 3))
    assert ctx.lib.gnx_train_crf(ctx.h, B.ctypes.data, 1, y.ctypes.data, k["N"], k["W"], k["A"], C.byref(P), st.ctypes.data, tr.ctypes.data, None) == 0
    assert np.any(st != 0)
