"""gnx_gnofix_ex / gnx_gnofix_ex_dev (k_gnofix_opts.hip) on the GPU: the reference's recorded outputs for every option set
(tests/golden/G24_gnofix_opts.npz), a fuzz against the numpy restatement (tests/gnofix_opts_exact.py), default options against
gnx_gnofix, the refusals, and HipGnomix.phase with options."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import load_golden, trees_from_npz
from gnofix_opts_exact import gnofix_opts

pytestmark = pytest.mark.gpu
FIXTURE = "G24_gnofix_opts.npz"


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _model(ga, g, p, name):
    W, A, S, Cn = (int(g[name + k]) for k in ("_W", "_A", "_S", "_C"))
    t = name + "_t_"
    return ga.GnxModelData(C=Cn, M=Cn // W, A=A, S=S, context=0, smooth_kind="xgb", tree_off=g[t + "tree_off"], left=g[t + "left"],
                           right=g[t + "right"], feat=g[t + "feat"], cond=g[t + "cond"], tree_class=g[t + "tree_class"],
                           base_score=float(g[t + "base_score"]))


@pytest.fixture(scope="module")
def fixture_models(ga):
    g = load_golden(FIXTURE)
    return g, {str(n): ga.DeviceModel(_model(ga, g, None, str(n))) for n in g["geoms"]}


def _cases():
    g = load_golden(FIXTURE)
    return [(str(n), k) for n in g["geoms"] for k in range(len(g[str(n) + "_cases"]))]


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name,k", _cases())
def test_fixture_cases(fixture_models, name, k, form):
    """X, Y and n_switches of every option set equal the REFERENCE's gnofix() (case 0 of a geometry: no option, the old entry)"""
    import torch
    g, models = fixture_models
    dev = models[name]
    opt = json.loads(str(g[name + "_cases"][k]))
    X, B = g[name + "_X"], g[name + "_B"]
    if form == "host":
        Xo, Y, nsw = dev.gnofix(X, B, **opt)
    else:
        Xt, Bt = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(B).cuda()
        Yt, nt = dev.gnofix_device(Xt, Bt, **opt)
        Xo, Y, nsw = Xt.cpu().numpy(), Yt.cpu().numpy(), nt.cpu().numpy()
    assert np.array_equal(Xo, g["%s_%d_oX" % (name, k)])
    assert np.array_equal(Y, g["%s_%d_oY" % (name, k)])
    assert np.array_equal(nsw, g["%s_%d_nhist" % (name, k)] - 2)


# (S, W, A, M, rem): W in {2S, 2S+1, 3S+2}; M = 2 is the smallest window the loader takes (C % M != 0 rules out M = 1); rem >= W (the last
# two) makes gnofix's window size C // W = M + 1 differ from the model's M; every C leaves a ragged last window
FUZZ_GEOMS = [(3, 6, 2, 2, 1), (3, 7, 3, 3, 2), (3, 11, 7, 2, 1), (5, 10, 3, 2, 1), (5, 11, 7, 8, 7), (5, 17, 2, 3, 1),
              (9, 18, 7, 2, 1), (9, 19, 2, 5, 4), (9, 29, 3, 8, 7), (5, 10, 2, 9, 8), (5, 10, 2, 13, 12), (3, 7, 3, 9, 8)]
FUZZ_SEEDS = 40
FUZZ_IND = 6
CHECKS = ["disc_smooth", "all", "disc_base", "disc_either"]


def _fuzz_options(rng, S):
    half = (S - 1) // 2
    return dict(check_criterion=CHECKS[rng.randint(4)], max_center_offset=int(rng.randint(half + 1)), non_lin_s=int(rng.randint(half + 1)),
                prob_comp=["max", "prod"][rng.randint(2)], prior_switch_prob=float([0.5, 0.3, 0.45, 0.55, 0.7][rng.randint(5)]),
                padding=bool(rng.randint(2)))


def fuzz_case(seed):
    """the inputs of fuzz seed `seed` (no GPU): geometry, tree arrays, options, max_it, X, B"""
    from gnomix_amd import synth
    rng = np.random.RandomState(7000 + seed)
    S, W, A, M, rem = FUZZ_GEOMS[seed % len(FUZZ_GEOMS)]
    Cn = W * M + rem
    depth, max_it = 2 + seed % 3, [2, 3, 6][seed % 3]
    trees = synth.synthetic_trees(2 + seed % 4, A, S * A, depth=depth, seed=seed, thr_lo=0.0, thr_hi=0.7, leaf_scale=1.0)
    opt = _fuzz_options(rng, S)
    if opt == dict(check_criterion="disc_smooth", max_center_offset=0, non_lin_s=0, prob_comp="max", prior_switch_prob=0.5, padding=True):
        opt["prob_comp"] = "prod"  # the fuzz is about the new kernel
    X = rng.randint(0, 3, size=(2 * FUZZ_IND, Cn)).astype(np.int8)
    X[2:4] = X[2:3]  # identical haplotypes: nothing ever changes X_m (the convergence stop)
    B = rng.dirichlet(np.ones(A) * 0.5, size=(2 * FUZZ_IND, W))
    return (S, W, A, M, Cn), trees, opt, max_it, X, B


def fuzz_reference(oracle, seed, events=None, stats=None):
    """the restatement's results for every individual of fuzz seed `seed`"""
    (S, W, A, M, Cn), trees, opt, max_it, X, B = fuzz_case(seed)
    T = oracle.Trees(trees["tree_off"], trees["left"], trees["right"], trees["feat"], trees["cond"], trees["tree_class"], A, 0.5)
    rows = lambda r: oracle.xgb_predict_proba(T, np.asarray(r, dtype=np.float32))
    labs = lambda b: oracle.smooth_xgb(T, b, S)[1]
    out = []
    for i in range(FUZZ_IND):
        st = {}
        out.append(gnofix_opts(X[2 * i], X[2 * i + 1], B[2 * i:2 * i + 2], S, rows, labs, max_it=max_it, events=events, stats=st, **opt))
        if stats is not None:
            stats.append(st)
    return out


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_against_the_restatement(ga, oracle, seed):
    """tests/test_gnofix_opts_host.py asserts (without a GPU) that these seeds reach the iteration cap, the convergence stop, accepted
    double switches, switches at window 0 and a window size that differs from M"""
    (S, W, A, M, Cn), trees, opt, max_it, X, B = fuzz_case(seed)
    d = ga.GnxModelData(C=Cn, M=M, A=A, S=S, context=0, smooth_kind="xgb")
    for key, v in trees.items():
        setattr(d, key, v)
    assert d.base_score == 0.5
    dev = ga.DeviceModel(d)
    Xo, Y, nsw = dev.gnofix(X, B, max_it=max_it, **opt)
    for i, (Xm, Xp, Ym, Yp, _, ns) in enumerate(fuzz_reference(oracle, seed)):
        assert np.array_equal(Xo[2 * i], Xm) and np.array_equal(Xo[2 * i + 1], Xp), (i, opt)
        assert np.array_equal(Y[2 * i], Ym) and np.array_equal(Y[2 * i + 1], Yp), (i, opt)
        assert int(nsw[i]) == ns, (i, opt)


def _opts(**kw):
    from gnomix_amd import _lib
    return _lib.gnofix_opts(**kw)


def _call_ex(dev, X, B, o, Y, nsw, form="host"):
    if form == "host":
        return dev.lib.gnx_gnofix_ex(dev.h, X.ctypes.data, X.shape[1], B.ctypes.data, X.shape[0] // 2, C.byref(o), Y.ctypes.data, nsw.ctypes.data)
    return dev.lib.gnx_gnofix_ex_dev(dev.h, X.data_ptr(), X.stride(0), B.data_ptr(), X.shape[0] // 2, C.byref(o), Y.data_ptr(), nsw.data_ptr())


def test_default_options_are_the_old_entry(fixture_models):
    """defaults through _ex and _ex_dev: bit-identical to gnx_gnofix on the same inputs"""
    import torch
    g, models = fixture_models
    for name in ("s5", "g5"):
        dev = models[name]
        X, B = g[name + "_X"], g[name + "_B"]
        X0, Y0, n0 = dev.gnofix(X, B, max_it=5)
        X1 = X.copy()
        Y1, n1 = np.full(Y0.shape, -7, np.int32), np.full(n0.shape, -7, np.int32)
        assert _call_ex(dev, X1, np.ascontiguousarray(B), _opts(max_it=5), Y1, n1) == 0
        assert np.array_equal(X1, X0) and np.array_equal(Y1, Y0) and np.array_equal(n1, n0)
        Xt, Bt = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(B).cuda()
        Yt, nt = torch.full(Y0.shape, -7, dtype=torch.int32, device="cuda"), torch.full(n0.shape, -7, dtype=torch.int32, device="cuda")
        dev._bind_torch_stream()
        assert _call_ex(dev, Xt, Bt, _opts(max_it=5), Yt, nt, "dev") == 0
        torch.cuda.synchronize()
        assert np.array_equal(Xt.cpu().numpy(), X0) and np.array_equal(Yt.cpu().numpy(), Y0) and np.array_equal(nt.cpu().numpy(), n0)


def _bad_options(S):
    from gnomix_amd import _lib
    half = (S - 1) // 2
    bad = []
    for field, value in [("check_criterion", 4), ("check_criterion", -1), ("prob_comp", 2), ("prob_comp", -1), ("max_center_offset", half + 1),
                         ("max_center_offset", -1), ("non_lin_s", half + 1), ("non_lin_s", -1), ("max_it", -1), ("struct_bytes", 32),
                         ("struct_bytes", 48), ("prior_switch_prob", 0.0), ("prior_switch_prob", 1.0), ("prior_switch_prob", float("nan")),
                         ("prior_switch_prob", float("inf")), ("prior_switch_prob", -0.25)]:
        o = _lib.gnofix_opts(max_it=3, non_lin_s=1)
        setattr(o, field, value)
        bad.append((field, value, o))
    return bad


def _assert_refused(dev, X, B, o, code, what):
    import torch
    X1, Y, nsw = X.copy(), np.full((X.shape[0], dev.W), -7, np.int32), np.full((X.shape[0] // 2,), -7, np.int32)
    assert _call_ex(dev, X1, B, o, Y, nsw) == code, what
    assert dev.lib.gnx_last_error(dev.ctx.h), what  # with a message
    assert np.array_equal(X1, X) and (Y == -7).all() and (nsw == -7).all(), what
    Xt, Bt = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(B).cuda()
    Yt = torch.full((X.shape[0], dev.W), -7, dtype=torch.int32, device="cuda")
    nt = torch.full((X.shape[0] // 2,), -7, dtype=torch.int32, device="cuda")
    dev._bind_torch_stream()
    assert _call_ex(dev, Xt, Bt, o, Yt, nt, "dev") == code, what
    torch.cuda.synchronize()
    assert np.array_equal(Xt.cpu().numpy(), X) and bool((Yt == -7).all()) and bool((nt == -7).all()), what


def test_invalid_options_are_refused(fixture_models):
    from gnomix_amd import _lib
    g, models = fixture_models
    dev = models["s5"]
    X, B = g["s5_X"], np.ascontiguousarray(g["s5_B"])
    for field, value, o in _bad_options(5):
        _assert_refused(dev, X, B, o, _lib.GNX_EINVAL, (field, value))
    # the context still works, and so does the model
    Xo, Y, nsw = dev.gnofix(X, B, max_it=6, non_lin_s=2)
    assert np.array_equal(Xo, g["s5_5_oX"]) and np.array_equal(Y, g["s5_5_oY"])


def test_unsupported_models_are_refused(ga, monkeypatch):
    from gnomix_amd import _lib, synth
    g = load_golden(FIXTURE)
    X, B = g["s5_X"], np.ascontiguousarray(g["s5_B"])
    o = _lib.gnofix_opts(max_it=3, non_lin_s=1)
    # 1) a smoother that is not the tree smoother
    W, A = int(g["s5_W"]), int(g["s5_A"])
    rng = np.random.RandomState(1)
    crf = ga.GnxModelData(C=int(g["s5_C"]), M=int(g["s5_C"]) // W, A=A, S=5, context=0, smooth_kind="crf",
                          crf_state=rng.standard_normal((A, A)), crf_trans=rng.standard_normal((A, A)))
    dev = ga.DeviceModel(crf)
    _assert_refused(dev, X, B, o, _lib.GNX_EUNSUPPORTED, "crf")
    _assert_refused(dev, X, B, _lib.gnofix_opts(max_it=3), _lib.GNX_EUNSUPPORTED, "crf, default options")
    assert dev.smooth_predict(B)[1].shape == (X.shape[0], W)  # the context still works
    # 2) a model the float32 kernel serves: no options there; the defaults still run
    monkeypatch.setenv("GNX_GNOFIX_IMPL", "f32")
    ctx = _lib.Context(0)
    try:
        dev = ga.DeviceModel(_model(ga, g, None, "s5"), ctx=ctx)
        _assert_refused(dev, X, B, o, _lib.GNX_EUNSUPPORTED, "f32 fallback")
        Xo, Y, nsw = dev.gnofix(X, B, max_it=6)
        assert np.array_equal(Xo, g["s5_0_oX"]) and np.array_equal(Y, g["s5_0_oY"])
        Y1, n1 = np.full(Y.shape, -7, np.int32), np.full(nsw.shape, -7, np.int32)
        X1 = X.copy()
        assert _call_ex(dev, X1, B, _lib.gnofix_opts(max_it=6), Y1, n1) == 0   # default options: the fallback, as gnx_gnofix
        assert np.array_equal(X1, Xo) and np.array_equal(Y1, Y) and np.array_equal(n1, nsw)
    finally:
        ctx.close()
    monkeypatch.delenv("GNX_GNOFIX_IMPL")
    # 3) a geometry beyond the kernel's LDS: 12 bytes per window
    Wb, Ab, Sb = 16000, 2, 3
    big = ga.GnxModelData(C=Wb * 2 + 1, M=2, A=Ab, S=Sb, context=0, smooth_kind="xgb")
    for key, v in synth.synthetic_trees(2, Ab, Sb * Ab, depth=2, seed=1).items():
        setattr(big, key, v)
    dev = ga.DeviceModel(big)
    Xb = rng.randint(0, 2, size=(2, big.C)).astype(np.int8)
    Bb = rng.dirichlet(np.ones(Ab), size=(2, Wb))
    _assert_refused(dev, Xb, Bb, o, _lib.GNX_EUNSUPPORTED, "W = 16000")
    assert dev.smooth_predict(Bb)[1].shape == (2, Wb)


def test_phase_passes_the_options(ga, fixture_models):
    g, models = fixture_models
    hip = ga.HipGnomix(_model(ga, g, None, "g5"))
    X, B = g["g5_X"], g["g5_B"]
    Xph, Yph = hip.phase(X, B=B, non_lin_s=2, prior_switch_prob=0.55, max_it=4)
    Xo, Y, _ = models["g5"].gnofix(X, B, max_it=4, non_lin_s=2, prior_switch_prob=0.55)
    assert np.array_equal(Xph, Xo) and np.array_equal(Yph, Y)
    Xd, Yd = hip.phase(X, B=B)
    assert not (np.array_equal(Xd, Xph) and np.array_equal(Yd, Yph))  # the options reached the loop
    with pytest.raises(NotImplementedError, match="naive_switch"):
        hip.phase(X, B=B, naive_switch=2)
