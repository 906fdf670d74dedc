"""-m gpu: the HIP path (through the C ABI) against the oracle and the golden vectors.

Bars (BASELINE.json north_star): argmax labels bit-identical; probabilities within 1e-5.
For the f32 tree pass we additionally assert BIT equality with the oracle (same f32 order of
operations), and for the f64 logistic base <= 1e-12 absolute on B with the float32 cast that the
smoother consumes differing in at most a handful of entries (MFMA summation order != sequential)."""
import os

import numpy as np
import pytest

from conftest import load_golden, trees_from_npz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _close_f32(got, ref):
    """The f32 tree walk and margin sums are bit-exact; the only divergence allowed is the last bit
    of expf (device: float(exp(double)), correctly rounded; glibc expf: <= 0.502 ulp, i.e. differs
    from correct rounding for < 0.5 % of arguments) and its knock-on through sum and division."""
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 2.4e-7          # <= 2 ulp at 1.0; the stated bar is 1e-5
    assert np.count_nonzero(got != ref) <= max(3, got.size // 20)


def _oracle_trees(O, d):
    return O.Trees(d.tree_off, d.left, d.right, d.feat, d.cond, d.tree_class, d.A, d.base_score)


def _lr_data(ga, C, M, A, ctx, seed):
    from gnomix_amd import synth
    return synth.synthetic_model(C=C, M=M, A=A, S=5, context=ctx, seed=seed, smooth=None)


# ---------------------------------------------------------------- logistic base ------------------
@pytest.fixture(params=["i8", "i8dl", "f64"])
def lr_impl(request, monkeypatch):
    """every shipped variant of the logistic pass on every geometry: exact int8-limb fixed point with register-staged loads
    (k_base_logistic_i8), the same arithmetic with LDS-direct loads (k_base_logistic_i8_dl), and f64 MFMA.  Launch knobs are read
    once per context, so each variant gets a context of its own.  (The measured-slower structures of DESIGN.md 5.2 were removed from the
    tree; their sources are at commit 8235b46.)"""
    from gnomix_amd import _lib
    monkeypatch.setenv("GNX_BASE_LR_IMPL", "f64" if request.param == "f64" else "i8")
    monkeypatch.setenv("GNX_LR_DL", "1" if request.param == "i8dl" else "0")
    return _lib.Context(0)


def test_base_golden_G1(ga, oracle, lr_impl):
    g = load_golden("G1_lr.npz")
    d = ga.GnxModelData(C=int(g["C"]), M=int(g["M"]), A=int(g["A"]), S=5, context=int(g["ctx"]), base_kind="logistic",
                        lr_coef=g["coef"], lr_intercept=g["intercept"])
    dev = ga.DeviceModel(d, ctx=lr_impl)
    b32, b64 = dev.base_predict(g["X"], want_f32=True, want_f64=True)
    assert np.max(np.abs(b64 - g["B"])) < 1e-12          # vs the REFERENCE's own output
    assert np.array_equal(np.argmax(b64, -1), np.argmax(g["B"], -1))
    assert np.count_nonzero(b32 != g["B"].astype(np.float32)) <= 2
    assert np.array_equal(b32, b64.astype(np.float32))


def test_base_golden_G15_binary(ga, lr_impl):
    """A = 2 logistic base against the REFERENCE's own output (sklearn's one-row binary form, see G15 in make_golden.py)"""
    g = load_golden("G15_lr_binary.npz")
    d = ga.GnxModelData(C=int(g["C"]), M=int(g["M"]), A=2, S=5, context=int(g["ctx"]), base_kind="logistic",
                        lr_coef=g["coef"], lr_intercept=g["intercept"])
    dev = ga.DeviceModel(d, ctx=lr_impl)
    b32, b64 = dev.base_predict(g["X"], want_f32=True, want_f64=True)
    assert np.max(np.abs(b64 - g["B"])) < 1e-12
    assert np.array_equal(np.argmax(b64, -1), np.argmax(g["B"], -1))
    assert np.count_nonzero(b32 != g["B"].astype(np.float32)) <= 2


@pytest.mark.parametrize("C,M,A,ctx,N", [
    (4037, 100, 7, 50, 24),      # default context ratio 0.5
    (4037, 100, 7, 0, 5),        # no context
    (2531, 100, 3, 30, 70),      # ratio 0.3: windows end mid-piece
    (1999, 64, 2, 32, 130),      # M multiple of 64
    (3001, 100, 12, 50, 33),     # A=12: 24 columns -> 2 MFMA column tiles (flat: 11 tiles instead of 14)
    (2201, 100, 9, 50, 600),     # A=9: 18 slots -> 8 flat tiles instead of 14; more rows than one block
    (1801, 60, 7, 45, 50),       # ratio 0.75: R = 3 windows per SNP, 21 slots -> 10 flat tiles
    (1503, 100, 16, 50, 9),      # A=16
    (2777, 100, 5, 120, 40),     # ratio 1.2: 4 windows per SNP, left/right reflection reaches window 1
    (1237, 50, 7, 25, 600),      # more haplotypes than one 64-row wave tile; exercises MT=4 kernels
    (1237, 50, 7, 25, 1),        # a single haplotype
    (937, 300, 4, 150, 66),      # W=3 windows only
])
def test_base_vs_oracle(ga, oracle, lr_impl, C, M, A, ctx, N):
    from gnomix_amd import synth
    d = _lr_data(ga, C, M, A, ctx, seed=C + A)
    X = synth.synthetic_X(N, C, seed=N, miss=0.03)
    dev = ga.DeviceModel(d, ctx=lr_impl)
    b32, b64 = dev.base_predict(X, want_f32=True, want_f64=True)
    ref = oracle.base_lr(X, M, ctx, d.lr_coef, d.lr_intercept)
    assert b64.shape == ref.shape
    assert np.max(np.abs(b64 - ref)) < 1e-12
    assert np.array_equal(np.argmax(b64, -1), np.argmax(ref, -1))
    assert np.count_nonzero(b32 != ref.astype(np.float32)) <= max(2, ref.size // 100000)
    assert np.allclose(b64.sum(-1), 1.0, atol=1e-12)


def test_base_transpose_detecting(ga, oracle, lr_impl):
    """asymmetric weights + one-hot haplotypes: catches row/column swaps in the MFMA C/D mapping"""
    C, M, A, ctx = 1037, 100, 7, 50
    d = _lr_data(ga, C, M, A, ctx, seed=1)
    W = C // M
    d.lr_coef = np.zeros_like(d.lr_coef)
    d.lr_intercept = np.zeros_like(d.lr_intercept)
    for w in range(W):
        for a in range(A):
            d.lr_coef[w, a, :] = 0.001 * (a + 1) * (1 + (np.arange(d.lr_coef.shape[2]) % 13)) * (1 if (w + a) % 2 else -1)
    X = np.zeros((80, C), dtype=np.int8)
    for n in range(80):
        X[n, (n * 37) % C::(n + 3)] = 1 + (n % 2)
    dev = ga.DeviceModel(d, ctx=lr_impl)
    _, b64 = dev.base_predict(X)
    ref = oracle.base_lr(X, M, ctx, d.lr_coef, d.lr_intercept)
    assert np.max(np.abs(b64 - ref)) < 1e-13


def test_base_rejects_bad_geometry(ga):
    from gnomix_amd import synth
    d = synth.synthetic_model(C=1037, M=100, A=7, S=5, smooth=None)
    d.C = 1000  # C % M == 0 (base.py:158)
    d.lr_coef = d.lr_coef[:10]
    d.lr_intercept = d.lr_intercept[:10]
    with pytest.raises(ga.GnxError):
        ga.DeviceModel(d)
    d2 = synth.synthetic_model(C=1037, M=100, A=7, S=5, smooth=None)
    dev = ga.DeviceModel(d2)
    with pytest.raises(ValueError):
        dev.base_predict(np.zeros((3, 999), dtype=np.int8))


def test_base_empty_input(ga):
    from gnomix_amd import synth
    d = synth.synthetic_model(C=1037, M=100, A=7, S=5, smooth=None)
    dev = ga.DeviceModel(d)
    _, b = dev.base_predict(np.zeros((0, 1037), dtype=np.int8))
    assert b.shape == (0, 10, 7)


# ---------------------------------------------------------------- xgb smoother ---------------------
def test_smooth_golden_G4(ga, oracle):
    g = load_golden("G4_smooth.npz")
    N, W, A = g["B"].shape
    S = int(g["S"])
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="xgb", tree_off=g["t_tree_off"],
                        left=g["t_left"], right=g["t_right"], feat=g["t_feat"], cond=g["t_cond"],
                        tree_class=g["t_tree_class"], base_score=float(g["t_base_score"]))
    dev = ga.DeviceModel(d)
    proba, lab = dev.smooth_predict(g["B"])
    assert np.array_equal(lab, g["labels"])
    _close_f32(proba, g["proba"])


@pytest.mark.parametrize("N,W,A,S,rounds,depth", [
    (5, 163, 7, 75, 6, 4),
    (33, 370, 7, 75, 10, 4),     # chr22 window count, ragged last strip (370 = 5*64 + 50)
    (17, 200, 3, 75, 8, 4),
    (9, 150, 12, 75, 5, 4),      # A=12 (config 5)
    (40, 64, 4, 31, 7, 4),       # exactly one strip
    (3, 65, 2, 31, 9, 3),        # shallow trees -> runtime-depth kernel
    (6, 90, 5, 41, 4, 6),        # deep trees
    (1, 160, 7, 75, 20, 4),      # single haplotype
    (70, 130, 8, 61, 3, 4),      # even A (bank-conflicted layout, same results)
])
def test_smooth_vs_oracle(ga, oracle, N, W, A, S, rounds, depth):
    from gnomix_amd import synth
    rng = np.random.RandomState(N * W + A)
    B = rng.dirichlet(np.ones(A) * 0.4, size=(N, W))
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(rounds, A, S * A, depth=depth, seed=W, thr_lo=0.0, thr_hi=0.7, p_early_leaf=0.2).items():
        setattr(d, k, v)
    dev = ga.DeviceModel(d)
    T = _oracle_trees(oracle, d)
    p_ref, l_ref = oracle.smooth_xgb(T, B, S)
    for Bin in (B, B.astype(np.float32)):
        p_ref, l_ref = oracle.smooth_xgb(T, Bin, S)
        proba, lab = dev.smooth_predict(Bin)
        assert np.array_equal(lab, l_ref)
        _close_f32(proba, p_ref)
    p64, _ = dev.smooth_predict(B, proba_dtype=np.float64)
    p32, _ = dev.smooth_predict(B)
    assert np.array_equal(p64, p32.astype(np.float64))


def test_smooth_rows_vs_oracle(ga, oracle):
    from gnomix_amd import synth
    A, S = 7, 75
    d = ga.GnxModelData(C=1603, M=10, A=A, S=S, context=5, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(15, A, S * A, seed=2).items():
        setattr(d, k, v)
    dev = ga.DeviceModel(d)
    rows = np.random.RandomState(0).uniform(size=(37, S * A)).astype(np.float32)
    _close_f32(dev.smooth_rows(rows), oracle.xgb_predict_proba(_oracle_trees(oracle, d), rows))


def test_smoother_too_large_is_rejected(ga):
    from gnomix_amd import synth
    d = ga.GnxModelData(C=1003, M=10, A=3, S=75, context=5, smooth_kind="xgb")  # W=100 < 2*S (models.py:13)
    for k, v in synth.synthetic_trees(2, 3, 75 * 3).items():
        setattr(d, k, v)
    with pytest.raises(ga.GnxError, match="Smoother size to large"):
        ga.DeviceModel(d)


# ---------------------------------------------------------------- whole path ------------------------
@pytest.mark.parametrize("C,M,A,S,N", [(16037, 100, 7, 75, 50), (9531, 50, 4, 31, 21), (20011, 100, 12, 75, 12)])
def test_infer_vs_oracle(ga, oracle, C, M, A, S, N):
    from gnomix_amd import synth
    d = synth.synthetic_model(C=C, M=M, A=A, S=S, n_rounds=15, seed=C)
    X = synth.synthetic_X(N, C, seed=5, miss=0.02)
    g = ga.HipGnomix(d)
    proba = g.predict_proba(X)
    labels = g.predict(X)
    B = oracle.base_lr(X, M, d.context, d.lr_coef, d.lr_intercept)
    p_ref, l_ref = oracle.smooth_xgb(_oracle_trees(oracle, d), B, S)
    assert labels.dtype == np.int64 and proba.dtype == np.float32
    assert np.array_equal(labels, l_ref)
    assert np.max(np.abs(proba - p_ref)) <= 1e-5
    # plugin-style use, as run_inference does it (gnomix.py:55-58)
    Bq = g.base.predict_proba(X)
    assert Bq.dtype == np.float64 and np.max(np.abs(Bq - B)) < 1e-12
    yp = g.smooth.predict_proba(Bq)
    assert np.array_equal(np.argmax(yp, axis=-1), l_ref)
    assert np.array_equal(g.smooth.predict(Bq), l_ref)


def test_full_size_properties_chr22(ga, oracle):
    """BASELINE config-2 shape (C=370500, W=370, A=7, S=75, 700 trees): size-independent properties +
    a sample of haplotypes against the oracle."""
    import torch
    from gnomix_amd import synth
    d = synth.synthetic_model(seed=0, **synth.CHR22)
    dev = ga.DeviceModel(d)
    N = 512
    Xd = synth.synthetic_X_device(N, d.C, "cuda:0", seed=94305)
    p, lab = dev.infer_device(Xd)
    torch.cuda.synchronize()
    p, lab = p.cpu().numpy(), lab.cpu().numpy()
    assert np.allclose(p.sum(-1), 1.0, atol=2e-6)
    assert np.array_equal(lab, np.argmax(p, -1))
    # permutation equivariance + batch-split independence (bit-exact)
    perm = torch.randperm(N, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1))
    p2, lab2 = dev.infer_device(Xd[perm].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(p2.cpu().numpy(), p[perm.cpu().numpy()])
    p3, _ = dev.infer_device(Xd[100:137])
    torch.cuda.synchronize()
    assert np.array_equal(p3.cpu().numpy(), p[100:137])
    # strided rows (ldx > C)
    Xs = torch.zeros((8, d.C + 77), dtype=torch.int8, device="cuda:0")
    Xs[:, :d.C] = Xd[:8]
    p4, _ = dev.infer_device(Xs[:, :d.C])
    torch.cuda.synchronize()
    assert np.array_equal(p4.cpu().numpy(), p[:8])
    # oracle on a sample
    idx = [0, 1, 255, 511]
    Xh = Xd[idx].cpu().numpy()
    B = oracle.base_lr(Xh, d.M, d.context, d.lr_coef, d.lr_intercept)
    p_ref, l_ref = oracle.smooth_xgb(_oracle_trees(oracle, d), B, d.S)
    assert np.array_equal(lab[idx], l_ref)
    assert np.max(np.abs(p[idx] - p_ref)) <= 1e-5


# ---------------------------------------------------------------- crf smoother ----------------------
@pytest.mark.parametrize("impl", ["", "scan", "lanes", "fused"])   # default = one haplotype per DPP row up to 16 labels
@pytest.mark.parametrize("N,W,A", [(5, 40, 7), (70, 370, 7), (33, 150, 12), (9, 97, 2), (1, 30, 3), (40, 64, 16), (21, 83, 9), (12, 70, 14), (6, 51, 20), (3, 5, 11), (130, 33, 4)])
def test_crf_vs_oracle(ga, oracle, monkeypatch, N, W, A, impl):
    from gnomix_amd import _lib
    rng = np.random.RandomState(N + W)
    B = rng.dirichlet(np.ones(A) * 0.5, size=(N, W))
    state = rng.standard_normal((A, A)) * 2 + 4 * np.eye(A)
    trans = rng.standard_normal((A, A)) * 0.5 + 3 * np.eye(A)
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=75, context=5, smooth_kind="crf", crf_state=state, crf_trans=trans)
    if impl:
        if impl == "fused":
            monkeypatch.setenv("GNX_CRF_FLAGS", "1")   # the row kernel computes psi itself
        else:
            monkeypatch.setenv("GNX_CRF_IMPL", impl)   # read once, at gnx_init
        dev = ga.DeviceModel(d, ctx=_lib.Context(0))
    else:
        dev = ga.DeviceModel(d)
    p_ref, l_ref = oracle.smooth_crf(B, state, trans)
    p, lab = dev.smooth_predict(B)
    assert p.dtype == np.float64
    assert np.max(np.abs(p - p_ref)) < 1e-11
    assert np.array_equal(lab, l_ref)
    assert np.allclose(p.sum(-1), 1.0, atol=1e-10)
    p32, _ = dev.smooth_predict(B, proba_dtype=np.float32)
    assert np.array_equal(p32, p.astype(np.float32))
    sm = ga.HipSmoother(dev)
    assert sm.gnofix is False and np.array_equal(sm.predict(B), l_ref)


@pytest.mark.parametrize("scale", [2.0, 5.0, 10.0, 20.0, 40.0])   # forward scale every 8th, 8th or 4th, 4th or 2nd, 2nd, every window
@pytest.mark.parametrize("W,A", [(133, 12), (61, 5)])
def test_crf_weights_far_beyond_a_trained_model(ga, oracle, scale, W, A):
    """the default kernel takes the forward scale every eighth window only (k_smooth_crf_ck, norm_mask): weights 10x and 40x a trained
    model's (per-window factors down to e^-160) must still give the oracle's marginals — the oracle rescales at every window."""
    rng = np.random.RandomState(int(scale) + W)
    N = 37
    B = rng.dirichlet(np.ones(A) * 0.3, size=(N, W))
    state = rng.standard_normal((A, A)) * scale
    trans = rng.standard_normal((A, A)) * scale
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=75, context=5, smooth_kind="crf", crf_state=state, crf_trans=trans)
    dev = ga.DeviceModel(d)
    p_ref, l_ref = oracle.smooth_crf(B, state, trans)
    assert np.isfinite(p_ref).all()
    p, lab = dev.smooth_predict(B)
    assert np.isfinite(p).all() and np.max(np.abs(p - p_ref)) < 1e-9
    clear = np.sort(p_ref, -1)[..., -1] - np.sort(p_ref, -1)[..., -2] > 1e-9
    assert np.array_equal(lab[clear], l_ref[clear])


def test_crf_end_to_end_and_no_phasing(ga, oracle):
    from gnomix_amd import synth
    d = synth.synthetic_model(C=12037, M=100, A=12, S=75, seed=4, smooth="crf")
    X = synth.synthetic_X(30, d.C, seed=2)
    g = ga.HipGnomix(d)
    p = g.predict_proba(X)
    B = oracle.base_lr(X, d.M, d.context, d.lr_coef, d.lr_intercept)
    p_ref, l_ref = oracle.smooth_crf(B, d.crf_state, d.crf_trans)
    assert np.max(np.abs(p - p_ref)) < 1e-9
    assert np.array_equal(g.predict(X), l_ref)
    with pytest.raises(AssertionError, match="does not currently support re-phasing"):  # src/model.py:194
        g.phase(X)


# ---------------------------------------------------------------- gnofix ----------------------------
@pytest.fixture(params=["rk512", "rk256", "rk1024", "f32"])
def gnofix_ctx(request, monkeypatch):
    """every Gnofix kernel on every case: the rank-strip kernel (k_gnofix.hip) with 512 (default), 256 and 1024 threads per
    individual, and the float32-strip kernel of rounds 1-3 (k_gnofix_f32.hip: the fallback for ensembles without a rank copy).
    The knobs are read once per context."""
    from gnomix_amd import _lib
    if request.param == "f32":
        monkeypatch.setenv("GNX_GNOFIX_IMPL", "f32")
    else:
        monkeypatch.setenv("GNX_GNOFIX_IMPL", "rk")
        monkeypatch.setenv("GNX_GNOFIX_T", request.param[2:])
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def _gnofix_model(ga, g, prefix):
    W, A, S, C = int(g["W"]), int(g["A"]), int(g["S"]), int(g["C"])
    return ga.GnxModelData(C=C, M=C // W, A=A, S=S, context=0, smooth_kind="xgb", tree_off=g[prefix + "tree_off"],
                           left=g[prefix + "left"], right=g[prefix + "right"], feat=g[prefix + "feat"],
                           cond=g[prefix + "cond"], tree_class=g[prefix + "tree_class"],
                           base_score=float(g[prefix + "base_score"]))


@pytest.mark.parametrize("name", ["none", "one", "two", "edges", "many", "rand"])
def test_gnofix_golden_G5(ga, name, gnofix_ctx):
    g = load_golden("G5_gnofix.npz")
    dev = ga.DeviceModel(_gnofix_model(ga, g, "r_" if name == "rand" else "t_"), ctx=gnofix_ctx)
    X = np.stack([g[name + "_Xm"], g[name + "_Xp"]]).astype(np.int8)
    Xo, Y, nsw = dev.gnofix(X, g[name + "_B"], max_it=4 if name == "rand" else 50)
    assert np.array_equal(Xo[0], g[name + "_oXm"]) and np.array_equal(Xo[1], g[name + "_oXp"])   # vs the REFERENCE's gnofix()
    assert np.array_equal(Y[0], g[name + "_oYm"]) and np.array_equal(Y[1], g[name + "_oYp"])
    assert int(nsw[0]) == int(g[name + "_nhist"]) - 2


def test_phase_wrapper_golden_G5(ga):
    g = load_golden("G5_gnofix.npz")
    hip = ga.HipGnomix(_gnofix_model(ga, g, "t_"))
    Xph, Yph = hip.phase(g["phase_X"], B=g["phase_B"])
    assert np.array_equal(Xph, g["phase_oX"]) and np.array_equal(Yph, g["phase_oY"])  # vs reference Gnomix.phase()


def test_gnofix_vs_oracle_random_individuals(ga, oracle, gnofix_ctx):
    """more individuals, chaotic smoother: many accepted switches, edge windows, max_it stops"""
    from gnomix_amd import synth
    W, A, S = 170, 5, 75
    C = W * 7 + 5
    d = ga.GnxModelData(C=C, M=7, A=A, S=S, context=0, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(6, A, S * A, seed=3, thr_lo=0.0, thr_hi=0.6, leaf_scale=1.0).items():
        setattr(d, k, v)
    dev = ga.DeviceModel(d, ctx=gnofix_ctx)
    T = _oracle_trees(oracle, d)
    rng = np.random.RandomState(0)
    n_ind = 12
    X = rng.randint(0, 3, size=(2 * n_ind, C)).astype(np.int8)
    X[6:8, :] = X[6:7, :]          # an individual with identical haplotypes (convergence signature path)
    B = rng.dirichlet(np.ones(A) * 0.3, size=(2 * n_ind, W))
    Xo, Y, nsw = dev.gnofix(X, B, max_it=6)
    rows = lambda r: oracle.xgb_predict_proba(T, r)
    labs = lambda b: oracle.smooth_xgb(T, b, S)[1]
    tot = 0
    for i in range(n_ind):
        Xm, Xp, Ym, Yp, _, ns = oracle.gnofix(X[2 * i], X[2 * i + 1], B[2 * i:2 * i + 2], S, rows, labs, max_it=6)
        assert np.array_equal(Xo[2 * i], Xm) and np.array_equal(Xo[2 * i + 1], Xp), i
        assert np.array_equal(Y[2 * i], Ym) and np.array_equal(Y[2 * i + 1], Yp), i
        assert int(nsw[i]) == ns
        tot += ns
    assert tot > 10  # the case really exercises accepted switches


# ---------------------------------------------------------------- CovRSK / SVC base ------------------
def _svc_oracle_windows(d):
    return [dict(Xfit=w["xfit"], Ms=list(w["ms"]), support=w["support"], dual=w["dual_coef"], intercept=w["intercept"],
                 probA=w["prob_a"], probB=w["prob_b"], n_support=w["n_support"]) for w in d.svc]


def test_covrsk_golden_G2(ga, oracle):
    from gnomix_amd import convert
    g = load_golden("G2_covrsk.npz")
    C, M, A, ctx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    W = C // M
    d = ga.GnxModelData(C=C, M=M, A=A, S=5, context=ctx, base_kind="covrsk")
    d.svc = []
    for i in range(W):
        xf = g["w%d_Xfit" % i]
        d.svc.append(dict(xfit=xf, support=g["w%d_support" % i], dual_coef=g["w%d_dual" % i], intercept=g["w%d_intercept" % i],
                          prob_a=g["w%d_probA" % i], prob_b=g["w%d_probB" % i], n_support=g["w%d_nsv" % i],
                          ms=convert.cov_sample(xf.shape[1])))
    dev = ga.DeviceModel(d)
    b32, b64 = dev.base_predict(g["X"], want_f32=True, want_f64=True)
    assert np.max(np.abs(b64 - g["B"])) < 1e-12          # vs the REFERENCE's CovRSKBase.predict_proba
    assert np.array_equal(np.argmax(b64, -1), np.argmax(g["B"], -1))
    assert np.array_equal(b32, b64.astype(np.float32))


@pytest.mark.parametrize("C,M,A,ctx,N,nfit", [
    (1537, 100, 3, 50, 70, 12),       # width 200 = 7 words (partial last word), last window 237
    (3511, 175, 7, 87, 130, 20),      # config-3 geometry: M=175, width 349 -> Ms = [1,4,8,39,42,117]
    (1029, 64, 4, 32, 5, 8),          # width 128: exact multiple of 32
    (2011, 500, 2, 250, 33, 30),      # width 1000 (>866: all eight canonical lengths), binary problem
    (1237, 50, 12, 25, 64, 6),        # A=12
    (1711, 200, 3, 100, 40, 10),      # width 400 (13 words): all seven lengths of the AND-shift fast path, incl. 376
])
def test_covrsk_vs_oracle(ga, oracle, C, M, A, ctx, N, nfit):
    from gnomix_amd import synth
    d = synth.synthetic_svc_model(C, M, A, context=ctx, n_fit_per_class=nfit, seed=C)
    # related haplotypes: queries copy training rows over long stretches so long match runs occur
    rng = np.random.RandomState(N)
    X = synth.synthetic_X(N, C, seed=N, miss=0.02)
    for n in range(0, N, 2):
        w = rng.randint(d.W)
        src = d.svc[w]["xfit"][rng.randint(d.svc[w]["xfit"].shape[0])]
        start = w * M - ctx
        seg = src if start >= 0 else src[-start:]
        lo = max(0, start)
        ln = min(len(seg), C - lo)
        X[n, lo:lo + ln] = seg[:ln]
    dev = ga.DeviceModel(d)
    _, b64 = dev.base_predict(X)
    ref = oracle.base_covrsk(X, M, ctx, _svc_oracle_windows(d))
    assert np.max(np.abs(b64 - ref)) < 1e-12
    assert np.array_equal(np.argmax(b64, -1), np.argmax(ref, -1))
    assert np.allclose(b64.sum(-1), 1.0, atol=1e-9)


# ---------------------------------------------------------------- CLI end to end ------------------------
def _write_synth_vcf(path, pos, ref, alt, X, samples, chm="22"):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=%s>\n" % chm)
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for v in range(len(pos)):
            gt = ["%s|%s" % ("." if X[2 * i, v] == 2 else X[2 * i, v], "." if X[2 * i + 1, v] == 2 else X[2 * i + 1, v])
                  for i in range(len(samples))]
            f.write("%s\t%d\trs%d\t%s\t%s\t.\tPASS\t.\tGT\t%s\n" % (chm, pos[v], v, ref[v], alt[v], "\t".join(gt)))


@pytest.mark.parametrize("phase", [False, True])
def test_cli_end_to_end(ga, oracle, tmp_path, phase):
    from gnomix_amd import synth, cli, postprocess
    d = synth.synthetic_model(C=16037, M=100, A=4, S=75, n_rounds=8, seed=11)
    rng = np.random.RandomState(1)
    d.snp_pos = np.sort(rng.choice(np.arange(10_000, 5_000_000), size=d.C, replace=False))
    d.snp_ref = rng.choice(list("ACGT"), size=d.C)
    d.snp_alt = rng.choice(list("ACGT"), size=d.C)
    d.gen_map_pos = np.array([1, 1_000_000, 3_000_000, 6_000_000])
    d.gen_map_cm = np.array([0.0, 1.1, 3.7, 7.2])
    mp = str(tmp_path / "model.gnx")
    d.save(mp)
    n_ind = 3
    keep = np.sort(rng.choice(d.C, size=d.C - 500, replace=False))      # the query lacks 500 model SNPs
    Xq = synth.synthetic_X(2 * n_ind, d.C, seed=3, miss=0.01)
    ref = d.snp_ref.copy()
    flip = rng.rand(d.C) < 0.05                                          # 5 % REF mismatches get flipped
    ref[flip] = np.where(ref[flip] == "A", "C", "A")
    vcf = str(tmp_path / "q.vcf")
    _write_synth_vcf(vcf, d.snp_pos[keep], ref[keep], d.snp_alt[keep], Xq[:, keep], ["S%d" % i for i in range(n_ind)])
    out = str(tmp_path / "out")
    assert cli.main(["gnomix.py", vcf, out, "22", "True" if phase else "False", mp]) == 0
    msp = open(out + "/query_results.msp").read().splitlines()
    fb = open(out + "/query_results.fb").read().splitlines()
    assert len(msp) == 2 + d.W and len(fb) == 2 + d.W
    assert msp[1].split("\t")[6:] == ["S0.0", "S0.1", "S1.0", "S1.1", "S2.0", "S2.1"]
    # what the model saw: model-order matrix with missing SNPs = 2 and flipped REFs
    Xm = np.full((2 * n_ind, d.C), 2, dtype=np.int8)
    Xm[:, keep] = Xq[:, keep]
    fl = flip & np.isin(np.arange(d.C), keep)
    Xm[:, fl] = np.where(Xm[:, fl] == 2, 2, 1 - Xm[:, fl])
    B = oracle.base_lr(Xm, d.M, d.context, d.lr_coef, d.lr_intercept)
    T = _oracle_trees(oracle, d)
    lab_file = np.array([[int(v) for v in ln.split("\t")[6:]] for ln in msp[2:]]).T
    if not phase:
        p_ref, l_ref = oracle.smooth_xgb(T, B, d.S)
        assert np.array_equal(lab_file, l_ref)
        p_file = np.array([[float(v) for v in ln.split("\t")[4:]] for ln in fb[2:]], dtype=np.float32)
        assert np.max(np.abs(p_file - np.swapaxes(p_ref, 1, 2).reshape(-1, d.W).T)) <= 1e-5
    else:
        rows = lambda r: oracle.xgb_predict_proba(T, r)
        labs = lambda b: oracle.smooth_xgb(T, b, d.S)[1]
        for i in range(n_ind):
            _, _, Ym, Yp, _, _ = oracle.gnofix(Xm[2 * i], Xm[2 * i + 1], B[2 * i:2 * i + 2], d.S, rows, labs)
            assert np.array_equal(lab_file[2 * i], Ym) and np.array_equal(lab_file[2 * i + 1], Yp)
        assert os.path.exists(out + "/query_file_phased.vcf")


@pytest.mark.parametrize("extra", [16, 4, 8, 13])  # row pitch: 16-, 4-, 8-byte and unaligned SNP granules
def test_gnofix_wide_windows_and_equal_blocks(ga, oracle, extra, gnofix_ctx):
    """windows of several hundred SNPs: blocks that are identical between the two haplotypes (no contribution to the
    convergence signature), blocks that differ only in their last SNP, and the vectorised SNP swap at every alignment"""
    from gnomix_amd import synth
    W, A, S, M = 96, 5, 11, 208
    C = W * M + extra
    d = ga.GnxModelData(C=C, M=M, A=A, S=S, context=0, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(3, A, S * A, seed=21, thr_lo=0.0, thr_hi=0.5, leaf_scale=1.0).items():
        setattr(d, k, v)
    dev = ga.DeviceModel(d, ctx=gnofix_ctx)
    T = _oracle_trees(oracle, d)
    rng = np.random.RandomState(40 + extra)
    n_ind = 3
    X = rng.randint(0, 2, size=(2 * n_ind, C)).astype(np.int8)
    for i in range(n_ind):
        for u in range(W):
            kind = rng.randint(4)
            lo, hi = u * M, (u + 1) * M if u < W - 1 else C
            if kind == 0:
                X[2 * i + 1, lo:hi] = X[2 * i, lo:hi]
            elif kind == 1:
                X[2 * i + 1, lo:hi] = X[2 * i, lo:hi]
                X[2 * i + 1, hi - 1] ^= 1
    B = rng.dirichlet(np.ones(A) * 0.3, size=(2 * n_ind, W))
    Xo, Y, nsw = dev.gnofix(X, B, max_it=8)
    rows = lambda r: oracle.xgb_predict_proba(T, r)
    labs = lambda b: oracle.smooth_xgb(T, b, S)[1]
    for i in range(n_ind):
        Xm, Xp, Ym, Yp, _, ns = oracle.gnofix(X[2 * i], X[2 * i + 1], B[2 * i:2 * i + 2], S, rows, labs, max_it=8)
        assert np.array_equal(Xo[2 * i], Xm) and np.array_equal(Xo[2 * i + 1], Xp), i
        assert np.array_equal(Y[2 * i], Ym) and np.array_equal(Y[2 * i + 1], Yp) and int(nsw[i]) == ns, i
    assert int(nsw.sum()) > 0


def test_gnofix_strips_in_global_scratch(ga, oracle, gnofix_ctx):
    """a long chromosome with many classes (W = 1500, A = 12): the float32 kernel's strips exceed the LDS and take its
    global-scratch path; the rank kernel reads its tiles from the rank strips in HBM whatever W is"""
    from gnomix_amd import synth
    W, A, S = 1500, 12, 75
    C = W * 3 + 2
    d = ga.GnxModelData(C=C, M=3, A=A, S=S, context=0, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(2, A, S * A, seed=8, thr_lo=0.0, thr_hi=0.4, leaf_scale=1.0).items():
        setattr(d, k, v)
    dev = ga.DeviceModel(d, ctx=gnofix_ctx)
    T = _oracle_trees(oracle, d)
    rng = np.random.RandomState(2)
    X = rng.randint(0, 2, size=(4, C)).astype(np.int8)
    B = rng.dirichlet(np.ones(A) * 0.2, size=(4, W))
    Xo, Y, nsw = dev.gnofix(X, B, max_it=2)
    rows = lambda r: oracle.xgb_predict_proba(T, r)
    labs = lambda b: oracle.smooth_xgb(T, b, S)[1]
    for i in range(2):
        Xm, Xp, Ym, Yp, _, ns = oracle.gnofix(X[2 * i], X[2 * i + 1], B[2 * i:2 * i + 2], S, rows, labs, max_it=2)
        assert np.array_equal(Xo[2 * i], Xm) and np.array_equal(Xo[2 * i + 1], Xp)
        assert np.array_equal(Y[2 * i], Ym) and np.array_equal(Y[2 * i + 1], Yp) and int(nsw[i]) == ns
    assert int(nsw.sum()) > 0


# ---------------------------------------------------------------- calibrator, plain string kernel -------
def test_calibrator_golden_G8(ga, oracle):
    """Smoother.predict_proba with calibrate=True: raw smoother output -> the reference's Calibrator.transform"""
    from gnomix_amd import synth
    g = load_golden("G8_calib_sk.npz")
    A = int(g["A"])
    N, W, _ = g["P"].shape
    # a smoother whose raw output is exactly P: CRF with zero transitions and identity-log state weights is awkward, so
    # drive the calibration stage directly through an xgb model with ONE depth-1 tree per class is not exact either ->
    # use the CRF smoother with state = 0, trans = 0 on B: marginals are uniform; instead test the kernel via the
    # ABI's own composition: smooth_predict on a model whose trees are all zero-leaf gives uniform margins, not P.
    # The direct route: calibrate_only through a tiny model whose smoother is the identity on one-hot-free inputs does not
    # exist in the reference either, so the golden pins k_calibrate through DeviceModel.calibrate_rows.
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=5, context=5, smooth_kind="crf", crf_state=np.zeros((A, A)), crf_trans=np.zeros((A, A)))
    off = [0]
    for i in range(A):
        off.append(off[-1] + len(g["x%d" % i]))
    d.calib_off = np.array(off, np.int32)
    d.calib_x = np.concatenate([g["x%d" % i] for i in range(A)])
    d.calib_y = np.concatenate([g["y%d" % i] for i in range(A)])
    d.calib_is_f32 = True    # fitted on float32 probabilities (make_golden.py)
    dev = ga.DeviceModel(d)
    out = dev.calibrate_rows(g["P"].reshape(-1, A)).reshape(N, W, A)
    assert out.dtype == np.float64
    assert np.max(np.abs(out - g["out"])) < 1e-12       # vs the REFERENCE's Calibrator.transform (numpy >= 2 float64 path)
    assert np.allclose(out.sum(-1), 1.0, atol=1e-12)
    # end to end: calibrate on -> uniform CRF marginals (state = trans = 0) go through the same maps
    sm = ga.HipSmoother(dev, calibrate=True)
    B = np.random.RandomState(0).dirichlet(np.ones(A), size=(3, W))
    p = sm.predict_proba(B)
    want = dev.calibrate_rows(np.full((3 * W, A), 1.0 / A)).reshape(3, W, A)
    assert p.dtype == np.float64 and np.max(np.abs(p - want)) < 1e-12
    assert np.array_equal(sm.predict(B), np.argmax(want, -1))
    sm.calibrate = False
    assert np.allclose(sm.predict_proba(B), 1.0 / A, atol=1e-12)


def test_string_kernel_base_golden_G8(ga, oracle):
    """StringKernelBase (plain triangular-number kernel = every substring length) through the generic run kernel"""
    from gnomix_amd import convert
    g = load_golden("G8_calib_sk.npz")
    C, M, A, ctx = int(g["sk_C"]), int(g["sk_M"]), int(g["sk_A"]), int(g["sk_ctx"])
    W = C // M
    d = ga.GnxModelData(C=C, M=M, A=A, S=5, context=ctx, base_kind="covrsk")
    d.svc = []
    for i in range(W):
        xf = g["sk%d_Xfit" % i]
        d.svc.append(dict(xfit=xf, support=g["sk%d_support" % i], dual_coef=g["sk%d_dual" % i], intercept=g["sk%d_intercept" % i],
                          prob_a=g["sk%d_probA" % i], prob_b=g["sk%d_probB" % i], n_support=g["sk%d_nsv" % i],
                          ms=convert.string_kernel_lengths(xf.shape[1], "string_kernel_DP_triangular_numbers")))
    dev = ga.DeviceModel(d)
    _, b64 = dev.base_predict(g["sk_X"])
    assert np.max(np.abs(b64 - g["sk_B"])) < 1e-12      # vs the REFERENCE's StringKernelBase.predict_proba
    K = oracle.string_kernel(np.zeros((1, 8), np.int8), np.zeros((1, 8), np.int8))
    assert K[0, 0] == 36


# ---------------------------------------------------------------- forest base (XGBBase) ----------
def _forest_oracle_trees(O, d):
    return O.Trees(d.fb_tree_off, d.fb_left, d.fb_right, d.fb_feat, d.fb_cond, d.fb_tree_class, d.A, d.fb_base_score,
                   default_left=d.fb_default_left)


@pytest.fixture(params=["forest2", "forest1"])
def forest_ctx(request, monkeypatch):
    """both tree-base kernels on every geometry: k_base_forest2 (two blocks per CU: the default wherever its tile fits) and
    k_base_forest (256-haplotype tile: the fallback, GNX_FOREST_IMPL=1).  The knob is read once per context."""
    from gnomix_amd import _lib
    monkeypatch.setenv("GNX_FOREST_IMPL", "1" if request.param == "forest1" else "0")
    return _lib.Context(0)


@pytest.mark.parametrize("C,M,A,ctx,N,rounds,depth", [
    (4037, 100, 7, 50, 70, 20, 4),     # the reference's XGBBase shape: 20 rounds, depth 4, A trees per round
    (4037, 100, 2, 50, 33, 20, 4),     # A == 2: binary:logistic, one tree per round
    (2531, 100, 3, 30, 300, 5, 2),     # more haplotypes than one 256-thread tile; shallow trees
    (1999, 64, 4, 0, 65, 3, 6),        # no context, deep trees, window start not on a 16-SNP word
    (937, 300, 12, 150, 1, 7, 1),      # stumps ("forest-of-stumps"), 3 windows, a single haplotype
    (1237, 48, 5, 24, 129, 4, 3),      # M multiple of 16: window starts on word boundaries
])
def test_forest_base_vs_oracle(ga, oracle, forest_ctx, C, M, A, ctx, N, rounds, depth):
    from gnomix_amd import synth
    d = synth.synthetic_forest_model(C, M, A, context=ctx, n_rounds=rounds, depth=depth, seed=C + A, p_early_leaf=0.2)
    X = synth.synthetic_X(N, C, seed=N + 1, miss=0.08)
    dev = ga.DeviceModel(d, ctx=forest_ctx)
    b32, b64 = dev.base_predict(X, want_f32=True, want_f64=True)
    ref = oracle.base_forest(_forest_oracle_trees(oracle, d), d.fb_win_tree0, X, M, ctx, A, missing=2)
    _close_f32(b32, ref)
    assert np.array_equal(b64, b32.astype(np.float64))
    # the missing code matters: flipping every default direction must change some outputs
    d2 = synth.synthetic_forest_model(C, M, A, context=ctx, n_rounds=rounds, depth=depth, seed=C + A, p_early_leaf=0.2)
    d2.fb_default_left = 1 - d2.fb_default_left
    b32b, _ = ga.DeviceModel(d2, ctx=forest_ctx).base_predict(X, want_f32=True, want_f64=False)
    ref2 = oracle.base_forest(_forest_oracle_trees(oracle, d2), d2.fb_win_tree0, X, M, ctx, A, missing=2)
    _close_f32(b32b, ref2)
    assert not np.array_equal(ref, ref2)


def test_forest_base_end_to_end_with_smoother(ga, oracle):
    """forest base -> xgb smoother in one gnx_infer call == oracle base_forest -> oracle smoother"""
    from gnomix_amd import synth
    C, M, A, S, N = 9037, 100, 5, 31, 40
    d = synth.synthetic_forest_model(C, M, A, n_rounds=20, depth=4, seed=3, S=S, smooth="xgb")
    X = synth.synthetic_X(N, C, seed=5, miss=0.02)
    dev = ga.DeviceModel(d)
    p32, lab = dev.infer(X)
    b32, _ = dev.base_predict(X, want_f32=True, want_f64=False)
    ref_p, _ = oracle.smooth_xgb(_oracle_trees(oracle, d), b32, S)   # from the device's own B: isolates the smoother
    _close_f32(p32, ref_p)
    assert np.array_equal(lab, np.argmax(ref_p, -1))
    Bo = oracle.base_forest(_forest_oracle_trees(oracle, d), d.fb_win_tree0, X, M, d.context, A)
    lab_o = oracle.smooth_xgb(_oracle_trees(oracle, d), Bo, S)[1]
    assert np.mean(lab != lab_o) < 1e-3   # expf last-bit differences in B may flip a knife-edge window


def test_forest_base_rejects_bad_models(ga):
    from gnomix_amd import synth
    d = synth.synthetic_forest_model(1237, 100, 3, n_rounds=2, depth=2, seed=1)
    d.fb_feat = d.fb_feat.copy()
    internal = np.where(d.fb_left != -1)[0]
    d.fb_feat[internal[0]] = 10 ** 6
    with pytest.raises(ga.GnxError, match="split feature outside"):
        ga.DeviceModel(d)
    d = synth.synthetic_forest_model(1237, 100, 3, n_rounds=2, depth=2, seed=1)
    d.fb_win_tree0 = d.fb_win_tree0.copy()
    d.fb_win_tree0[-1] -= 1
    with pytest.raises(ga.GnxError, match="fb_win_tree0"):
        ga.DeviceModel(d)


# ---------------------------------------------------------------- rank-quantised smoother vs float smoother --------
@pytest.mark.parametrize("W,A,S,rounds,depth", [(370, 7, 75, 12, 4), (131, 3, 31, 6, 5), (160, 12, 75, 4, 2), (500, 5, 75, 8, 4),
                                                 (200, 4, 31, 7, 4), (700, 7, 75, 23, 4)])
def test_smooth_rank_kernel_equals_float_kernel(ga, oracle, monkeypatch, W, A, S, rounds, depth):
    """k_smooth_xgb_rk replaces every `p < threshold` by a 16-bit rank compare: outputs must be BIT-identical to the
    float kernel, including probabilities that sit exactly on a threshold (p == thr goes right), just below / above
    one, 0, 1, values outside [0, 1], infinities and NaN (never < anything)."""
    from gnomix_amd import synth
    rng = np.random.RandomState(W + A)
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(rounds, A, S * A, depth=depth, seed=W, thr_lo=0.0, thr_hi=1.0, p_early_leaf=0.15).items():
        setattr(d, k, v)
    N = 24
    B = rng.dirichlet(np.ones(A) * 0.4, size=(N, W)).astype(np.float32)
    thr = d.cond[d.left != -1]
    pick = rng.choice(thr, size=B.shape)
    m = rng.random_sample(B.shape)
    B = np.where(m < 0.25, pick, B)                                            # exactly on a threshold
    B = np.where((m >= 0.25) & (m < 0.35), np.nextafter(pick, np.float32(-1)), B)   # one ulp below
    B = np.where((m >= 0.35) & (m < 0.45), np.nextafter(pick, np.float32(2)), B)    # one ulp above
    special = np.array([0.0, 1.0, -0.25, 1.75, np.inf, -np.inf, np.nan, 1e-30, -0.0], np.float32)
    sp = m > 0.97
    sp[8:] = False                                                            # keep some haplotypes finite for the oracle
    B = np.where(sp, rng.choice(special, size=B.shape), B).astype(np.float32)
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "f32")
    pf, lf = ga.DeviceModel(d).smooth_predict(B)
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "rk")
    for rpl in ("1", "2", "3", "4", "5", "6"):
        monkeypatch.setenv("GNX_RK_RPL", rpl)
        pr, lr = ga.DeviceModel(d).smooth_predict(B)
        assert np.array_equal(pf, pr, equal_nan=True), rpl
        assert np.array_equal(lf, lr), rpl
    # pointer nodes (k_smooth_xgb_rk<.., PTR>: depth 4 and <= 3 segments per strip, other shapes run the plain rank kernel);
    # 7 and 23 rounds leave an odd tree at the end of a staging group (the single-tree walk)
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "rp")
    for rpl in ("1", "2", "3", "4"):
        monkeypatch.setenv("GNX_RK_RPL", rpl)
        pr, lr = ga.DeviceModel(d).smooth_predict(B)
        assert np.array_equal(pf, pr, equal_nan=True), rpl
        assert np.array_equal(lf, lr), rpl
    monkeypatch.delenv("GNX_RK_RPL")
    finite = np.isfinite(B).all(axis=(1, 2))                                  # oracle as the third opinion
    T = _oracle_trees(oracle, d)
    p_ref, l_ref = oracle.smooth_xgb(T, B[finite], S)
    assert np.array_equal(lf[finite], l_ref)
    _close_f32(pf[finite], p_ref)


def test_smooth_retired_impl_names_take_the_rank_kernel(ga, monkeypatch):
    """GNX_SMOOTH_IMPL=bs and =h64 named kernels that are no longer in the tree: like any unrecognised name they select the rank
    kernel with pointer nodes, so probabilities and labels are BIT-identical to GNX_SMOOTH_IMPL=rp, values exactly on a threshold,
    one ulp off it, outside [0, 1], infinities and NaN included."""
    from gnomix_amd import synth
    N, W, A, S = 5, 40, 3, 9
    rng = np.random.RandomState(W + A)
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(3, A, S * A, depth=4, seed=W, thr_lo=0.0, thr_hi=1.0, p_early_leaf=0.15).items():
        setattr(d, k, v)
    B = rng.dirichlet(np.ones(A) * 0.4, size=(N, W)).astype(np.float32)
    thr = d.cond[d.left != -1]
    pick = rng.choice(thr, size=B.shape)
    m = rng.random_sample(B.shape)
    B = np.where(m < 0.25, pick, B)                                            # exactly on a threshold
    B = np.where((m >= 0.25) & (m < 0.35), np.nextafter(pick, np.float32(-1)), B)   # one ulp below
    B = np.where((m >= 0.35) & (m < 0.45), np.nextafter(pick, np.float32(2)), B)    # one ulp above
    special = np.array([0.0, 1.0, -0.25, 1.75, np.inf, -np.inf, np.nan, 1e-30, -0.0], np.float32)
    B = np.where(m > 0.97, rng.choice(special, size=B.shape), B).astype(np.float32)
    assert np.count_nonzero(np.isin(B, thr)) > 0
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "rp")
    pr, lr = ga.DeviceModel(d).smooth_predict(B)
    for name in ("bs", "h64"):
        monkeypatch.setenv("GNX_SMOOTH_IMPL", name)
        p, lab = ga.DeviceModel(d).smooth_predict(B)
        assert np.array_equal(pr, p, equal_nan=True), name
        assert np.array_equal(lr, lab), name


def test_forest_kernels_on_lgbm_and_catboost_models(ga, oracle, forest_ctx):
    """LGBMBase / CBBase (src/Base/models.py:38-52, 68-81): LightGBM model strings and CatBoost JSON exports converted to the forest
    base's arrays (gnomix_amd.convert) run through the forest kernels == the oracle on the same arrays (which tests/test_host_cpu.py
    checks against each library's own prediction rule evaluated directly)"""
    import json
    from gnomix_amd import convert
    from test_host_cpu import _lgbm_model_string
    rng = np.random.RandomState(77)
    C, M, A, ctx = 1237, 100, 7, 50
    W = C // M
    widths = [M + 2 * ctx + (C - M * W if w == W - 1 else 0) for w in range(W)]
    lg = convert.forest_from_lgbm_text([_lgbm_model_string(rng, wd, A, rounds=20)[0] for wd in widths], A)
    cb_models = []
    for wd in widths:
        trees = []
        for t in range(20):
            splits = [{"float_feature_index": int(rng.randint(wd)), "border": float(rng.choice([0.5, 1.5])), "split_type": "FloatFeature"}
                      for _ in range(4)]
            trees.append({"splits": splits, "leaf_values": [float(np.float32(v)) for v in rng.randn(A << 4) * 0.3]})
        cb_models.append(json.dumps({"oblivious_trees": trees, "scale_and_bias": [1.0, [float(b) for b in rng.randn(A) * 0.1]]}))
    cb = convert.forest_from_catboost_json(cb_models, A)
    X = rng.randint(0, 3, size=(300, C)).astype(np.int8)
    for fb in (lg, cb):
        d = ga.GnxModelData(C=C, M=M, A=A, S=5, context=ctx, base_kind="forest", **fb)
        b32, _ = ga.DeviceModel(d, ctx=forest_ctx).base_predict(X, want_f32=True, want_f64=False)
        ref = oracle.base_forest(_forest_oracle_trees(oracle, d), d.fb_win_tree0, X, M, ctx, A, missing=2)
        assert np.array_equal(np.argmax(b32, -1), np.argmax(ref, -1))
        _close_f32(b32, ref)


# ---------------------------------------------------------------- random-forest base (RFBase) -----
def _rf_dict(d):
    return {k[3:]: getattr(d, k) for k in ("rf_win_tree0", "rf_tree_off", "rf_left", "rf_right", "rf_feat", "rf_thr", "rf_value")}


def test_rforest_base_golden_G9(ga, oracle, forest_ctx):
    """k_base_rforest against the REFERENCE's RFBase.predict_proba output (sklearn forests): bit-exact float64"""
    g = load_golden("G9_rf.npz")
    d = ga.GnxModelData(C=int(g["C"]), M=int(g["M"]), A=int(g["A"]), S=5, context=int(g["ctx"]), base_kind="rforest",
                        **{k: g[k] for k in g.files if k.startswith("rf_")})
    dev = ga.DeviceModel(d, ctx=forest_ctx)
    b32, b64 = dev.base_predict(g["X"], want_f32=True, want_f64=True)
    assert np.array_equal(b64, g["B"])
    assert np.array_equal(b32, g["B"].astype(np.float32))
    assert np.array_equal(np.argmax(b64, -1), np.argmax(g["B"], -1))


@pytest.mark.parametrize("C,M,A,ctx,N,trees,depth", [
    (4037, 100, 7, 50, 70, 20, 4),      # the reference's RFBase shape
    (2531, 100, 3, 30, 300, 5, 2),      # more haplotypes than one tile
    (1999, 64, 12, 0, 65, 7, 6),        # A > 8: 16-class accumulator variant, deep trees, no context
    (937, 300, 20, 150, 1, 3, 1),       # stumps, A > 16, a single haplotype
    (1237, 48, 2, 24, 129, 9, 3),
])
def test_rforest_base_vs_oracle(ga, oracle, forest_ctx, C, M, A, ctx, N, trees, depth):
    from gnomix_amd import synth
    d = synth.synthetic_rforest_model(C, M, A, context=ctx, n_trees=trees, depth=depth, seed=C + A, p_early_leaf=0.2)
    X = synth.synthetic_X(N, C, seed=N + 2, miss=0.08)
    b32, b64 = ga.DeviceModel(d, ctx=forest_ctx).base_predict(X, want_f32=True, want_f64=True)
    ref = oracle.base_rforest(_rf_dict(d), X, M, ctx, A)
    assert np.array_equal(b64, ref)
    assert np.array_equal(b32, ref.astype(np.float32))


def test_base_long_chromosome_many_windows(ga, oracle):
    """chr1-sized window count with 12 ancestries and only a few haplotype tiles: the per-block chunk / window tables of
    the logistic kernel must be sized from the real chunk spans (the first sizing rule asked for 187 KB of LDS here)"""
    from gnomix_amd import synth
    C, M, A, ctx, N = 1431 * 400 + 211, 400, 12, 200, 600
    d = synth.synthetic_model(C=C, M=M, A=A, S=5, context=ctx, seed=5, smooth=None)
    X = synth.synthetic_X(N, C, seed=9, miss=0.02)
    dev = ga.DeviceModel(d)
    _, big = dev.base_predict(X, want_f32=False, want_f64=True)          # 256-haplotype tiles
    _, small = dev.base_predict(X[:48], want_f32=False, want_f64=True)   # 64-haplotype tiles, other launch geometry
    assert np.array_equal(big[:48], small)                                # exact integer logits: tiling-independent
    ref = oracle.base_lr(X[:6], M, ctx, d.lr_coef, d.lr_intercept)
    assert np.max(np.abs(big[:6] - ref)) < 1e-12


# ---------------------------------------------------------------- host-pointer staging in several batches ---------
def test_host_path_batching_is_invisible(ga, monkeypatch):
    """the host-pointer entry points stage X in batches (~1 GiB); force batches of 6 haplotypes / 3 individuals on small
    inputs and require bit-identical results to the single-batch run (offsets, last partial batch, workspace reuse)"""
    from gnomix_amd import synth
    C, M, A, S, N = 6037, 100, 5, 21, 40
    d = synth.synthetic_model(C=C, M=M, A=A, S=S, n_rounds=10, seed=8)
    X = synth.synthetic_X(N, C, seed=4, miss=0.02)
    ref_dev = ga.DeviceModel(d)
    b32_ref, b64_ref = ref_dev.base_predict(X, want_f32=True, want_f64=True)
    p_ref, l_ref = ref_dev.infer(X)
    Xg, yg, ns = ref_dev.gnofix(X, b64_ref)
    monkeypatch.setenv("GNX_HOST_BATCH", "6")
    from gnomix_amd import _lib
    ctx = _lib.Context(0)   # the knobs are read once per context (gnx_init), never on a launch path
    dev = ga.DeviceModel(d, ctx=ctx)
    b32, b64 = dev.base_predict(X, want_f32=True, want_f64=True)
    p, l = dev.infer(X)
    assert np.array_equal(b32, b32_ref) and np.array_equal(b64, b64_ref)
    assert np.array_equal(p, p_ref) and np.array_equal(l, l_ref)
    Xg2, yg2, ns2 = dev.gnofix(X, b64_ref)
    assert np.array_equal(Xg2, Xg) and np.array_equal(yg2, yg) and np.array_equal(ns2, ns)


def test_pinned_host_arrays(ga):
    """Context.pinned_empty (gnx_host_alloc): numpy arrays over page-locked memory work as inputs of the host-pointer path"""
    from gnomix_amd import synth
    d = synth.synthetic_model(C=3037, M=100, A=3, S=11, n_rounds=4, seed=2)
    X = synth.synthetic_X(10, d.C, seed=3)
    dev = ga.DeviceModel(d)
    Xp = dev.ctx.pinned_empty(X.shape, np.int8)
    Xp[...] = X
    p0, l0 = dev.infer(X)
    p1, l1 = dev.infer(Xp)
    assert np.array_equal(p0, p1) and np.array_equal(l0, l1)
    del Xp


# ---------------------------------------------------------------- polynomial string kernel base -----------------
def test_poly_string_kernel_golden_G10(ga, oracle):
    """k_covrsk_dec<POLY> + SVC coupling against the reference's PolynomialStringKernelBase.predict_proba"""
    g = load_golden("G10_poly.npz")
    wins = []
    for i in range(int(g["n_win"])):
        pre = "svc%d_" % i
        wins.append({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
    d = ga.GnxModelData(C=int(g["C"]), M=int(g["M"]), A=int(g["A"]), S=5, context=int(g["ctx"]), base_kind="covrsk", svc=wins)
    _, b64 = ga.DeviceModel(d).base_predict(g["X"])
    assert np.max(np.abs(b64 - g["B"])) < 1e-12
    assert np.array_equal(np.argmax(b64, -1), np.argmax(g["B"], -1))


@pytest.mark.parametrize("M,ctx,A,N,nfit,pmatch", [
    (100, 50, 3, 70, 8, 0.5),        # ~100 mismatches per window: one numpy leaf block
    (300, 150, 2, 33, 6, 0.5),       # ~300 run lengths: the pairwise recursion splits once
    (700, 350, 4, 5, 5, 0.45),       # ~800: two levels of splits, odd remainders
    (260, 0, 3, 64, 6, 0.97),        # few mismatches: n < 8 and n < 128 paths, long runs
    (64, 32, 5, 129, 4, 0.7),
])
def test_poly_string_kernel_vs_oracle(ga, oracle, M, ctx, A, N, nfit, pmatch):
    from gnomix_amd import synth, convert
    W = 4
    C = W * M + M // 3 + 1
    d = synth.synthetic_svc_model(C, M, A, context=ctx, n_fit_per_class=nfit, seed=M + A)
    for i, w in enumerate(d.svc):
        w.pop("ms")
        w.update(convert.poly_run_values(d.window_width(i)))
    rng = np.random.RandomState(N)
    X = synth.synthetic_X(N, C, seed=N, miss=0.02)
    for n in range(N):           # queries related to training rows with probability pmatch per SNP
        w = rng.randint(d.W)
        src = d.svc[w]["xfit"][rng.randint(d.svc[w]["xfit"].shape[0])]
        start = w * M - ctx
        seg = src if start >= 0 else src[-start:]
        lo = max(0, start)
        ln = min(len(seg), C - lo)
        keep = rng.random_sample(ln) < pmatch
        X[n, lo:lo + ln] = np.where(keep, seg[:ln], X[n, lo:lo + ln])
    _, b64 = ga.DeviceModel(d).base_predict(X)
    ow = [dict(Xfit=w["xfit"], support=w["support"], dual=w["dual_coef"], intercept=w["intercept"], probA=w["prob_a"],
               probB=w["prob_b"], n_support=w["n_support"], run_value=w["run_value"], poly_p=w["poly_p"]) for w in d.svc]
    ref = oracle.base_covrsk(X, M, ctx, ow)
    assert np.max(np.abs(b64 - ref)) < 1e-12
    assert np.array_equal(np.argmax(b64, -1), np.argmax(ref, -1))


# ---------------------------------------------------------------- CNN smoother ("large" mode) -------------------
def test_cnn_smoother_golden_G11(ga, oracle):
    g = load_golden("G11_cnn.npz")
    A, S, W = int(g["A"]), int(g["S"]), int(g["W"])
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="cnn", cnn_weight=g["weight"], cnn_bias=g["bias"])
    proba, labels = ga.DeviceModel(d).smooth_predict(g["B"])
    assert proba.dtype == np.float32
    assert np.max(np.abs(proba - g["proba"])) < 1e-5       # vs the REFERENCE's output
    assert np.array_equal(labels, g["labels"])


@pytest.mark.parametrize("N,W,A,S", [(5, 163, 7, 75), (33, 370, 7, 75), (9, 150, 12, 31), (1, 64, 2, 5), (70, 130, 20, 41), (3, 200, 32, 75)])
def test_cnn_smoother_vs_oracle(ga, oracle, N, W, A, S):
    rng = np.random.RandomState(N * W + A)
    B = rng.dirichlet(np.ones(A) * 0.4, size=(N, W))
    wgt = (rng.standard_normal((A, A, S)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(A) * 0.2).astype(np.float32)
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="cnn", cnn_weight=wgt, cnn_bias=bias)
    dev = ga.DeviceModel(d)
    p_ref, l_ref = oracle.smooth_cnn(B, wgt, bias)
    for Bin in (B, B.astype(np.float32)):
        proba, labels = dev.smooth_predict(Bin)
        assert np.max(np.abs(proba - p_ref)) < 1e-5
        close = np.sort(p_ref, -1)[..., -1] - np.sort(p_ref, -1)[..., -2] < 1e-5     # ties within the tolerance may flip
        assert np.array_equal(labels[~close], l_ref[~close])
    p64, _ = dev.smooth_predict(B, proba_dtype=np.float64)
    assert np.array_equal(p64, dev.smooth_predict(B)[0].astype(np.float64))


def test_cnn_end_to_end(ga, oracle):
    """"large" mode shape: logistic base -> CNN smoother in one gnx_infer call"""
    from gnomix_amd import synth
    C, M, A, S, N = 9037, 100, 5, 31, 40
    d = synth.synthetic_model(C=C, M=M, A=A, S=S, seed=3, smooth=None)
    rng = np.random.RandomState(1)
    d.smooth_kind = "cnn"
    d.cnn_weight = (rng.standard_normal((A, A, S)) * 0.3).astype(np.float32)
    d.cnn_bias = (rng.standard_normal(A) * 0.2).astype(np.float32)
    X = synth.synthetic_X(N, C, seed=5, miss=0.02)
    p, lab = ga.DeviceModel(d).infer(X)
    Bo = oracle.base_lr(X, M, d.context, d.lr_coef, d.lr_intercept)
    po, lo = oracle.smooth_cnn(Bo, d.cnn_weight, d.cnn_bias)
    assert np.max(np.abs(p - po)) < 1e-5
    assert np.mean(lab != lo) < 1e-3
