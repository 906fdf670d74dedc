"""k_smooth_xgb_h32 (GNX_SMOOTH_IMPL=h32: lane = haplotype, 32 per half-wave, the strip [slot pair][class][32 haplotypes]) against
the rank kernel (GNX_SMOOTH_IMPL=rk) and the oracle's smooth_xgb.

Same ranks, same leaves, summed in the same order: probabilities and labels must be BIT-identical to the rank kernel's; against
the oracle the tolerance of the other smoother tests (labels identical, 2.4e-7: the last bit of expf).

The shapes are the smallest at which this kernel can go wrong.  A block is 96 windows x 32 haplotypes; a staging group is at most 16
trees (8 beside the 76 KB strip of S = 75 / A = 7).  The model loader refuses W < 2 S as the reference does (src/Smooth/models.py:13),
so W = 1 and W < pad cannot reach any smoother kernel: test_loader_refuses_short_chromosomes pins that, and W = 2 with S = 1 is the
smallest chromosome there is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _model(ga, W, A, S, rounds, depth=4, drop=0, seed=0):
    from gnomix_amd import synth
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="xgb")
    T = synth.synthetic_trees(rounds, A, S * A, depth=depth, seed=seed + W, thr_lo=0.0, thr_hi=1.0, p_early_leaf=0.15)
    if drop:  # the last classes get one tree less: uneven trees per class
        n = len(T["tree_class"]) - drop
        nn = int(T["tree_off"][n])
        T = dict(tree_off=T["tree_off"][:n + 1], tree_class=T["tree_class"][:n], **{k: T[k][:nn] for k in ("left", "right", "feat", "cond")})
    for k, v in T.items():
        setattr(d, k, v)
    return d


def _inputs(d, N, W, A, seed):
    """Dirichlet rows with values exactly on a threshold and one ulp either side; haplotypes >= 8 also carry 0, 1, values outside
    [0, 1], infinities and NaN (the first 8 stay finite for the oracle)"""
    rng = np.random.RandomState(seed)
    B = rng.dirichlet(np.ones(A) * 0.4, size=(N, W)).astype(np.float32)
    thr = d.cond[d.left != -1]
    pick = rng.choice(thr, size=B.shape)
    m = rng.random_sample(B.shape)
    B = np.where(m < 0.25, pick, B)
    B = np.where((m >= 0.25) & (m < 0.35), np.nextafter(pick, np.float32(-1)), B)
    B = np.where((m >= 0.35) & (m < 0.45), np.nextafter(pick, np.float32(2)), B)
    special = np.array([0.0, 1.0, -0.25, 1.75, np.inf, -np.inf, np.nan, 1e-30, -0.0], np.float32)
    sp = m > 0.95
    sp[:8] = False
    return np.where(sp, rng.choice(special, size=B.shape), B).astype(np.float32)


def _bits(p):
    return np.ascontiguousarray(p).view(np.int32 if p.dtype == np.float32 else np.int64)


def _run(ga, monkeypatch, impl, d, B, **kw):
    monkeypatch.setenv("GNX_SMOOTH_IMPL", impl)
    return ga.DeviceModel(d).smooth_predict(B, **kw)


def _check(ga, oracle, monkeypatch, d, B, S):
    pr, lr = _run(ga, monkeypatch, "rk", d, B)
    ph, lh = _run(ga, monkeypatch, "h32", d, B)
    assert np.array_equal(_bits(pr), _bits(ph))
    assert np.array_equal(lr, lh)
    fin = np.isfinite(B).all(axis=(1, 2))
    T = oracle.Trees(d.tree_off, d.left, d.right, d.feat, d.cond, d.tree_class, d.A, d.base_score)
    p_ref, l_ref = oracle.smooth_xgb(T, B[fin], S)
    assert np.array_equal(lh[fin], l_ref)
    assert ph.dtype == p_ref.dtype == np.float32
    assert np.max(np.abs(ph[fin] - p_ref)) <= 2.4e-7
    return ph, lh


# N: 1, 31, 32, 33, 70 (partial haplotype groups, clamped loads).  W: 2 (the smallest), 95 / 96 / 97 (one window tile and +-1),
# 200 (ragged last tile), 151 (odd: the last slot pair half-used).  S: 1, 3, 75.  A: 2, 3, 7, 12, 16.
# Trees per class (rounds, minus one for the last `drop` classes): 16 = exactly one staging group where a group is 16 trees, 8 where
# it is 8 (S = 75, A = 7); 23 and 9 = more than one group with an odd pair-walk tail; 5 and 3 = odd; early leaves everywhere.
@pytest.mark.parametrize("N,W,A,S,rounds,drop", [
    (1, 2, 2, 1, 16, 0),
    (31, 95, 3, 3, 23, 2),
    (32, 96, 7, 3, 5, 0),
    (33, 97, 12, 3, 3, 5),
    (33, 97, 16, 1, 2, 7),
    (70, 200, 7, 75, 9, 3),
    (33, 151, 7, 75, 8, 0),
])
def test_h32_equals_rank_kernel_and_oracle(ga, oracle, monkeypatch, N, W, A, S, rounds, drop):
    d = _model(ga, W, A, S, rounds, drop=drop)
    B = _inputs(d, N, W, A, seed=N + W)
    _check(ga, oracle, monkeypatch, d, B, S)


def test_h32_f64_input_proba64_and_no_labels(ga, monkeypatch):
    """float64 B is narrowed as the rank kernel narrows it; the float64 output is the float32 probability widened; labels may be absent"""
    N, W, A, S = 33, 97, 7, 3
    d = _model(ga, W, A, S, 5, drop=2)
    B = _inputs(d, N, W, A, seed=5)
    p32, lab = _run(ga, monkeypatch, "rk", d, B)
    p64, none = _run(ga, monkeypatch, "h32", d, B.astype(np.float64), want_labels=False, proba_dtype=np.float64)
    assert none is None and p64.dtype == np.float64
    assert np.array_equal(_bits(p64), _bits(p32.astype(np.float64)))
    p, l2 = _run(ga, monkeypatch, "h32", d, B.astype(np.float64))
    assert np.array_equal(_bits(p), _bits(p32)) and np.array_equal(l2, lab)
    none, l3 = _run(ga, monkeypatch, "h32", d, B, want_proba=False)
    assert none is None and np.array_equal(l3, lab)


@pytest.mark.parametrize("N,W,A,S,rounds,depth", [
    (33, 100, 3, 3, 5, 3),      # depth 3: the kernel walks depth-4 trees only
    (5, 150, 16, 75, 2, 4),     # (S / 2 + 1) * A * 128 = 77 824: a strip offset no longer fits 16 bits
    (5, 150, 12, 75, 2, 4),     # chr1's 12 classes at S = 75: a 130 KB strip, two blocks do not fit a CU's LDS
])
def test_h32_unsupported_shapes_take_the_rank_kernel(ga, oracle, monkeypatch, N, W, A, S, rounds, depth):
    d = _model(ga, W, A, S, rounds, depth=depth)
    B = _inputs(d, N, W, A, seed=W + A)
    _check(ga, oracle, monkeypatch, d, B, S)


def test_loader_refuses_short_chromosomes(ga, monkeypatch):
    """W = 1 and W < pad: refused at model load whatever the smoother kernel (W < 2 S, src/Smooth/models.py:13)"""
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "h32")
    for W, S in ((1, 1), (30, 75)):
        d = _model(ga, W, 3, S, 2)
        with pytest.raises(ga.GnxError):
            ga.DeviceModel(d)


def test_h32_through_infer_device(ga, monkeypatch):
    import torch
    from gnomix_amd import synth
    data = synth.synthetic_model(C=100 * 10 + 3, M=10, A=7, S=21, n_rounds=9, seed=11)
    X = torch.from_numpy(synth.synthetic_X(64, data.C, seed=2)).cuda()
    out = {}
    for impl in ("rk", "h32"):
        monkeypatch.setenv("GNX_SMOOTH_IMPL", impl)
        p, lab = ga.DeviceModel(data).infer_device(X)
        torch.cuda.synchronize()
        out[impl] = (p.cpu(), lab.cpu())
    assert torch.equal(out["rk"][1], out["h32"][1])
    assert torch.equal(out["rk"][0].view(torch.int32), out["h32"][0].view(torch.int32))
