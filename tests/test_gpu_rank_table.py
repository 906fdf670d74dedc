"""The per-model rank table (gnomix_amd/csrc/gnx_rank_table.h) through the kernels that use it: k_smooth_xgb_h32 (GNX_SMOOTH_IMPL=h32),
the rank kernel (rk) and k_gnofix's rank pre-pass, against the float kernel (f32), which knows no ranks, and the oracle.

r(p) = #{k : U[k] <= p} must come out exactly whatever the thresholds do to the table: the bench's uniform ones, all of them inside one
1/1024 interval (the fullest-bucket path: bisections behind the entry, rk_steps > 1), a single one, thresholds at 0, at 1 and at the
smallest denormal, and a set with a run of neighbouring floats that takes the largest table.  The probabilities are random ones, every
threshold itself and the floats either side of it, 0, 1, -0.0, 1.5, -1, NaN, the infinities and denormals.  tests/test_rank_table_host.py
checks the same tables against brute force on the host.

Shapes: S = 75 / A = 7 / depth 4 (the 76 KB strip), about 30 trees, N = 33 and 70 (a ragged last block of 32 haplotypes).  The
loader refuses W < 2 S as the reference does (src/Smooth/models.py:13), so at S = 75 the smallest chromosome with two window blocks
is W = 150 (96 + 54 windows: one block per reflection); W = 230 adds a block between them whose strip touches no reflection (the
staging loop's interior path) and a last block of 38.  W = 100 (96 + 4) runs at S = 49."""
import json

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

DENORM = np.finfo(np.float32).smallest_subnormal


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _thresholds(name):
    from gnomix_amd import synth
    rng = np.random.RandomState(7)
    if name == "bench_uniform":     # synth.synthetic_trees' own: uniform in [0.02, 0.5), what bench.py's ensemble holds
        return None
    if name == "one_1024th":
        return (307.0 / 1024.0 + rng.random_sample(2000) / 1024.0 * 0.999).astype(np.float32)
    if name == "single":
        return np.array([0.37], np.float32)
    if name == "edges":
        return np.array([0.0, 1.0, DENORM], np.float32)
    if name == "large":             # eight neighbouring floats: no table below 2^16 buckets fits them into an entry
        run = np.float32(0.5) + np.arange(8, dtype=np.float32) * np.spacing(np.float32(0.5))
        return np.concatenate([rng.random_sample(6000).astype(np.float32), run.astype(np.float32)])
    raise KeyError(name)


def _model(ga, W, A, S, rounds, thr, seed=0):
    from gnomix_amd import synth
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=S, context=5, smooth_kind="xgb")
    T = synth.synthetic_trees(rounds, A, S * A, depth=4, seed=seed + W, thr_lo=0.02, thr_hi=0.5, p_early_leaf=0.15)
    if thr is not None:
        split = T["left"] != -1
        rng = np.random.RandomState(seed + 1)
        n = int(split.sum())
        pick = thr[rng.permutation(len(thr))[:n]] if len(thr) >= n else np.concatenate([thr, rng.choice(thr, size=n - len(thr))])
        T["cond"] = T["cond"].copy()
        T["cond"][split] = pick
    for k, v in T.items():
        setattr(d, k, v)
    return d


def _inputs(d, N, W, A, seed):
    """Dirichlet rows with every threshold itself and the float either side of it; haplotypes >= 8 also carry the special values
    (the first 8 stay finite for the oracle)"""
    rng = np.random.RandomState(seed)
    B = rng.dirichlet(np.ones(A) * 0.4, size=(N, W)).astype(np.float32)
    thr = np.unique(d.cond[d.left != -1])
    flat = B.reshape(-1)
    trip = np.concatenate([thr, np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf))]).astype(np.float32)
    if len(trip) <= flat.size // 2:      # every threshold and both neighbours at least once, the rest of that half drawn from them
        pos = rng.permutation(flat.size)[:flat.size // 2]
        flat[pos] = np.concatenate([trip, rng.choice(trip, size=len(pos) - len(trip))])
    else:
        pos = rng.permutation(flat.size)[:flat.size // 2]
        flat[pos] = rng.choice(trip, size=len(pos))
    B = flat.reshape(N, W, A)
    special = np.array([0.0, 1.0, -0.0, 1.5, -1.0, np.nan, np.inf, -np.inf, DENORM, 2 * DENORM, -DENORM, 1e-40, 1e-30], np.float32)
    m = rng.random_sample(B.shape)
    sp = m > 0.93
    sp[:8] = False
    return np.where(sp, rng.choice(special, size=B.shape), B).astype(np.float32)


def _bits(p):
    return np.ascontiguousarray(p).view(np.int32)


def _run(ga, monkeypatch, impl, d, B):
    monkeypatch.setenv("GNX_SMOOTH_IMPL", impl)
    m = ga.DeviceModel(d)
    try:
        return m.smooth_predict(B)
    finally:
        m.close()


SHAPES = [(33, 150, 75), (70, 230, 75), (33, 100, 49)]
CASES = [(name, N, W, S, 4) for name in ("bench_uniform", "one_1024th", "single", "edges") for N, W, S in SHAPES]
CASES.append(("large", 33, 150, 75, 60))      # 420 trees: enough split nodes for 6 000 thresholds' worth of buckets and the run of eight


@pytest.mark.parametrize("name,N,W,S,rounds", CASES)
def test_h32_rk_and_float_kernel_agree_bit_for_bit(ga, oracle, monkeypatch, name, N, W, S, rounds):
    A = 7
    d = _model(ga, W, A, S, rounds, _thresholds(name))
    B = _inputs(d, N, W, A, seed=N + W)
    pf, lf = _run(ga, monkeypatch, "f32", d, B)
    pr, lr = _run(ga, monkeypatch, "rk", d, B)
    ph, lh = _run(ga, monkeypatch, "h32", d, B)
    assert np.array_equal(_bits(pr), _bits(ph)) and np.array_equal(lr, lh)
    assert np.array_equal(_bits(pf), _bits(ph)) and np.array_equal(lf, lh)
    fin = np.isfinite(B).all(axis=(1, 2))
    assert fin[:8].all()
    T = oracle.Trees(d.tree_off, d.left, d.right, d.feat, d.cond, d.tree_class, d.A, d.base_score)
    p_ref, l_ref = oracle.smooth_xgb(T, B[fin], S)
    assert np.array_equal(lh[fin], l_ref)
    assert ph.dtype == p_ref.dtype == np.float32
    assert np.max(np.abs(ph[fin] - p_ref)) <= 2.4e-7      # the tolerance of the other smoother tests: the last bit of expf


def test_gnofix_ranks_give_the_golden_run(ga):
    """k_gnofix_ranks reads the same table: one Gnofix call per geometry of G26 (the reference's own run) comes out as before"""
    g = load_golden("G26_gnofix_calibrated.npz")
    for n in g["geoms"]:
        name = str(n)
        W, A, S, Cn = (int(g[name + k]) for k in ("_W", "_A", "_S", "_C"))
        t = name + "_t_"
        d = ga.GnxModelData(C=Cn, M=Cn // W, A=A, S=S, context=0, smooth_kind="xgb", tree_off=g[t + "tree_off"], left=g[t + "left"],
                            right=g[t + "right"], feat=g[t + "feat"], cond=g[t + "cond"], tree_class=g[t + "tree_class"],
                            base_score=float(g[t + "base_score"]))
        d.calib_off, d.calib_x, d.calib_y, d.calib_is_f32 = g[name + "_calib_off"], g[name + "_calib_x"], g[name + "_calib_y"], True
        dev = ga.DeviceModel(d)
        dev.set_calibrate(True)
        X, B = g[name + "_X"], np.ascontiguousarray(g[name + "_B"])
        max_it = json.loads(str(g[name + "_cases"][0]))["max_it"]
        Xo, Y, nsw = dev.gnofix(X, B, max_it=max_it)
        assert np.array_equal(Xo, g[name + "_0_oX"]) and np.array_equal(Y, g[name + "_0_oY"])
        assert np.array_equal(nsw, g[name + "_0_nhist"] - 2)
        dev.close()
