"""Training the boosted-tree base (XGBBase) on the device: gnx_train_gbt_base / train_forest_arrays / HipBase.train.

The trainer is held to tests/gbt_base_exact.py, the plain-Python restatement of the algorithm (itself checked against brute force in
tests/test_train_forest_host.py): the SAME trees, bit for bit.  xgboost is absent here, so parity with xgboost itself is unpinned."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbt_base_exact as E  # noqa: E402

pytestmark = pytest.mark.gpu

# forest/k_train_gbt_base.hip: a histogram block takes FBT_CHUNK features (one per thread) and FBT_SLICE rows
FBT_CHUNK, FBT_SLICE = 256, 2048

INT_KEYS = ("fb_win_tree0", "fb_tree_off", "fb_left", "fb_right", "fb_feat", "fb_default_left", "fb_tree_class")


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _panel(N, C, M, A, seed, miss=0.05, empty_class=None):
    """codes that depend on the window's label; 5 % missing; an all-missing column, a monomorphic one, one identical to another"""
    rng = np.random.RandomState(seed)
    W = C // M
    y = rng.randint(A, size=(N, W)).astype(np.int32)
    if empty_class is not None:
        w, c = empty_class
        y[y[:, w] == c, w] = (c + 1) % A
    f = rng.uniform(0.1, 0.9, (A, C))
    win = np.minimum(np.arange(C) // M, W - 1)
    X = (rng.uniform(size=(N, C)) < f[y[:, win], np.arange(C)[None, :]]).astype(np.int8)
    X[rng.uniform(size=X.shape) < miss] = 2
    X[:, 5] = 2
    X[:, 7] = 0
    X[:, 9] = X[:, 3]
    return X, y


CASES = {
    # three windows, a wider last one, N not a multiple of 64
    "A3": dict(C=79, M=24, ctx=12, N=130, A=3, kw=dict(n_rounds=4, max_depth=4)),
    "A7": dict(C=79, M=24, ctx=12, N=130, A=7, kw=dict(n_rounds=4, max_depth=4)),
    "A2_binary": dict(C=79, M=24, ctx=12, N=130, A=2, kw=dict(n_rounds=4, max_depth=4)),
    "ctx0_M17": dict(C=79, M=17, ctx=0, N=130, A=3, kw=dict(n_rounds=4, max_depth=4)),      # window starts off any word boundary
    "empty_class": dict(C=79, M=24, ctx=12, N=130, A=3, kw=dict(n_rounds=4, max_depth=4), empty_class=(1, 2)),
    "depth1": dict(C=79, M=24, ctx=12, N=130, A=3, kw=dict(n_rounds=4, max_depth=1)),
    "depth5": dict(C=79, M=24, ctx=12, N=130, A=3, kw=dict(n_rounds=4, max_depth=5)),
    # a window wider than one block's feature chunk (320 and 327 > FBT_CHUNK) and more rows than one block's slice (2100 > FBT_SLICE)
    "chunks_and_slices": dict(C=607, M=300, ctx=10, N=FBT_SLICE + 52, A=3, kw=dict(n_rounds=2, max_depth=2)),
    # the gradient kernel's wider instantiations: A in (8, 16] and (16, 32], and 32, the most the entry accepts
    "A9": dict(C=41, M=20, ctx=0, N=130, A=9, kw=dict(n_rounds=2, max_depth=2)),
    "A17": dict(C=41, M=20, ctx=0, N=130, A=17, kw=dict(n_rounds=2, max_depth=2)),
    "A32": dict(C=41, M=20, ctx=0, N=130, A=32, kw=dict(n_rounds=2, max_depth=2)),
}
WIDE_A = ("A9", "A17", "A32")
assert CASES["chunks_and_slices"]["M"] + 2 * CASES["chunks_and_slices"]["ctx"] > FBT_CHUNK


@functools.lru_cache(maxsize=None)
def _case(name):
    """(X, y, restatement's trees, restatement's losses): computed once, shared, never changed"""
    c = CASES[name]
    X, y = _panel(c["N"], c["C"], c["M"], c["A"], seed=len(name), empty_class=c.get("empty_class"))
    k = c["kw"]
    fb, loss = E.train(X, y, c["M"], c["ctx"], c["A"], n_rounds=k["n_rounds"], max_depth=k["max_depth"])
    X.setflags(write=False); y.setflags(write=False)
    return X, y, fb, loss


def _assert_equal_trees(got, ref, what):
    for key in INT_KEYS:
        assert np.array_equal(got[key], ref[key]), (what, key)
    assert got["fb_cond"].dtype == np.float32 and np.array_equal(got["fb_cond"].view(np.uint32), ref["fb_cond"].view(np.uint32)), what


@pytest.mark.parametrize("name", list(CASES))
def test_trees_equal_the_restatement(ga, name):
    import torch
    from gnomix_amd.train import train_forest_arrays
    c = CASES[name]
    X, y, ref, ref_loss = _case(name)
    if name in WIDE_A:      # not a degenerate input: at least A of the reference's trees split
        assert np.count_nonzero(ref["fb_left"][ref["fb_tree_off"][:-1]] >= 0) >= c["A"]
    host, loss_h = train_forest_arrays(X, y, c["M"], c["ctx"], c["A"], **c["kw"])
    _assert_equal_trees(host, ref, "host entry")
    assert np.max(np.abs(loss_h - ref_loss)) <= 1e-12
    Xd, yd = torch.as_tensor(np.array(X), device="cuda:0"), torch.as_tensor(np.array(y), device="cuda:0")
    dev, loss_d = train_forest_arrays(Xd, yd, c["M"], c["ctx"], c["A"], **c["kw"])
    _assert_equal_trees(dev, ref, "_dev entry")
    assert np.max(np.abs(loss_d - ref_loss)) <= 1e-12
    again, loss_a = train_forest_arrays(Xd, yd, c["M"], c["ctx"], c["A"], **c["kw"])
    for key in host:
        assert again[key].tobytes() == dev[key].tobytes() == host[key].tobytes(), key
    assert loss_a.tobytes() == loss_d.tobytes() == loss_h.tobytes()
    # the planted columns in window 0 (feature j is column j - 12; j < 12 mirrors column 11 - j): the all-missing SNP 5 and the
    # monomorphic SNP 7 never split; columns 3 and 9 are identical, so of their four features 2, 8, 15, 21 only the lowest can win
    if c["ctx"] == 12 and c["M"] == 24:
        n0 = host["fb_tree_off"][host["fb_win_tree0"][1]]
        used = set(host["fb_feat"][:n0][host["fb_left"][:n0] >= 0].tolist())
        assert not used & {5 + 12, 11 - 5, 7 + 12, 11 - 7, 8, 15, 21}


@pytest.mark.parametrize("planted,cand", [("class0_missing", 3), ("missing_with_zeros", 2)])
def test_missing_direction_matters(ga, planted, cand):
    from gnomix_amd.train import train_forest_arrays
    C, M, ctx, N, A = 41, 20, 0, 96, 2
    rng = np.random.RandomState(5)
    y = np.repeat(np.arange(2), N // 2)[:, None].repeat(2, axis=1).astype(np.int32)
    X = rng.randint(0, 2, size=(N, C)).astype(np.int8)
    j = 6
    if planted == "class0_missing":          # class 0 rows are missing at SNP j, class 1 rows carry both alleles
        X[: N // 2, j] = 2
    else:                                    # class 0: allele 0 or missing; class 1: allele 1 -> {0, missing} | {1}
        X[: N // 2, j] = np.where(np.arange(N // 2) % 3 == 0, 2, 0)
        X[N // 2:, j] = 1
    fb, loss = train_forest_arrays(X, y, M, ctx, A, n_rounds=1, max_depth=2)
    assert fb["fb_left"][0] >= 0 and fb["fb_feat"][0] == j
    assert fb["fb_cond"][0] == np.float32(1.5 if cand == 3 else 0.5)
    assert fb["fb_default_left"][0] == (1 if cand == 2 else 0)
    ref, ref_loss = E.train(X, y, M, ctx, A, n_rounds=1, max_depth=2)
    _assert_equal_trees(fb, ref, planted)


def _close_f32(got, ref):
    """tests/test_gpu_parity.py's criterion for the forest base, restated: the tree walk and the margin sums are bit-exact, only the last
    bit of expf (device: correctly rounded; glibc: <= 0.502 ulp) and its knock-on through sum and division may differ"""
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 2.4e-7
    assert np.count_nonzero(got != ref) <= max(3, got.size // 20)


@pytest.mark.parametrize("impl", ["0", "1"])
@pytest.mark.parametrize("A", [3, 2])
def test_trained_model_runs_on_both_forest_kernels(ga, oracle, monkeypatch, impl, A):
    from gnomix_amd import _lib
    from gnomix_amd.train import train_forest_base, untrained_model
    monkeypatch.setenv("GNX_FOREST_IMPL", impl)     # read once per context
    ctx = _lib.Context(0)
    name = "A3" if A == 3 else "A2_binary"
    c = CASES[name]
    X, y, ref, _ = _case(name)
    d = untrained_model(c["C"], c["M"], A, 1, c["ctx"], "default", base="xgb")
    loss = train_forest_base(d, X, y, ctx=ctx, **c["kw"])
    assert d.base_kind == "forest" and d.fb_missing == 2 and d.fb_base_score == 0.5 and len(loss) == c["kw"]["n_rounds"] + 1
    _assert_equal_trees({k: getattr(d, k) for k in ref}, ref, "train_forest_base")
    b32, _ = ga.DeviceModel(d, ctx=ctx).base_predict(np.array(X), want_f32=True, want_f64=False)
    T = oracle.Trees(d.fb_tree_off, d.fb_left, d.fb_right, d.fb_feat, d.fb_cond, d.fb_tree_class, d.A, d.fb_base_score,
                     default_left=d.fb_default_left)
    _close_f32(b32, oracle.base_forest(T, d.fb_win_tree0, np.array(X), c["M"], c["ctx"], A, missing=2))


def test_learning_on_admixed_haplotypes(ga):
    from gnomix_amd import synth
    from gnomix_amd.train import train_forest_base, untrained_model
    C, M, A, N = 1237, 48, 5, 400
    X, y, _ = synth.synthetic_admixed_device(N // 2, C, M, A, "cuda:0", seed=11)
    d = untrained_model(C, M, A, 5, M // 2, "default", base="xgb")
    Xh = X.cpu().numpy()
    b0, _ = ga.DeviceModel(d).base_predict(Xh, want_f32=True, want_f64=False)
    acc0 = float(np.mean(np.argmax(b0, -1) == y))
    loss = train_forest_base(d, X, y)            # the device tensor: the _dev entry, XGBBase's 20 rounds of depth 4
    assert abs(loss[0] - math.log(A)) <= 1e-12   # every class at 1 / A before the first round
    assert loss[-1] < loss[0]
    b1, _ = ga.DeviceModel(d).base_predict(Xh, want_f32=True, want_f64=False)
    acc1 = float(np.mean(np.argmax(b1, -1) == y))
    assert np.allclose(b0, 1.0 / A, rtol=0, atol=1e-6)     # the placeholder: every class at 1 / A, accuracy that of always saying 0
    print("window accuracy: placeholder %.4f, trained %.4f; loss %.6f -> %.6f" % (acc0, acc1, loss[0], loss[-1]))
    assert acc1 > acc0 and acc1 > 1.0 / A, (acc0, acc1)


def test_public_path_trains_saves_and_loads(ga, tmp_path):
    from gnomix_amd.train import untrained_model
    C, M, A, S, ctx = 295, 24, 3, 5, 12         # W = 12 >= 2 S
    parts = []
    for i, n in enumerate((48, 48, 24)):
        X, y = _panel(n, C, M, A, seed=40 + i, miss=0.02)
        parts.append((X, y))
    g = ga.HipGnomix(untrained_model(C, M, A, S, ctx, "default", base="xgb"))
    g.train(tuple(parts), retrain_base=True, n_rounds=5)
    assert g.dev.data.base_kind == "forest" and len(g.dev.data.fb_tree_off) - 1 == (C // M) * 20 * A
    for k in ("base_train_acc", "smooth_train_acc", "base_val_acc", "smooth_val_acc"):
        assert 0.0 <= g.accuracies[k] <= 100.0
    assert g.accuracies["base_train_acc"] > 100.0 / A
    p = g.predict_proba(parts[2][0])
    path = g.save(str(tmp_path / "forest.gnx"))
    again = ga.HipGnomix.load(path)
    assert again.dev.data.base_kind == "forest"
    assert np.array_equal(again.predict_proba(parts[2][0]), p) and np.array_equal(again.predict(parts[2][0]), g.predict(parts[2][0]))


def test_random_forest_base_still_refuses(ga):
    from gnomix_amd import synth
    d = synth.synthetic_rforest_model(1237, 100, 3, n_trees=2, depth=2, seed=1)
    from gnomix_amd.base import HipBase
    with pytest.raises(NotImplementedError, match="random-forest"):
        HipBase(ga.DeviceModel(d)).train(np.zeros((4, 1237), np.int8), np.zeros((4, 12), np.int32))


def test_rejections(ga):
    import torch
    from gnomix_amd import _lib
    from gnomix_amd.train import train_forest_arrays
    C, M, ctx, N, A = 79, 24, 12, 20, 3
    X, y = _panel(N, C, M, A, seed=1)
    for bad in (3, -1):
        Xb = X.copy()
        Xb[4, 30] = bad
        with pytest.raises(_lib.GnxError) as e:
            train_forest_arrays(Xb, y, M, ctx, A, n_rounds=1)
        assert e.value.code == _lib.GNX_EINVAL
    for bad in (-1, A):      # gnx_train_gbt's rule: the host entry refuses a label outside [0, A)
        yb = y.copy()
        yb[3, 1] = bad
        with pytest.raises(_lib.GnxError) as e:
            train_forest_arrays(X, yb, M, ctx, A, n_rounds=1)
        assert e.value.code == _lib.GNX_EINVAL
    for depth in (0, 6):
        with pytest.raises(_lib.GnxError) as e:
            train_forest_arrays(X, y, M, ctx, A, n_rounds=1, max_depth=depth)
        assert e.value.code == _lib.GNX_EINVAL
    with pytest.raises(_lib.GnxError) as e:
        train_forest_arrays(X[:0], y[:0], M, ctx, A, n_rounds=1)
    assert e.value.code == _lib.GNX_EINVAL
    # the _dev entry reads neither back (as gnx_train_gbt_dev): a code of 3 trains as a 0, a label outside [0, A) belongs to no class
    Xb, yb = X.copy(), y.copy()
    Xb[4, 30] = 3
    yb[3, 1] = A
    fb, loss = train_forest_arrays(torch.as_tensor(Xb, device="cuda:0"), torch.as_tensor(yb, device="cuda:0"), M, ctx, A, n_rounds=2)
    X0 = Xb.copy()
    X0[4, 30] = 0
    ref, ref_loss = E.train(X0, yb, M, ctx, A, n_rounds=2)
    _assert_equal_trees(fb, ref, "code 3 as 0")
    assert np.max(np.abs(loss - ref_loss)) <= 1e-12
