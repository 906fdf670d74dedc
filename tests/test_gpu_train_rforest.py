"""Training the random-forest base (RFBase) on the device: gnx_train_rforest / train_rforest_arrays / HipBase.train.

The trainer is held to tests/rf_exact.py, the plain-Python restatement of scikit-learn's chain (itself held to live scikit-learn bit
for bit in tests/test_rf_host.py), and to the reference's own RFBase fit (G26): every rf_* array equal bit for bit."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rf_exact as E  # noqa: E402

pytestmark = pytest.mark.gpu
RF_KEYS = ("rf_win_tree0", "rf_tree_off", "rf_left", "rf_right", "rf_feat", "rf_thr", "rf_value")
# (C, M, ctx, A, N): the last window 237 wide, 140 (tree, class) rows = a padded third macro-tile of 64 and a padded ninth tile of 16,
# N no multiple of 64 and more than one chunk;  two classes, one chunk;  four identical row pairs with different labels (impure nodes
# whose every column is constant, leaves above depth 4), N = 8
SHAPES = {"seven": (1237, 100, 50, 7, 150), "two": (403, 50, 25, 2, 37), "pairs": (131, 24, 12, 3, 8)}
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _problem(name):
    """-> (geometry, X, y, seeds, reference rf_* arrays, counters), computed once"""
    if name not in _cache:
        C, M, cx, A, N = SHAPES[name]
        if name == "pairs":
            X, _ = E.identical_pairs(N // 2, C, seed=5)
            y = np.tile(np.array([0, 1, 0, 2, 1, 2, 0, 1], np.int32)[:, None], (1, C // M))
        else:
            X, _ = E.make_problem(A, C, N, 40 + A)
            y = E.window_labels(X, M, A, 41 + A)
        seeds = np.random.RandomState(len(name)).randint(2 ** 31 - 1, size=C // M).astype(np.int64)
        cnt = E.new_counters()
        ref = E.fit_windows(X, y, M, cx, A, seeds, counters=cnt)
        for v in ref.values():
            v.setflags(write=False)
        _cache[name] = ((C, M, cx, A, N), X, y, seeds, ref, cnt)
    return _cache[name]


def _equal(got, ref):
    for k in RF_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), (k, int(np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))[0]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_trees_equal_the_restatement_bit_for_bit(ctx, name):
    from gnomix_amd.train import train_rforest_arrays
    (C, M, cx, A, N), X, y, seeds, ref, cnt = _problem(name)
    print(name, "nodes", len(ref["rf_left"]), cnt)
    if name == "pairs":
        assert cnt["all_constant_search"] > 0 and cnt["leaf_above_max_depth"] > 0
    else:
        assert cnt["known_constant_drawn"] > 0 and cnt["constant_found"] > 0 and cnt["threshold_one"] > 0
    _equal(train_rforest_arrays(X, y, M, cx, A, seeds, ctx=ctx), ref)


def test_other_depths_and_tree_counts_equal_the_restatement(ctx):
    from gnomix_amd.train import train_rforest_arrays
    (C, M, cx, A, N), X, y, seeds, _, _ = _problem("two")
    for T, D in ((3, 5), (5, 1)):
        _equal(train_rforest_arrays(X, y, M, cx, A, seeds, n_trees=T, max_depth=D, ctx=ctx), E.fit_windows(X, y, M, cx, A, seeds, T, D))


def test_device_pointer_form_equals_the_host_form(ctx):
    import torch
    from gnomix_amd.train import train_rforest_arrays
    (C, M, cx, A, N), X, y, seeds, ref, _ = _problem("two")
    pitch = C + 13                               # rows with a pitch
    dX = torch.zeros((N, pitch), dtype=torch.int8, device="cuda")
    dX[:, :C] = torch.as_tensor(X, device="cuda")
    _equal(train_rforest_arrays(dX[:, :C], y, M, cx, A, seeds, ctx=ctx), ref)


def test_reference_fit_G26_trees_and_probabilities(ctx):
    from gnomix_amd.model import DeviceModel
    from gnomix_amd.train import train_rforest_base, untrained_model
    g = load_golden("G26_rf_fit.npz")
    C, M, cx, A = int(g["C"]), int(g["M"]), int(g["ctx"]), int(g["A"])
    d = untrained_model(C, M, A, 3, cx, "default", base="rf", seed=1)      # (W = 8 windows: a smoother of 3)
    info = train_rforest_base(d, g["X"], g["y"], seeds=g["seeds"], ctx=ctx)
    assert info["n_trees"] == 20 and info["max_depth"] == 4 and info["n_nodes"] == len(g["rf_left"])
    _equal({k: getattr(d, k) for k in RF_KEYS}, g)
    _, B = DeviceModel(d, ctx=ctx).base_predict(g["Xq"], want_f32=False, want_f64=True)
    assert B.dtype == np.float64 and np.array_equal(B, g["B"])


def test_trains_through_the_public_interface(ctx, tmp_path):
    import lda_exact as LE
    from gnomix_amd import HipGnomix, GnxModelData
    from gnomix_amd.train import untrained_model
    (C, M, cx, A), data = LE.e2e_data(seed=7)
    models = []
    for _ in range(2):
        np.random.seed(1234)
        model = HipGnomix(untrained_model(C, M, A, 3, cx, "default", base="rf", seed=1), ctx=ctx)
        model.train(data=data, retrain_base=True, evaluate=True)
        models.append(model)
    model = models[0]
    d = model.dev.data
    print("accuracies", model.accuracies)
    assert d.base_kind == "rforest" and d.smooth_kind == "xgb" and len(d.rf_tree_off) == (C // M) * 20 + 1
    assert model.accuracies["base_train_acc"] > 100.0 / A
    for k in RF_KEYS:                            # the same global seed, the same model
        assert np.array_equal(getattr(d, k), getattr(models[1].dev.data, k)), k
    X_q = data[2][0]
    p, lab = model.predict_proba(X_q), model.predict(X_q)
    assert np.array_equal(p, models[1].predict_proba(X_q))
    path = str(tmp_path / "rf.gnx")
    model.save(path)
    again = HipGnomix(GnxModelData.load(path), ctx=ctx)
    assert again.dev.data.base_kind == "rforest" and np.array_equal(again.predict_proba(X_q), p) and np.array_equal(again.predict(X_q), lab)
    with pytest.raises(NotImplementedError, match="random-forest base"):     # a loaded .gnx carries no hyper-parameters
        again.base.train(*data[0])


def test_rejections(ctx):
    from gnomix_amd import _lib
    from gnomix_amd.train import train_rforest_arrays, train_rforest_base, untrained_model
    (C, M, cx, A, N), X, y, seeds, _, _ = _problem("two")
    bad = X.copy()
    bad[N - 1, C - 1] = 3
    with pytest.raises(_lib.GnxError, match="code") as e:
        train_rforest_arrays(bad, y, M, cx, A, seeds, ctx=ctx)
    assert e.value.code == _lib.GNX_EINVAL
    bad = y.copy()
    bad[N - 1, C // M - 1] = A
    with pytest.raises(_lib.GnxError, match="label") as e:
        train_rforest_arrays(X, bad, M, cx, A, seeds, ctx=ctx)
    assert e.value.code == _lib.GNX_EINVAL
    y1 = y.copy()
    y1[:, 3] = 0
    with pytest.raises(ValueError, match="window 3: class 1 has no row"):
        train_rforest_base(untrained_model(C, M, A, 3, cx, "default", base="rf"), X, y1, seeds=seeds, ctx=ctx)
    # decided on the arguments, before any pointer is followed: N >= 2^24, a depth outside 1..5; on the host form a weight above 127
    p = X.ctypes.data
    W = C // M
    wt, st = np.full((W, 20, N), 1, np.uint8), np.ones((W, 20), np.uint32)
    args = lambda n, dep, w: (ctx.h, p, n, C, y.ctypes.data, C, M, cx, A, 20, dep, w.ctypes.data, st.ctypes.data) + (p,) * 8
    for fn in (ctx.lib.gnx_train_rforest, ctx.lib.gnx_train_rforest_dev):
        assert fn(*args(1 << 24, 4, wt)) == _lib.GNX_EINVAL and "2^24" in ctx.lib.gnx_last_error(ctx.h).decode()
        assert fn(*args(N, 6, wt)) == _lib.GNX_EINVAL and fn(*args(N, 0, wt)) == _lib.GNX_EINVAL
    wt[W - 1, 19, N - 1] = 128
    assert ctx.lib.gnx_train_rforest(*args(N, 4, wt)) == _lib.GNX_EINVAL and "127" in ctx.lib.gnx_last_error(ctx.h).decode()
