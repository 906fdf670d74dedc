"""The 1-nearest-neighbour base (KNNBase) without a GPU: tests/knn_exact.py — the numpy restatement the GPU tests lean on — pinned
to the reference's own KNNBase output (tests/golden/G22_knn.npz) on every cell whose nearest label is unambiguous, the converter
(live KNeighborsClassifier and a stubbed pickle's attribute bag), every refusal, the .gnx round trip of both model forms, the C
description, untrained_model(base="knn") and fitting-is-storing."""
import ctypes
import io
import pickle
import types

import numpy as np
import pytest

from conftest import load_golden
import knn_exact as KE


def _golden_windows(g):
    return [(g["w%d_fit_X" % w], g["w%d_y" % w]) for w in range(int(g["C"]) // int(g["M"]))]


def _fit(seed=0, n=50, width=37, A=3, **kw):
    from sklearn.neighbors import KNeighborsClassifier
    rng = np.random.RandomState(seed)
    y = np.concatenate([np.arange(A), rng.randint(0, A, n - A)])
    f = rng.uniform(0.1, 0.9, (A, width))
    X = (rng.uniform(size=(n, width)) < f[y]).astype(np.int8)
    X[rng.uniform(size=X.shape) < 0.02] = 2
    return KNeighborsClassifier(**dict(dict(n_neighbors=1), **kw)).fit(X, y), X, y


def test_restatement_equals_the_references_KNNBase_G22_on_every_unambiguous_cell():
    g = load_golden("G22_knn.npz")
    C, M, A, ctx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    B, idx, amb = KE.predict(g["Xq"], _golden_windows(g), C, M, ctx, A)
    assert B.shape == g["B"].shape == (60, C // M, A)
    assert np.array_equal(amb, g["ambiguous"]) and amb.mean() <= 0.02      # the fixture's condition, restated
    assert np.array_equal(B[~amb], g["B"][~amb])
    assert set(np.unique(g["B"]).tolist()) == {0.0, 1.0} and np.all(g["B"].sum(-1) == 1.0)
    # the fixture is what the issue asks for: missing codes, a remainder, every class in every window, the fitted rows = the
    # window slices of the training matrix
    assert (g["Xt"] == 2).any() and C % M > 0 and all(len(np.unique(g["yt"][:, w])) == A for w in range(C // M))
    for (xf, yw), (xs, ys) in zip(_golden_windows(g), KE.shared_windows(g["Xt"], g["yt"], C, M, ctx)):
        assert np.array_equal(xf, xs) and np.array_equal(yw, ys)


def test_restatement_takes_the_lowest_index_among_ties():
    xf = np.array([[0, 1, 2], [1, 1, 1], [0, 1, 2], [1, 1, 1]], np.int8)
    yw = np.array([2, 0, 1, 1])
    Xq = np.array([[0, 1, 2], [1, 1, 1], [2, 2, 2], [3, 3, 3]], np.int8)
    B, idx, amb = KE.predict(Xq, [(xf, yw)], 3, 2, 0, 3)    # C = 3, M = 2: one window of width 3 (M + rem)
    assert idx[:, 0].tolist() == [0, 1, 1, 1] and amb[:, 0].tolist() == [True, True, True, True]
    assert np.array_equal(B[:, 0], np.eye(3)[[2, 0, 0, 0]])
    assert KE.tied_classes(Xq, xf, yw) == [{1, 2}, {0, 1}, {0, 1}, {0, 1}]


def test_converter_from_a_live_classifier_and_from_an_attribute_bag_agree():
    from gnomix_amd.convert import knn_window_from_sklearn
    from gnomix_amd.refpickle import load_reference_pickle
    for seed, width, A in ((0, 37, 3), (1, 300, 4), (2, 9, 2)):
        m, X, y = _fit(seed, width=width, A=A)
        w = knn_window_from_sklearn(m, width, A)
        assert w["xfit"].dtype == np.int8 and w["y"].dtype == np.int32
        assert np.array_equal(w["xfit"], X) and np.array_equal(w["y"], y)
        bag = load_reference_pickle(io.BytesIO(pickle.dumps(m)), use_sklearn=False)
        assert type(bag).__name__ == "KNeighborsClassifier" and not hasattr(bag, "predict_proba")
        wb = knn_window_from_sklearn(bag, width, A)
        assert np.array_equal(wb["xfit"], w["xfit"]) and np.array_equal(wb["y"], w["y"])
    # labels go through classes_: a window that lacks class 1 keeps the label 2
    from sklearn.neighbors import KNeighborsClassifier
    m = KNeighborsClassifier(n_neighbors=1).fit(np.array([[0, 1], [1, 1], [2, 0]]), np.array([2, 0, 2]))
    assert knn_window_from_sklearn(m, 2, 3)["y"].tolist() == [2, 0, 2] and m._y.tolist() == [1, 0, 1]
    # float fit data that hold whole codes are accepted
    m = KNeighborsClassifier(n_neighbors=1).fit(np.array([[0., 1.], [2., 1.]]), np.array([0, 1]))
    assert knn_window_from_sklearn(m, 2, 2)["xfit"].tolist() == [[0, 1], [2, 1]]


def test_from_reference_model_keeps_the_per_window_arrays():
    from gnomix_amd.convert import from_reference_model
    C, M, ctx, A = 83, 40, 3, 3
    widths = [M + 2 * ctx, M + 2 * ctx + C % M]
    fits = [_fit(5 + w, n=20 + 7 * w, width=widths[w]) for w in range(2)]

    class CRF_Smoother:   # the attributes the converter reads of the reference's CRF smoother (src/Smooth/models.py:27-32)
        S = 1
        calibrator = None
        model = types.SimpleNamespace(CRF=types.SimpleNamespace(state_features_={(str(a), str(a)): 1.5 for a in range(A)},
                                                                transition_features_={("0", "1"): -0.25}))

    model = types.SimpleNamespace(C=C, M=M, A=A, context=ctx, smooth=CRF_Smoother(), base=types.SimpleNamespace(models=[f[0] for f in fits]),
                                  snp_pos=np.arange(C), snp_ref=np.array(["A"] * C), snp_alt=np.array(["G"] * C),
                                  population_order=["p%d" % a for a in range(A)], gen_map_df=None)
    d = from_reference_model(model)
    assert d.base_kind == "knn" and d.knn_X is None and len(d.knn) == 2
    for w, (m, X, y) in enumerate(fits):
        assert np.array_equal(d.knn[w]["xfit"], X) and np.array_equal(d.knn[w]["y"], y)
    assert [x.shape[0] for x, _ in d.knn_windows()] == [20, 27]


REFUSED = [
    ("n_neighbors", dict(n_neighbors=3), "n_neighbors"),
    ("weights", dict(weights="distance"), "weights"),
    ("weights_callable", dict(weights=lambda d: 1.0 / (1e-9 + d)), "weights"),
    ("manhattan", dict(metric="manhattan"), "metric"),
    ("minkowski_p1", dict(p=1), "metric"),
    ("minkowski_p3", dict(p=3), "metric"),
    ("chebyshev", dict(metric="chebyshev"), "metric"),
]


@pytest.mark.parametrize("name,kw,says", REFUSED, ids=[r[0] for r in REFUSED])
def test_converter_refuses_other_classifiers(name, kw, says):
    from gnomix_amd.convert import knn_window_from_sklearn
    m, X, y = _fit(0, **kw)
    with pytest.raises(NotImplementedError, match=says):
        knn_window_from_sklearn(m, X.shape[1], 3)


def test_converter_refuses_fit_data_that_are_not_snp_codes_and_bad_labels():
    from gnomix_amd.convert import knn_window_from_sklearn
    m, X, y = _fit(1)

    def bag(**kw):
        return types.SimpleNamespace(**dict(dict(n_neighbors=1, weights="uniform", metric="minkowski", p=2, _fit_X=X.astype(np.float64),
                                                 _y=m._y, classes_=m.classes_), **kw))

    assert np.array_equal(knn_window_from_sklearn(bag(), X.shape[1], 3)["xfit"], X)
    for bad in (0.5, 3.0, -1.0, np.nan):
        fx = X.astype(np.float64)
        fx[1, 2] = bad
        with pytest.raises(ValueError, match="_fit_X"):
            knn_window_from_sklearn(bag(_fit_X=fx), X.shape[1], 3)
    with pytest.raises(ValueError, match="_fit_X"):
        knn_window_from_sklearn(bag(), X.shape[1] + 1, 3)            # not this window's width
    with pytest.raises(ValueError, match="_fit_X"):
        knn_window_from_sklearn(bag(_fit_X=X[:0].astype(np.float64), _y=m._y[:0]), X.shape[1], 3)   # no fit row
    with pytest.raises(ValueError, match="classes_"):
        knn_window_from_sklearn(bag(), X.shape[1], 2)                # label 2 with A = 2
    with pytest.raises(ValueError, match="classes_"):
        knn_window_from_sklearn(bag(classes_=np.array([0.0, 1.5, 2.0])), X.shape[1], 3)
    with pytest.raises(ValueError, match="_y"):
        knn_window_from_sklearn(bag(_y=m._y[:-1]), X.shape[1], 3)


def test_untrained_model_fitting_is_storing_gnx_round_trip_and_description(tmp_path):
    from gnomix_amd import GnxModelData, _lib
    from gnomix_amd.train import untrained_model, train_knn_base, window_columns
    C, M, ctx, A = 83, 40, 3, 3
    d = untrained_model(C, M, A, 1, ctx, "default", base="knn")
    assert d.base_kind == "knn" and d.smooth_kind == "xgb" and d.knn is None
    assert d.knn_X.shape == (1, C) and d.knn_y.shape == (1, 2) and not d.knn_X.any() and not d.knn_y.any()
    with pytest.raises(ValueError, match="knn"):
        untrained_model(C, M, A, 1, ctx, "default", base="lda")
    rng = np.random.RandomState(0)
    X, y = rng.randint(0, 3, (31, C)).astype(np.int8), rng.randint(0, A, (31, 2))
    assert train_knn_base(d, X, y) == {"n_fit": 31}
    assert np.array_equal(d.knn_X, X) and np.array_equal(d.knn_y, y) and d.knn_y.dtype == np.int32
    for bad_X, bad_y in ((X[:, :-1], y), (np.where(X == 2, 3, X), y), (-X, y), (X + 0.5, y), (X, y[:-1]), (X, y + 1), (X, y - 1), (X[:0], y[:0])):
        with pytest.raises(ValueError):
            train_knn_base(untrained_model(C, M, A, 1, ctx, "default", base="knn"), bad_X, bad_y)
    path = str(tmp_path / "knn.gnx")
    d.save(path)
    again = GnxModelData.load(path)
    assert again.base_kind == "knn" and again.knn is None
    assert np.array_equal(again.knn_X, X) and np.array_equal(again.knn_y, y)
    desc, keep = again.to_desc()
    assert desc.abi_version == _lib.GNX_ABI_VERSION == 16 and desc.base_kind == _lib.BASE_KNN == 5
    arr = ctypes.cast(desc.knn, ctypes.POINTER(_lib.KnnWindow))
    for w in range(2):
        cols = window_columns(C, M, ctx, w)
        assert arr[w].n_fit == 31 and arr[w].width == len(cols) == d.window_width(w)
        got = np.ctypeslib.as_array(ctypes.cast(arr[w].xfit, ctypes.POINTER(ctypes.c_int8)), (31, len(cols)))
        assert np.array_equal(got, X[:, cols])
        assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(arr[w].y, ctypes.POINTER(ctypes.c_int32)), (31,)), y[:, w])
        assert np.array_equal(KE.window_columns(C, M, ctx, w), cols)
    # the per-window form of a converted pickle survives the file too, with different row counts per window
    per = GnxModelData(C=C, M=M, A=A, S=1, context=ctx, base_kind="knn",
                       knn=[dict(xfit=rng.randint(0, 3, (4 + w, d.window_width(w))).astype(np.int8), y=rng.randint(0, A, 4 + w).astype(np.int32))
                            for w in range(2)])
    per.save(path)
    again = GnxModelData.load(path)
    assert again.knn_X is None and len(again.knn) == 2
    for a, b in zip(again.knn, per.knn):
        assert set(a) == {"xfit", "y"} and np.array_equal(a["xfit"], b["xfit"]) and np.array_equal(a["y"], b["y"])
    desc, keep = again.to_desc()
    arr = ctypes.cast(desc.knn, ctypes.POINTER(_lib.KnnWindow))
    assert [arr[w].n_fit for w in range(2)] == [4, 5]
    with pytest.raises(ValueError):
        GnxModelData(C=C, M=M, A=A, S=1, context=ctx, base_kind="knn").to_desc()


def test_header_and_binding_agree_on_the_new_fields():
    import os
    import re
    from gnomix_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "gnomix_hip.h")).read()
    assert re.search(r"#define GNX_ABI_VERSION 16\b", h) and re.search(r"GNX_BASE_KNN = 5\b", h)
    body = re.search(r"typedef struct gnx_knn_window \{(.*?)\} gnx_knn_window;", h, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.KnnWindow._fields_]
    desc = re.search(r"typedef struct gnx_model_desc \{(.*?)\} gnx_model_desc;", h, re.S).group(1)
    assert re.findall(r"(\w+);", desc)[-1] == "knn" == _lib.ModelDesc._fields_[-1][0]      # appended at the end
    assert ctypes.sizeof(_lib.KnnWindow) == 24
