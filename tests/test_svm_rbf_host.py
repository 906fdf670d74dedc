"""The RBF SVC base (SVMBase) without a GPU: the converter (live sklearn fit -> window dict -> .gnx round trip -> C description,
the stubbed-pickle route, refusals) and tests/svm_rbf_exact.py — the numpy restatement the GPU tests lean on — pinned to the
reference's own SVMBase output (tests/golden/G21_svm_rbf.npz) within 1e-12."""
import io
import pickle
import types

import numpy as np
import pytest

from conftest import load_golden
import svm_rbf_exact as E


def _fit(seed=0, n=60, width=37, A=3):
    from sklearn.svm import SVC
    rng = np.random.RandomState(seed)
    y = np.concatenate([np.arange(A), rng.randint(0, A, n - A)])
    f = rng.uniform(0.1, 0.9, (A, width))
    X = (rng.uniform(size=(n, width)) < f[y]).astype(np.int8)
    X[rng.uniform(size=X.shape) < 0.02] = 2
    return SVC(C=100., gamma=0.001, probability=True, random_state=np.random.RandomState(seed)).fit(X, y), X, y


def test_converter_round_trip_and_description(tmp_path):
    from gnomix_amd import GnxModelData, _lib
    from gnomix_amd.convert import svc_window_from_sklearn
    from gnomix_amd.model import svc_window_is_rbf
    from gnomix_amd.train import untrained_model
    C, M, ctx, A = 83, 40, 3, 3
    d = untrained_model(C, M, A, 1, ctx, "default", base="svm")
    fits = [_fit(w, width=d.window_width(w))[0] for w in range(d.W)]
    d.svc = [svc_window_from_sklearn(m, d.window_width(w)) for w, m in enumerate(fits)]
    for w, (m, s) in enumerate(zip(fits, d.svc)):
        assert svc_window_is_rbf(s) and float(s["gamma"]) == m._gamma == 0.001
        assert s["xfit"].dtype == np.int8 and np.array_equal(s["xfit"], m.support_vectors_)
        assert np.array_equal(s["support"], np.arange(len(m.support_))) and np.array_equal(s["n_support"], m._n_support)
        assert np.array_equal(s["dual_coef"], m._dual_coef_) and np.array_equal(s["prob_a"], m._probA)
    path = str(tmp_path / "svm.gnx")
    d.save(path)
    again = GnxModelData.load(path)
    assert again.base_kind == "covrsk" and len(again.svc) == d.W
    for a, b in zip(again.svc, d.svc):
        assert svc_window_is_rbf(a) and set(a) == set(b)
        for k in b:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    desc, keep = again.to_desc()
    import ctypes
    arr = ctypes.cast(desc.svc, ctypes.POINTER(_lib.SvcWindow))
    for w in range(d.W):
        assert arr[w].kernel_kind == _lib.SVC_KERNEL_RBF == 3 and arr[w].gamma == 0.001 and arr[w].width == d.window_width(w)
        assert arr[w].n_sv == len(fits[w].support_) and not arr[w].ms
    # an older .gnx (string-kernel windows carry no tag) still reads as a string kernel
    assert not svc_window_is_rbf(dict(ms=np.arange(3)))


def test_from_reference_model_and_the_stubbed_pickle_reach_the_same_arrays():
    from gnomix_amd.convert import from_reference_model
    from gnomix_amd.refpickle import load_reference_pickle
    C, M, ctx, A = 83, 40, 3, 3
    widths = [M + 2 * ctx, M + 2 * ctx + C % M]
    fits = [_fit(5 + w, width=widths[w])[0] for w in range(2)]

    class CRF_Smoother:   # the attributes the converter reads of the reference's CRF smoother (src/Smooth/models.py:27-32)
        S = 1
        calibrator = None
        model = types.SimpleNamespace(CRF=types.SimpleNamespace(state_features_={(str(a), str(a)): 1.5 for a in range(A)},
                                                                transition_features_={("0", "1"): -0.25}))

    model = types.SimpleNamespace(C=C, M=M, A=A, context=ctx, smooth=CRF_Smoother(), base=types.SimpleNamespace(models=fits),
                                  snp_pos=np.arange(C), snp_ref=np.array(["A"] * C), snp_alt=np.array(["G"] * C),
                                  population_order=["p%d" % a for a in range(A)], gen_map_df=None)
    d = from_reference_model(model)
    assert d.base_kind == "covrsk" and d.smooth_kind == "crf" and len(d.svc) == 2 and d.crf_trans[0, 1] == -0.25
    svc = d.svc
    for w, m in enumerate(fits):
        assert str(svc[w]["kernel"]) == "rbf" and float(svc[w]["gamma"]) == m._gamma
        assert np.array_equal(svc[w]["xfit"], m.support_vectors_) and svc[w]["xfit"].shape[1] == widths[w]
        assert np.array_equal(svc[w]["dual_coef"], m._dual_coef_) and np.array_equal(svc[w]["n_support"], m._n_support)
    bags = load_reference_pickle(io.BytesIO(pickle.dumps(fits)), use_sklearn=False)
    from gnomix_amd.convert import svc_window_from_sklearn
    for w, bag in enumerate(bags):
        assert type(bag).__name__ == "SVC" and not hasattr(bag, "predict_proba")
        s = svc_window_from_sklearn(bag, widths[w])
        for k in svc[w]:
            assert np.array_equal(np.asarray(s[k]), np.asarray(svc[w][k])), k


def test_support_rows_that_are_not_snp_codes_are_refused():
    from gnomix_amd.convert import svc_window_from_sklearn
    m, X, y = _fit(1)
    for bad in (0.5, 3.0, -1.0, np.nan):
        sv = m.support_vectors_.copy()
        sv[1, 2] = bad
        bag = types.SimpleNamespace(kernel="rbf", support_vectors_=sv, _gamma=m._gamma, _dual_coef_=m._dual_coef_, _intercept_=m._intercept_,
                                    _probA=m._probA, _probB=m._probB, _n_support=m._n_support)
        with pytest.raises(ValueError, match="support_vectors_"):
            svc_window_from_sklearn(bag, X.shape[1])
    bag = types.SimpleNamespace(kernel="rbf", support_vectors_=m.support_vectors_, _gamma=0.0, _dual_coef_=m._dual_coef_,
                                _intercept_=m._intercept_, _probA=m._probA, _probB=m._probB, _n_support=m._n_support)
    with pytest.raises(ValueError, match="_gamma"):
        svc_window_from_sklearn(bag, X.shape[1])
    with pytest.raises(NotImplementedError):
        svc_window_from_sklearn(types.SimpleNamespace(kernel="sigmoid"), X.shape[1])


def test_restatement_decision_values_equal_sklearn_bit_for_bit():
    from gnomix_amd.convert import svc_window_from_sklearn
    from sklearn.svm import SVC
    for seed, A, width in ((0, 3, 37), (1, 4, 300), (2, 2, 65)):
        m, X, y = _fit(seed, n=120, width=width, A=A)
        Xq = _fit(seed + 50, n=40, width=width, A=A)[1]
        win = svc_window_from_sklearn(m, width)
        m.decision_function_shape = "ovo"
        ref = m.decision_function(Xq).reshape(len(Xq), -1)
        if A == 2:
            ref = -ref   # sklearn's public decision_function flips the binary case; libsvm's own value is what predict_proba uses
        assert np.array_equal(E.decision_values(win, Xq), ref)
        assert np.max(np.abs(E.predict_proba_window(win, Xq) - m.predict_proba(Xq))) <= 1e-12


def test_restatement_equals_the_references_SVMBase_G21():
    g = load_golden("G21_svm_rbf.npz")
    C, M, ctx = int(g["C"]), int(g["M"]), int(g["ctx"])
    B = E.predict_proba(E.golden_windows(g), g["Xq"], C, M, ctx)
    err = np.max(np.abs(B - g["B"]))
    print("restatement vs G21 predict_proba: max |diff| = %.3g" % err)
    assert B.shape == g["B"].shape and err <= 1e-12
    assert np.array_equal(np.argmax(B, -1), np.argmax(g["B"], -1))
    assert (g["Xt"] == 2).any() and C % M > 0 and all(len(np.unique(g["yt"][:, w])) == int(g["A"]) for w in range(C // M))
