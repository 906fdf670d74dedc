"""CPU: gnomix_amd.convert against REAL reference objects.  Bases trained by the reference's own LogisticRegressionBase / RFBase
(Base.train) are stored pickled, with query haplotypes and the reference's own predict_proba of them, in tests/golden/G20_convert_ref/
(tests/golden/make_golden.py G20).  A base is read back with gnomix_amd.refpickle (which never imports `src`), exported to flat arrays
and run through the oracle: the export must reproduce the reference's predict_proba."""
import os
import types

import numpy as np
import pytest

G20 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G20_convert_ref")


def _stored_base(name, use_sklearn=True):
    """(base read back from its pickle, the fixture's arrays)"""
    from gnomix_amd import refpickle
    base = refpickle.load_reference_pickle(os.path.join(G20, name + ".pkl.gz"), use_sklearn=use_sklearn)["base"]
    return base, np.load(os.path.join(G20, name + ".npz"))


class CRF_Smoother:  # name-compatible stand-ins: from_reference_model dispatches on the class name like the pickle would
    pass


class _FakeCRF:
    pass


def _fake_crf_smoother(A, S, rng):
    sm = CRF_Smoother()
    sm.S = S
    sm.calibrator = None
    sm.model = types.SimpleNamespace(CRF=_FakeCRF())
    st = rng.standard_normal((A, A))
    tr = rng.standard_normal((A, A))
    sm.model.CRF.state_features_ = {(str(a), str(y)): st[a, y] for a in range(A) for y in range(A)}
    sm.model.CRF.transition_features_ = {(str(a), str(y)): tr[a, y] for a in range(A) for y in range(A)}
    return sm, st, tr


def test_export_logistic_model_reproduces_reference(oracle):
    """a LogisticRegressionBase with its scikit-learn estimators rebuilt for real (refpickle's use_sklearn=True: cli.load_model's first
    choice)"""
    from gnomix_amd import convert, GnxModelData
    base, z = _stored_base("export_lr")
    assert type(base).__name__ == "LogisticRegressionBase" and type(base.models[0]).__name__ == "LogisticRegression"
    C, M, A, ctx = int(z["C"]), int(z["M"]), int(z["A"]), int(z["ctx"])
    W = C // M
    Xq, B_ref = z["Xq"], z["B_ref"]
    rng = np.random.RandomState(1)
    sm, st, tr = _fake_crf_smoother(A, 75, rng)
    model = types.SimpleNamespace(C=C, M=M, A=A, context=ctx, base=base, smooth=sm, snp_pos=np.arange(C), snp_ref=None,
                                  snp_alt=None, population_order=["a", "b", "c", "d"], gen_map_df={})
    d = convert.from_reference_model(model)
    assert isinstance(d, GnxModelData) and d.base_kind == "logistic" and d.smooth_kind == "crf"
    assert d.lr_coef.shape == (W, A, M + 2 * ctx + C - M * W)
    B = oracle.base_lr(Xq, d.M, d.context, d.lr_coef, d.lr_intercept)
    assert np.max(np.abs(B - B_ref)) < 1e-13
    assert np.array_equal(d.crf_state, st) and np.array_equal(d.crf_trans, tr)
    desc, keep = d.to_desc()   # the description the C ABI receives
    assert desc.lr_ldc == d.lr_coef.shape[2] and desc.C == C


def test_export_calibrator_and_string_kernel_lengths():
    from sklearn.isotonic import IsotonicRegression
    from gnomix_amd import convert
    rng = np.random.RandomState(2)
    iso = [IsotonicRegression(out_of_bounds="clip").fit(rng.rand(200).astype(np.float32), rng.rand(200) < 0.5) for _ in range(3)]
    c = convert.calibrator_arrays(iso)
    assert c["calib_is_f32"] and c["calib_off"][0] == 0 and len(c["calib_x"]) == c["calib_off"][-1]
    assert list(convert.string_kernel_lengths(349, "CovRSK_DP_triangular_numbers")) == [1, 4, 8, 39, 42, 117]
    assert list(convert.string_kernel_lengths(5, "string_kernel_DP_triangular_numbers_multithread")) == [1, 2, 3, 4, 5]
    with pytest.raises(NotImplementedError):
        convert.string_kernel_lengths(5, "poly_kernel")


def test_restricted_unpickle_of_real_reference_objects(oracle):
    """REAL reference objects (src.Base.models.LogisticRegressionBase / RFBase trained by Base.train) read back from their pickle
    with gnomix_amd.refpickle (which never imports `src`), converted, reproduce the reference's output"""
    from gnomix_amd import convert, refpickle
    rng = np.random.RandomState(2)
    for name in ("LogisticRegressionBase", "RFBase"):
        got, z = _stored_base(name)
        C, M, A, ctx = int(z["C"]), int(z["M"]), int(z["A"]), int(z["ctx"])
        Xq, B_ref = z["Xq"], z["B_ref"]
        sm, st, tr = _fake_crf_smoother(A, 75, rng)
        model = types.SimpleNamespace(C=C, M=M, A=A, context=ctx, base=None, smooth=sm, snp_pos=np.arange(C), snp_ref=None,
                                      snp_alt=None, population_order=["a", "b", "c"], gen_map_df=None)
        assert isinstance(got, refpickle.Stub) and type(got).__name__ == name and type(got).__module__ == "src.Base.models"
        model.base = got
        d = convert.from_reference_model(model)
        if name == "LogisticRegressionBase":
            B = oracle.base_lr(Xq, M, ctx, d.lr_coef, d.lr_intercept)
            assert np.max(np.abs(B - B_ref)) < 1e-13
        else:
            rf = {k[3:]: getattr(d, k) for k in ("rf_win_tree0", "rf_tree_off", "rf_left", "rf_right", "rf_feat", "rf_thr", "rf_value")}
            assert np.array_equal(oracle.base_rforest(rf, Xq, M, ctx, A), B_ref)
