"""A reference `model.pkl` pickled by an OLDER scikit-learn / numpy than the one reading it (the closable half of SURVEY 8(f).1:
the published bundles were written by scikit-learn 1.0.1 / numpy 1.20.3, requirements.txt:2,6; the test interpreter has 1.7.2 / 2.2).

tests/golden/make_refpickle_py39.py, run under Python 3.9 with scikit-learn 0.24.2 / numpy 1.26.4 and the reference importable, trains
small `src.model.Gnomix` objects with the reference's own LogisticRegressionBase / CovRSKBase / RFBase, pickles them as Gnomix.save does
and stores the reference's OWN predict_proba next to them, in tests/golden/refpickle_py39/.  Here, under Python 3.10:

    load_reference_pickle (use_sklearn = False AND True; cli.load_model's fallback order) -> from_reference_model -> oracle
    == the old environment's reference output (<= 1e-12, arg-max labels identical); under -m gpu the HIP path as well."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def old_pickles():
    out = os.path.join(ROOT, "tests", "golden", "refpickle_py39")
    meta = np.load(os.path.join(out, "lr.npz"))
    import sklearn
    # the point of the test: a scikit-learn MAJOR version gap between writer and reader
    assert str(meta["sklearn_version"]).split(".")[0] != sklearn.__version__.split(".")[0], (str(meta["sklearn_version"]), sklearn.__version__)
    return out


def _load_both_modes(path):
    """(mode, model or exception) for use_sklearn False and True — cli.load_model tries True first and falls back to False"""
    from gnomix_amd import refpickle
    out = []
    for use in (False, True):
        try:
            out.append((use, refpickle.load_reference_pickle(path, use_sklearn=use)))
        except Exception as e:  # noqa: BLE001 - an old estimator the new scikit-learn refuses to rebuild is a legitimate outcome of mode True
            out.append((use, e))
    return out


def _oracle_base(oracle, d, Xq):
    if d.base_kind == "logistic":
        return oracle.base_lr(Xq, d.M, d.context, d.lr_coef, d.lr_intercept)
    if d.base_kind == "covrsk":
        wins = [dict(Xfit=w["xfit"], Ms=list(w["ms"]), support=w["support"], dual=w["dual_coef"], intercept=w["intercept"],
                     probA=w["prob_a"], probB=w["prob_b"], n_support=w["n_support"]) for w in d.svc]
        return oracle.base_covrsk(Xq, d.M, d.context, wins)
    if d.base_kind == "rforest":
        rf = {k[3:]: getattr(d, k) for k in ("rf_win_tree0", "rf_tree_off", "rf_left", "rf_right", "rf_feat", "rf_thr", "rf_value")}
        return oracle.base_rforest(rf, Xq, d.M, d.context, d.A)
    raise AssertionError(d.base_kind)


@pytest.mark.parametrize("name,kind", [("lr", "logistic"), ("covrsk", "covrsk"), ("rf", "rforest")])
def test_pickle_from_older_sklearn_converts_and_reproduces_the_reference(old_pickles, oracle, name, kind):
    from gnomix_amd import convert, refpickle
    z = np.load(os.path.join(old_pickles, name + ".npz"))
    Xq, B_ref = z["Xq"], z["B_ref"]
    path = os.path.join(old_pickles, name + ".pkl.gz")
    modes = _load_both_modes(path)
    assert not isinstance(modes[0][1], Exception), "attribute-bag mode (use_sklearn=False) must always read the pickle: %r" % (modes[0][1],)
    worked = 0
    for use, model in modes:
        if isinstance(model, Exception):
            continue            # mode True may refuse an estimator of another major version: the command line then falls back to mode False
        worked += 1
        # nothing of the reference's `src` package (nor of xgboost / crfsuite) was imported to read it
        assert type(model).__module__ == "src.model" and isinstance(model, refpickle.Stub)
        d = convert.from_reference_model(model)
        assert d.base_kind == kind and d.smooth_kind == "crf" and (d.C, d.M, d.A) == (int(z["C"]), int(z["M"]), int(z["A"]))
        assert np.array_equal(d.crf_state, z["crf_state"]) and np.array_equal(d.crf_trans, z["crf_trans"])
        B = _oracle_base(oracle, d, Xq)
        assert B.shape == B_ref.shape
        assert np.max(np.abs(B - B_ref)) <= 1e-12, (name, use, float(np.max(np.abs(B - B_ref))))
        assert np.array_equal(B.argmax(-1), B_ref.argmax(-1))
    assert worked >= 1


def test_command_line_loader_reads_the_old_pickle(old_pickles, tmp_path):
    """gnomix_amd.cli.load_model's own order (rebuild scikit-learn objects, fall back to attribute bags) up to the point where a device
    is needed: the converted model of the old LogisticRegression pickle round-trips through .gnx"""
    from gnomix_amd import convert, refpickle
    from gnomix_amd.model import GnxModelData
    path = os.path.join(old_pickles, "lr.pkl.gz")
    try:
        ref_model = refpickle.load_reference_pickle(path)
    except Exception:
        ref_model = refpickle.load_reference_pickle(path, use_sklearn=False)
    d = convert.from_reference_model(ref_model)
    out = str(tmp_path / "lr.gnx")
    d.save(out)
    d2 = GnxModelData.load(out)
    assert np.array_equal(d2.lr_coef, d.lr_coef) and d2.smooth_kind == "crf" and list(d2.population_order) == ["p0", "p1", "p2"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lr", "covrsk", "rf"])
def test_hip_path_on_the_old_pickle(old_pickles, name):
    import gnomix_amd
    from gnomix_amd import convert, refpickle
    z = np.load(os.path.join(old_pickles, name + ".npz"))
    d = convert.from_reference_model(refpickle.load_reference_pickle(os.path.join(old_pickles, name + ".pkl.gz"), use_sklearn=False))
    dev = gnomix_amd.DeviceModel(d)
    _, B = dev.base_predict(z["Xq"])   # (f32, f64): the f64 probabilities are what the reference returns
    assert np.max(np.abs(B - z["B_ref"])) <= 1e-12 and np.array_equal(B.argmax(-1), z["B_ref"].argmax(-1))
