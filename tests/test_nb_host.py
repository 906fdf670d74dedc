"""The three Naive-Bayes bases without a GPU: tests/nb_exact.py — the numpy restatement the GPU tests lean on — pinned to the
reference's own NB*Base output (tests/golden/G23_nb.npz), the closed forms of the fit against live scikit-learn, the converter (live
estimator and attribute bag, absent classes), every refusal, the .gnx round trip, the C structure and untrained_model."""
import ctypes
import os
import re
import subprocess
import types
import warnings

import numpy as np
import pytest

from conftest import load_golden
import nb_exact as NE

from nb_exact import KINDS, ATTRS, golden_windows, sk_estimator, numpy_counts, degenerate_panel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_the_references_base_G23(kind):
    g = load_golden("G23_nb.npz")
    C, M, A, ctx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    B, J = NE.predict(g["Xq"], golden_windows(g, kind), C, M, ctx, A)
    ref = g[kind + "_B"]
    err = np.abs(B - ref).max()
    print(kind, "max |restatement - reference| =", err)
    assert B.shape == ref.shape == (60, C // M, A)
    assert err <= 1e-12
    assert np.array_equal(B.argmax(-1), ref.argmax(-1))
    assert ref.max() <= 1 - 1e-9 and (g["Xt"] == 2).any() and (g["Xq"] == 2).any() and C % M > 0


@pytest.mark.parametrize("panel", ("g23", "degenerate"))
def test_closed_forms_equal_live_scikit_learn(panel):
    from gnomix_amd.train import nb_fit_from_counts
    if panel == "g23":
        g = load_golden("G23_nb.npz")
        C, M, A, ctx, X, y = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"]), g["Xt"], g["yt"]
    else:
        C, M, A, ctx, X, y, _ = degenerate_panel()
    n1, n2, cc = numpy_counts(X, y, C, M, ctx, A)
    mono = 0
    for w in range(C // M):
        cols = NE.window_columns(C, M, ctx, w)
        Xw = X[:, cols].astype(np.float64)
        for kind in KINDS:
            sk = sk_estimator(kind).fit(Xw, y[:, w])
            fit = nb_fit_from_counts(kind, n1[w, :, :len(cols)], n2[w, :, :len(cols)], cc[w])
            assert np.array_equal(fit["classes_"], sk.classes_)
            if kind == "gaussian":
                assert np.array_equal(fit["theta_"], sk.theta_) and np.array_equal(fit["class_prior_"], sk.class_prior_)
                bound = (cc[w][cc[w] > 0].astype(np.float64)[:, None] + 10) * 2.0 ** -53
                rel = np.abs(fit["var_"] - sk.var_) / sk.var_
                assert np.all(rel <= bound), (rel / bound).max()
            else:
                assert np.array_equal(fit["feature_log_prob_"], sk.feature_log_prob_)
                assert np.array_equal(fit["class_log_prior_"], sk.class_log_prior_)
        mono += int(((n1[w] + n2[w])[:, :len(cols)] == 0).sum())
    assert (mono > 0) == (panel == "degenerate")


@pytest.mark.parametrize("kind", KINDS)
def test_converter_from_a_live_estimator_and_from_an_attribute_bag(kind):
    from gnomix_amd.convert import nb_window_from_sklearn, from_reference_model
    g = load_golden("G23_nb.npz")
    C, M, A, ctx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    W = C // M
    live, bags = [], []
    for w in range(W):
        cols = NE.window_columns(C, M, ctx, w)
        sk = sk_estimator(kind).fit(g["Xt"][:, cols], g["yt"][:, w])
        bag = types.SimpleNamespace(**{nm: getattr(sk, nm) for nm in ATTRS[kind] + ("classes_",)})
        t1, b1 = nb_window_from_sklearn(sk, len(cols), A)
        t2, b2 = nb_window_from_sklearn(bag, len(cols), A, kind=kind)
        tr, br = NE.tables(kind, {nm: getattr(sk, nm) for nm in ATTRS[kind] + ("classes_",)}, A)
        assert t1.shape == (len(cols), 4, A) and np.array_equal(t1, t2) and np.array_equal(b1, b2)
        assert np.array_equal(t1, tr) and np.array_equal(b1, br)
        live.append(sk)
        # an attribute bag as a stubbed pickle gives it: the class NAME is what from_reference_model reads
        bags.append(type(type(sk).__name__, (), {})())
        bags[-1].__dict__.update(bag.__dict__)
    for models in (live, bags):
        d = from_reference_model(_reference_model(C, M, A, ctx, models))
        assert d.base_kind == "nb" and d.nb_kind == kind and d.smooth_kind == "crf"
        assert d.nb_table.shape == (W, M + 2 * ctx + C - M * W, 4, A) and d.nb_bias.shape == (W, A)
        for w in range(W):
            width = d.window_width(w)
            t, b = nb_window_from_sklearn(live[w], width, A)
            assert np.array_equal(d.nb_table[w, :width], t) and not d.nb_table[w, width:].any()
            assert np.array_equal(d.nb_bias[w], b)
        d.to_desc()
        arr, keep = d.nb_windows()
        assert [arr[w].width for w in range(W)] == [d.window_width(w) for w in range(W)]


def _reference_model(C, M, A, ctx, models):
    """the attributes the converter reads of an unpickled reference model, with the reference's CRF smoother (src/Smooth/models.py:27-32)"""
    class CRF_Smoother:
        S = 1
        calibrator = None
        model = types.SimpleNamespace(CRF=types.SimpleNamespace(state_features_={(str(a), str(a)): 1.5 for a in range(A)},
                                                                transition_features_={("0", "1"): -0.25}))

    return types.SimpleNamespace(C=C, M=M, A=A, context=ctx, smooth=CRF_Smoother(), base=types.SimpleNamespace(models=models),
                                 snp_pos=np.arange(C), snp_ref=np.array(["A"] * C), snp_alt=np.array(["G"] * C),
                                 population_order=["p%d" % a for a in range(A)], gen_map_df=None)


@pytest.mark.parametrize("kind", ("bernoulli", "multinomial"))
def test_from_reference_model_names_the_window_of_a_non_finite_feature_log_prob(kind):
    from gnomix_amd.convert import from_reference_model
    g = load_golden("G23_nb.npz")
    C, M, A, ctx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    models = []
    for w in range(C // M):
        cols = NE.window_columns(C, M, ctx, w)
        models.append(sk_estimator(kind).fit(g["Xt"][:, cols], g["yt"][:, w]))
    from_reference_model(_reference_model(C, M, A, ctx, models))          # converts as fitted
    models[7].feature_log_prob_[2, 3] = -np.inf                           # what alpha=0 leaves on a class-monomorphic SNP
    with pytest.raises(ValueError, match=r"^window 7: .*alpha=0 under scikit-learn >= 1.4.*NaN"):
        from_reference_model(_reference_model(C, M, A, ctx, models))
    # a window that lacks a class converts, with the class absent in that window alone
    cols = NE.window_columns(C, M, ctx, 4)
    keep = g["yt"][:, 4] != 1
    models[7] = sk_estimator(kind).fit(g["Xt"][:, NE.window_columns(C, M, ctx, 7)], g["yt"][:, 7])
    models[4] = sk_estimator(kind).fit(g["Xt"][keep][:, cols], g["yt"][keep, 4])
    d = from_reference_model(_reference_model(C, M, A, ctx, models))
    assert np.isneginf(d.nb_bias[4, 1]) and np.isfinite(np.delete(d.nb_bias, 4 * A + 1)).all() and not d.nb_table[4, :, :, 1].any()


def test_a_window_that_lacks_a_class_gets_minus_infinity_and_zero_rows():
    from gnomix_amd.convert import nb_window_from_sklearn
    rng = np.random.RandomState(1)
    X = rng.randint(0, 3, (40, 9)).astype(np.int8)
    y = rng.choice([0, 2, 3], 40)
    for kind in KINDS:
        t, b = nb_window_from_sklearn(sk_estimator(kind).fit(X, y), 9, 5)
        assert np.isneginf(b[[1, 4]]).all() and np.isfinite(b[[0, 2, 3]]).all()
        assert not t[:, :, [1, 4]].any() and np.isfinite(t).all()
        B, J = NE.predict(X[:, :9], [(t, b)], 9, 8, 0, 5)      # C = 9, M = 8: one window of width 9
        assert not B[:, 0, [1, 4]].any() and np.allclose(B.sum(-1), 1, atol=1e-15)
        assert np.abs(B[:, 0, [0, 2, 3]] - sk_estimator(kind).fit(X, y).predict_proba(X)).max() <= 1e-12


def test_refusals_of_the_converter():
    from sklearn.naive_bayes import BernoulliNB, MultinomialNB
    from gnomix_amd.convert import nb_window_from_sklearn, nb_tables
    rng = np.random.RandomState(2)
    X = rng.randint(0, 3, (30, 6)).astype(np.int8)
    y = np.arange(30) % 3
    X[y == 1, 2] = 0                 # class-monomorphic at 0: log 0 under alpha = 0
    X[y == 2, 4] = 1                 # non-zero in every row of a class: log(1 - exp(0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for est in (BernoulliNB(alpha=0, force_alpha=True), MultinomialNB(alpha=0, force_alpha=True)):
            with pytest.raises(ValueError, match=r"alpha=0 under scikit-learn >= 1.4.*NaN"):
                nb_window_from_sklearn(est.fit(X, y), 6, 3)
    ok = BernoulliNB(alpha=1e-10).fit(X, y)
    flp = ok.feature_log_prob_.copy()
    flp[2, 4] = 0.0
    with pytest.raises(ValueError, match="NaN"):
        nb_tables("bernoulli", dict(classes_=ok.classes_, feature_log_prob_=flp, class_log_prior_=ok.class_log_prior_), 3)
    with pytest.raises(ValueError, match="binarize"):
        nb_window_from_sklearn(BernoulliNB(alpha=1e-10, binarize=0.5).fit(X, y), 6, 3)
    with pytest.raises(ValueError, match="binarize"):
        nb_window_from_sklearn(BernoulliNB(alpha=1e-10, binarize=None).fit(X, y), 6, 3)
    with pytest.raises(ValueError, match="wide"):
        nb_window_from_sklearn(ok, 7, 3)
    with pytest.raises(ValueError, match="classes_"):
        nb_window_from_sklearn(ok, 6, 2)
    with pytest.raises(NotImplementedError):
        nb_window_from_sklearn(object(), 6, 3)
    with pytest.raises(ValueError, match="kind"):
        nb_tables("complement", {"classes_": [0]}, 3)


def test_gnx_round_trip_untrained_model_and_the_description(tmp_path):
    from gnomix_amd import _lib
    from gnomix_amd.model import GnxModelData
    from gnomix_amd.train import untrained_model
    C, M, A, ctx = 53, 20, 3, 4
    for kind in KINDS:
        d = untrained_model(C, M, A, 1, ctx, "default", base="nb_" + kind)
        assert d.base_kind == "nb" and d.nb_kind == kind and d.smooth_kind == "xgb"
        assert d.nb_table.shape == (2, 20 + 8 + 13, 4, A) and d.nb_bias.shape == (2, A) and not d.nb_table.any() and not d.nb_bias.any()
    with pytest.raises(ValueError, match="knn"):
        untrained_model(C, M, A, 1, ctx, "default", base="lda")
    with pytest.raises(ValueError, match="nb_bernoulli"):
        untrained_model(C, M, A, 1, ctx, "default", base="nb")
    rng = np.random.RandomState(3)
    d.nb_table, d.nb_bias = rng.normal(size=d.nb_table.shape), rng.normal(size=d.nb_bias.shape)
    d.nb_bias[1, 2] = -np.inf
    path = str(tmp_path / "nb.gnx")
    d.save(path)
    again = GnxModelData.load(path)
    assert again.base_kind == "nb" and again.nb_kind == "gaussian" and isinstance(again.nb_kind, str)
    assert np.array_equal(again.nb_table, d.nb_table) and np.array_equal(again.nb_bias, d.nb_bias)
    desc, keep = again.to_desc()
    assert desc.abi_version == _lib.GNX_ABI_VERSION == 16 and desc.base_kind == _lib.BASE_NB == 6
    arr, keep2 = again.nb_windows()
    assert [arr[w].width for w in range(2)] == [28, 41] and arr[0].reserved == 0
    for w in range(2):
        got = np.ctypeslib.as_array(ctypes.cast(arr[w].table, ctypes.POINTER(ctypes.c_double)), (arr[w].width, 4, A))
        assert np.array_equal(got, d.nb_table[w, :arr[w].width])
        assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(arr[w].bias, ctypes.POINTER(ctypes.c_double)), (A,)), d.nb_bias[w])
    for field in ("nb_table", "nb_bias"):
        bad = GnxModelData.load(path)
        setattr(bad, field, None)
        with pytest.raises(ValueError, match="nb_table"):
            bad.to_desc()
    bad = GnxModelData.load(path)
    bad.nb_table = bad.nb_table[:, :-1]
    with pytest.raises(ValueError):
        bad.nb_windows()


def test_train_nb_base_refuses_bad_inputs_before_touching_the_device():
    from gnomix_amd.train import train_nb_base, untrained_model
    C, M, A, ctx = 53, 20, 3, 4
    rng = np.random.RandomState(0)
    X, y = rng.randint(0, 3, (31, C)).astype(np.int8), rng.randint(0, A, (31, 2))
    for bad_X, bad_y in ((X[:, :-1], y), (np.where(X == 2, 3, X), y), (-X, y), (X + 0.5, y), (X, y[:-1]), (X, y + 1), (X, y - 1), (X[:0], y[:0])):
        with pytest.raises(ValueError):
            train_nb_base(untrained_model(C, M, A, 1, ctx, "default", base="nb_gaussian"), bad_X, bad_y, "gaussian")
    with pytest.raises(ValueError, match="kind"):
        train_nb_base(untrained_model(C, M, A, 1, ctx, "default", base="nb_gaussian"), X, y, "complement")


def test_header_and_binding_agree_on_gnx_nb_window(tmp_path):
    from gnomix_amd import _lib
    h = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    assert re.search(r"#define GNX_ABI_VERSION 16\b", h) and re.search(r"GNX_BASE_NB = 6\b", h)
    body = re.search(r"typedef struct gnx_nb_window \{(.*?)\} gnx_nb_window;", h, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.NbWindow._fields_]
    assert "gnx_model_load_nb" in _lib.SYMBOLS and "gnx_train_nb_counts" in _lib.SYMBOLS and "gnx_train_nb_counts_dev" in _lib.SYMBOLS
    assert not re.search(r"GNX_K_\w*NB", h) and re.search(r"GNX_K_COUNT = 9\b", h)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gnomix_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(gnx_nb_window), offsetof(gnx_nb_window, table), offsetof(gnx_nb_window, bias),\n'
                   '         offsetof(gnx_nb_window, width), offsetof(gnx_nb_window, reserved));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    N = _lib.NbWindow
    assert got == [ctypes.sizeof(N), N.table.offset, N.bias.offset, N.width.offset, N.reserved.offset] == [24, 0, 8, 16, 20]
