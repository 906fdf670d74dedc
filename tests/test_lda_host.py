"""The LDA base without a GPU: tests/lda_exact.py — int64 integers through gnomix_amd.train.lda_finish, the restatement the GPU tests
lean on — against a live scikit-learn fit and against the reference's own LDABase (tests/golden/G25_lda_base.npz); the converter, its
refusals, the .gnx round trip, the header and untrained_model.

DECISION_TOL: the largest |decision_function difference| between the restatement and LinearDiscriminantAnalysis().fit over every
case below was measured at 1.6e-12 (the sixth shape with A = 2, window 4; the N < width case gave 1.1e-12); the assertion stands at
100 x that, which covers other LAPACK builds, and never above 1e-9: more than that is a wrong std or rank, not rounding."""
import io
import os
import pickle
import re
import types
import warnings

import numpy as np
import pytest

from conftest import load_golden
import lda_exact as LE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = 1.6e-12
DECISION_TOL = min(100 * MEASURED, 1e-9)
TOL = 1e-4
CASES = ["table%d" % i for i in range(len(LE.TABLE))] + ["sixth"]


def _panel(case):
    return LE.table_panel(int(case[5:])) if case.startswith("table") else LE.sixth_panel(3)


def _sk(Xw, yw):
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LinearDiscriminantAnalysis().fit(Xw.astype(np.float64), yw)


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_a_live_scikit_learn_fit(case):
    (C, M, cx, A), X, y, Xq = _panel(case)
    assert len(Xq) == 64
    coef, icpt, infos = LE.fit(X, y, C, M, cx, A, TOL)
    D = LE.decision(Xq, coef, icpt, C, M, cx)
    P = LE.proba(D, A)
    worst = 0.0
    for w in range(C // M):
        cols = LE.window_columns(C, M, cx, w)
        sk = _sk(X[:, cols], y[:, w])
        rank, rank2, sv, sv2 = LE.sklearn_svd_steps(X[:, cols], y[:, w], TOL)
        info = infos[w]
        # no singular value of either decomposition, on either route, within a factor 100 of its threshold: a rank never hangs on rounding
        for s, thr in ((sv, TOL), (info["sv"], TOL), (sv2, TOL * sv2[0]), (info["sv2"], TOL * info["sv2"][0])):
            assert not np.any((s > thr / 100) & (s < thr * 100)), (w, s, thr)
        assert (info["rank"], info["rank2"]) == (rank, rank2), (w, info["rank"], info["rank2"], rank, rank2)
        Xw = Xq[:, cols].astype(np.float64)
        err = np.abs(D[:, w] - sk.decision_function(Xw).reshape(len(Xq), -1)).max()
        worst = max(worst, err)
        assert np.array_equal(P[:, w].argmax(-1), sk.predict_proba(Xw).argmax(-1)), w
    print(case, "max |decision - scikit-learn| = %.3e (bar %.1e)" % (worst, DECISION_TOL))
    assert worst <= DECISION_TOL
    if case == "sixth":
        assert C // M == 8 and {len(LE.window_columns(C, M, cx, w)) for w in range(8)} == {48, 59}
        assert infos[0]["rank"] < 48 - 12 and infos[3]["rank"] == 46       # window 0: reflected, duplicated, constant; window 3: two
    if case == "table3":
        assert X.shape[0] < X.shape[1]


def _golden(A):
    g = load_golden("G25_lda_base.npz")
    pre = "A%d_" % A
    C, M, cx = int(g[pre + "C"]), int(g[pre + "M"]), int(g[pre + "ctx"])
    return g, pre, C, M, cx


@pytest.mark.parametrize("A", (3, 2))
def test_restatement_and_converter_equal_the_references_base_G25(A):
    from gnomix_amd.convert import lda_from_sklearn
    g, pre, C, M, cx = _golden(A)
    (C2, M2, cx2, _), X, y, Xq = LE.sixth_panel(A)
    assert (C, M, cx) == (C2, M2, cx2) and np.array_equal(X, g[pre + "X"]) and np.array_equal(y, g[pre + "y"]) and np.array_equal(Xq, g[pre + "Xq"])
    ref = g[pre + "B"]
    coef, icpt, _ = LE.fit(X, y, C, M, cx, A, TOL)
    B = LE.predict(Xq, coef, icpt, C, M, cx, A)
    err = np.abs(B - ref).max()
    print("A =", A, "max |restatement - reference| = %.3e" % err)
    assert B.shape == ref.shape == (64, 8, A) and err <= DECISION_TOL
    assert np.array_equal(B.argmax(-1), ref.argmax(-1))
    # the stored coef_ / intercept_ through the converter, evaluated in numpy
    W, R = C // M, (1 if A == 2 else A)
    c2, b2 = np.zeros_like(coef), np.zeros_like(icpt)
    for w in range(W):
        bag = types.SimpleNamespace(coef_=g["%sw%d_coef_" % (pre, w)], intercept_=g["%sw%d_intercept_" % (pre, w)], classes_=np.arange(A))
        cw, bw = lda_from_sklearn(bag, len(LE.window_columns(C, M, cx, w)), A)
        assert cw.shape[0] == R
        c2[w, :, :cw.shape[1]], b2[w] = cw, bw
    err2 = np.abs(LE.predict(Xq, c2, b2, C, M, cx, A) - ref).max()
    print("A =", A, "max |converted coefficients in numpy - reference| = %.3e" % err2)
    assert err2 <= 1e-12


def _reference_model(C, M, A, cx, models):
    class CRF_Smoother:
        S = 1
        calibrator = None
        model = types.SimpleNamespace(CRF=types.SimpleNamespace(state_features_={(str(a), str(a)): 1.5 for a in range(A)},
                                                                transition_features_={("0", "1"): -0.25}))

    return types.SimpleNamespace(C=C, M=M, A=A, context=cx, smooth=CRF_Smoother(), base=types.SimpleNamespace(models=models),
                                 snp_pos=np.arange(C), snp_ref=np.array(["A"] * C), snp_alt=np.array(["G"] * C),
                                 population_order=["p%d" % a for a in range(A)], gen_map_df=None)


@pytest.mark.parametrize("A", (3, 2))
def test_from_reference_model_live_estimators_and_stubbed_pickles(A):
    from gnomix_amd.convert import from_reference_model
    from gnomix_amd.refpickle import load_reference_pickle
    (C, M, cx, _), X, y, Xq = LE.sixth_panel(A)
    W = C // M
    live = [_sk(X[:, LE.window_columns(C, M, cx, w)], y[:, w]) for w in range(W)]
    # the attribute-bag reader: scikit-learn's own pickle of the estimator, read back without scikit-learn's classes
    bags = [load_reference_pickle(io.BytesIO(pickle.dumps(m)), use_sklearn=False) for m in live]
    assert type(bags[0]).__name__ == "LinearDiscriminantAnalysis" and type(bags[0]) is not type(live[0])
    ds = [from_reference_model(_reference_model(C, M, A, cx, models)) for models in (live, bags)]
    for d in ds:
        assert d.base_kind == "lda" and d.lda_coef.shape == (W, 1 if A == 2 else A, 59) and d.lda_intercept.shape == (W, 1 if A == 2 else A)
        for w in range(W):
            width = d.window_width(w)
            assert np.array_equal(d.lda_coef[w, :, :width], live[w].coef_) and not d.lda_coef[w, :, width:].any()
            assert np.array_equal(d.lda_intercept[w], live[w].intercept_)
        d.to_desc()
        arr, keep = d.lda_windows()
        assert [(arr[w].width, arr[w].n_rows) for w in range(W)] == [(d.window_width(w), 1 if A == 2 else A) for w in range(W)]
    B = LE.predict(Xq, ds[1].lda_coef, ds[1].lda_intercept, C, M, cx, A)
    for w in range(W):
        assert np.abs(B[:, w] - live[w].predict_proba(Xq[:, LE.window_columns(C, M, cx, w)].astype(np.float64))).max() <= 1e-12


def test_refusals_of_the_converter_and_of_the_fit():
    from gnomix_amd.convert import lda_from_sklearn, from_reference_model
    from gnomix_amd.train import lda_finish
    ok = dict(coef_=np.ones((3, 5)), intercept_=np.zeros(3), classes_=np.arange(3))
    lda_from_sklearn(types.SimpleNamespace(**ok), 5, 3)
    for change, word in ((dict(solver="eigen"), "solver"), (dict(solver="lsqr"), "solver"), (dict(shrinkage="auto"), "shrinkage"),
                         (dict(shrinkage=0.1), "shrinkage"), (dict(classes_=np.array([0, 1, 3])), "classes_"),
                         (dict(classes_=np.array([0, 1])), "classes_"), (dict(coef_=np.ones((3, 4))), "wide"),
                         (dict(coef_=np.full((3, 5), np.nan)), "finite"), (dict(intercept_=np.array([0, np.inf, 0])), "finite"),
                         (dict(coef_=np.ones((1, 5))), "coef_")):
        with pytest.raises(ValueError, match=word):
            lda_from_sklearn(types.SimpleNamespace(**dict(ok, **change)), 5, 3)
    bad = type("LinearDiscriminantAnalysis", (), {})()
    bad.__dict__.update(dict(ok, coef_=np.ones((3, 4)), solver="eigen"))
    with pytest.raises(ValueError, match="window 0"):
        from_reference_model(_reference_model(8, 4, 3, 0, [bad, bad]))
    # the fit: a class without rows, and fewer rows than the pooled covariance needs
    (C, M, cx, A), X, y, _ = LE.table_panel(0)
    G, S, n = LE.numpy_gram(X, np.where(y == 2, 1, y), C, M, cx, A)
    with pytest.raises(ValueError, match="class 2 has no row"):
        lda_finish(G[0], S[0], n[0], len(X))
    G, S, n = LE.numpy_gram(X[:3], np.arange(3, dtype=np.int32)[:, None], C, M, cx, A)
    with pytest.raises(ValueError, match="N - A"):
        lda_finish(G[0], S[0], n[0], 3)


def test_train_lda_base_refuses_bad_inputs_before_touching_the_device():
    from gnomix_amd.train import train_lda_base, untrained_model
    C, M, A, cx = 53, 20, 3, 4
    d = untrained_model(C, M, A, 1, cx, "default", base="lda_svd")
    X, y = np.zeros((6, C), np.int8), np.zeros((6, 2), np.int32)
    for Xb, yb, word in ((X[:, :-1], y, "X must be"), (X + 3, y, "codes"), (X.astype(np.float64) + 0.5, y, "whole"), (X, y[:, :1], "y must be"),
                         (X, y + 3, "labels"), (X[:3], y[:3], "N - A")):
        with pytest.raises(ValueError, match=word):
            train_lda_base(d, Xb, yb)


def test_untrained_model_is_uniform_and_the_gnx_round_trip_keeps_the_model(tmp_path):
    from gnomix_amd import _lib
    from gnomix_amd.model import GnxModelData
    from gnomix_amd.train import untrained_model
    for A in (2, 5):
        d = untrained_model(203, 24, A, 5, 12, "default", base="lda_svd", seed=1)
        R = 1 if A == 2 else A
        assert d.base_kind == "lda" and d.smooth_kind == "xgb" and d.lda_coef.shape == (8, R, 59) and d.lda_intercept.shape == (8, R)
        Xq = np.random.RandomState(A).randint(0, 3, (9, 203)).astype(np.int8)
        assert np.array_equal(LE.predict(Xq, d.lda_coef, d.lda_intercept, 203, 24, 12, A), np.full((9, 8, A), 1.0 / A))
        desc, keep = d.to_desc()
        assert desc.base_kind == _lib.BASE_LDA == 7
    for name in ("qda", "lda"):      # the accepted-names message lists the new name; the bare "lda" stays refused (older tests pin it)
        with pytest.raises(ValueError, match="lda_svd"):
            untrained_model(203, 24, 3, 5, 12, "default", base=name)
    (C, M, cx, A), X, y, Xq = LE.sixth_panel(3)
    d = untrained_model(C, M, A, 5, cx, "fast", base="lda_svd")
    d.lda_coef, d.lda_intercept, _ = LE.fit(X, y, C, M, cx, A)
    path = str(tmp_path / "lda.gnx")
    d.save(path)
    e = GnxModelData.load(path)
    assert e.base_kind == "lda" and e.smooth_kind == "crf" and (e.C, e.M, e.A, e.context) == (C, M, A, cx)
    assert np.array_equal(e.lda_coef, d.lda_coef) and np.array_equal(e.lda_intercept, d.lda_intercept) and e.lda_coef.dtype == np.float64
    bad = untrained_model(C, M, A, 5, cx, "default", base="lda_svd")
    bad.lda_coef = bad.lda_coef[:, :, :-1]
    with pytest.raises(ValueError, match="lda_coef"):
        bad.lda_windows()


def test_header_and_binding_agree(tmp_path):
    import ctypes
    import subprocess
    from gnomix_amd import _lib
    h = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    assert re.search(r"GNX_BASE_LDA = 7\b", h) and "#define GNX_ABI_VERSION 16\n" in h and _lib.GNX_ABI_VERSION == 16 and _lib.BASE_LDA == 7
    for name in ("gnx_model_load_lda", "gnx_train_lda_gram", "gnx_train_lda_gram_dev"):
        assert name in _lib.SYMBOLS and re.search(r"\bint %s\(" % name, h)
    assert not re.search(r"GNX_K_\w*LDA", h) and re.search(r"GNX_K_COUNT = 9\b", h)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gnomix_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(gnx_lda_window), offsetof(gnx_lda_window, coef), offsetof(gnx_lda_window, intercept), '
                   'offsetof(gnx_lda_window, width), offsetof(gnx_lda_window, n_rows)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    L = _lib.LdaWindow
    assert got == [ctypes.sizeof(L), L.coef.offset, L.intercept.offset, L.width.offset, L.n_rows.offset]
    src = open(os.path.join(ROOT, "gnomix_amd", "csrc", "gnx_api.hip")).read()
    assert re.search(r"case GNX_BASE_LDA: rc = fail\(ctx, GNX_EINVAL, \"[^\"]*gnx_model_load_lda", src)
