"""CPU tests (-m "not gpu") of the logistic ancestry-specific association: the numpy restatement (tests/assoc_logit_exact.py) against
scikit-learn and against the same iteration converged with math.fsum sums (which measures the tolerance the GPU tests use), the cap on
the SNPs left out, the p-values, write_assoc_logit's bytes, the phenotype refusal and the ABI symbols."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_logit_cases as LC
import assoc_logit_exact as LE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("A", [2, 3, 7])
def test_restatement_against_sklearn_and_the_converged_run(A):
    """max_j |d theta_j| / se_j of the restatement against scikit-learn's newton-cholesky (tol 1e-12) and against the Newton iteration run
    on to lambda2 <= 1e-26 with math.fsum sums, on the explicit design of every 13th SNP: both within MEASURED, and TOL_SE = 8 MEASURED.
    Measured on this case: against scikit-learn 9.4e-13 (A = 2), 6.5e-13 (A = 3), 1.07e-11 (A = 7); against the converged run 1.5e-14,
    4.1e-14, 1.1e-13 (the restatement takes one more full step once lambda2 <= 1e-10, which leaves it far closer to the optimum than
    scikit-learn's own stopping rule leaves scikit-learn: the first figure is mostly scikit-learn's distance)."""
    from sklearn.linear_model import LogisticRegression
    X, lab, y, Z, use = LC.logit_case(A)
    want = LC.logit_fit(A)
    worst_sk = worst_cv = 0.0
    for c in range(0, LC.C, 13):
        assert want["status"][c] == 0
        part, D, yy = LE.design(X, lab, LC.M, A, y, Z, use, c)
        kept = want["kept"][c]
        Dk = D[:, kept]
        th, se = want["theta"][c][kept], want["se_theta"][c][kept]
        sk = LogisticRegression(penalty=None, fit_intercept=False, solver="newton-cholesky", tol=1e-12, max_iter=200).fit(Dk, yy)
        worst_sk = max(worst_sk, float(np.max(np.abs(sk.coef_[0] - th) / se)))
        th_cv, se_cv = LE.converge(Dk, yy, th)
        worst_cv = max(worst_cv, float(np.max(np.abs(th_cv - th) / se)), float(np.max(np.abs(se_cv - se) / se)))
    print("A = %d: against scikit-learn %.3g, against the converged run %.3g (MEASURED = %.3g, TOL_SE = %.3g)" % (A, worst_sk, worst_cv, LC.MEASURED, LC.TOL_SE))
    assert worst_sk <= LC.MEASURED and worst_cv <= LC.MEASURED
    assert 8 * LC.MEASURED <= LC.TOL_SE <= 8.5 * LC.MEASURED


@pytest.mark.parametrize("A", [2, 3, 7])
def test_few_snps_are_left_out(A):
    want = LC.logit_fit(A)
    ok, left_out = LC.compared(want)
    print("A = %d: %d of %d left out, kappa <= %.4g, at most %d steps" % (A, (~ok).sum(), LC.C, np.nanmax(want["kappa"]), want["iters"].max()))
    assert left_out < 0.05
    assert (want["status0"] == 0).all() and set(np.unique(want["status"])) <= {0, 3}


def test_designed_statuses_of_the_restatement():
    """all cases -> status0 3 and status 4; a window without ancestry A - 1 -> status0 1; one-sided allele -> NaN term, others fitted;
    separation -> status 3; n <= p_kept -> status 2"""
    X, lab, y, Z, use = (v.copy() for v in LC.logit_case(3))
    cols = [0, 25, 45]
    y1 = y.copy()
    lab1 = lab.copy()
    lab1[:, 1][lab1[:, 1] == 2] = 0                      # window 1: nobody carries ancestry 2
    r = LE.fit(X, lab1, LC.M, 3, y1, Z, use, cols=cols)
    assert r["status0"][1] == 1 and r["status"][25] == 4 and r["status"][0] in (0, 3)
    r = LE.fit(X, lab, LC.M, 3, np.ones_like(y), Z, use, cols=cols)
    assert (r["status0"] != 0).all() and (r["status"][cols] == 4).all()
    Zs = np.concatenate([Z, y[:, None]], 1)              # a covariate equal to y
    r = LE.fit(X, lab, LC.M, 3, y, Zs, use, cols=cols)
    assert (r["status0"] == 3).all()
    few = np.zeros_like(use)
    few[:5] = 1                                          # n = 5 against up to 1 + 2 + 3 columns
    r = LE.fit(X, lab, LC.M, 3, y, Z[:, :1], few)
    win = np.minimum(np.arange(LC.C) // LC.M, LC.W - 1)
    short = (r["n"][win] - r["kept"].sum(1) < 1) & (r["status0"][win] == 0)
    assert short.any() and (r["status"][short] == 2).all() and (r["status"][(r["status0"][win] != 0)] == 4).all()
    Xo = X.copy()                                        # ancestry 0's ALT allele at SNP 0 among the cases only
    w0 = lab[:, 0]
    ctrl = np.repeat(y == 0, 2)
    Xo[(w0 == 0) & ctrl, 0] = 0
    r = LE.fit(Xo, lab, LC.M, 3, y, Z, use, cols=[0])
    assert r["status"][0] == 0 and np.isnan(r["beta"][0, 0]) and not np.isnan(r["beta"][0, 1:]).any() and r["theta"][0, LC.K + 2] == 0.0


def test_p_values_against_scipy():
    from scipy import stats
    from gnomix_amd import assoc
    beta, se = np.array([[0.5, -1.2, np.nan]]), np.array([[0.25, 0.4, np.nan]])
    z, p, lrt_p = assoc.logit_p_values(beta, se, np.array([7.5]), np.array([2]))
    assert np.allclose(z[0, :2], [2.0, -3.0]) and np.isnan(z[0, 2]) and np.isnan(p[0, 2])
    assert p[0, 0] == 2 * stats.norm.sf(abs(z[0, 0])) and p[0, 1] == 2 * stats.norm.sf(abs(z[0, 1])) and lrt_p[0] == stats.chi2.sf(7.5, 2)
    assert np.allclose(p[0, :2], [0.04550026389635839, 0.0026997960632601866], rtol=1e-12, atol=0)
    assert np.isnan(assoc.logit_p_values(beta, se, np.array([np.nan]), np.array([0]))[2][0])


def _result(A, n=2):
    from gnomix_amd import assoc
    want = LC.logit_fit(A)
    sl = slice(0, n)
    fit = assoc.LogitFit(want["beta"][sl], want["se"][sl], want["dev"][sl], want["theta"][sl], want["n_alt"][sl], want["n_alt_case"][sl], want["n_miss"][sl],
                         want["iters"][sl], want["status"][sl], want["theta0"][:1], want["dev0"][:1], want["n"][:1], want["n_case"][:1], want["sum_h"][:1],
                         want["iters0"][:1], want["status0"][:1], np.zeros(n, np.int64), 0)
    return assoc.logit_from_fits(lambda c0, c1: fit, n, A, LC.K)


def test_write_assoc_logit_round_trip(tmp_path):
    from gnomix_amd import postprocess as pp
    res = _result(2)
    assert res.lrt_df.tolist() == [2, 2] and np.all(res.lrt > 0) and np.all(res.df == res.n - (LC.K + 1 + 2))
    pp.write_assoc_logit(str(tmp_path / "q"), "22", [101, 202], LC.M, LC.W, res, ["AFR", "EUR"])
    text = (tmp_path / "q.assoc.logistic.tsv").read_text()
    assert text == LE.logit_text("22", [101, 202], LC.M, LC.W, res, ["AFR", "EUR"])
    rows = [ln.split("\t") for ln in text.splitlines()]
    assert len(rows) == 3 and len(rows[0]) == 12 + 7 * 2 and float(rows[1][rows[0].index("AFR.beta")]) == pytest.approx(res.beta[0, 0], rel=1e-5)
    with pytest.raises(ValueError):
        pp.write_assoc_logit(str(tmp_path / "q"), "22", [1], LC.M, LC.W, res, ["AFR", "EUR"])


def test_non_binary_phenotype_is_refused(tmp_path):
    from gnomix_amd import assoc, cli
    with pytest.raises(ValueError, match="sample 's1' has 0.5"):
        assoc.check_binary(np.array([0.0, 0.5, 2.0, np.nan]), np.array([1, 1, 0, 1]), ["s0", "s1", "s2", "s3"])
    assoc.check_binary(np.array([0.0, 1.0, 2.0, np.nan]), np.array([1, 1, 0, 1]))
    args = dict(query_file="q.vcf", chm="22", output_basename=str(tmp_path), phase=True)
    with pytest.raises(ValueError, match="ancestry_assoc_output with phase=True"):
        cli.run_inference(args, None, ancestry_assoc_output=True, phenotype_file="p.tsv", ancestry_assoc_model="logistic")
    with pytest.raises(ValueError, match="ancestry_assoc_model"):
        cli.run_inference(dict(args, phase=False), None, ancestry_assoc_output=True, phenotype_file="p.tsv", ancestry_assoc_model="probit")


def test_symbols_and_limits():
    so = os.path.join(ROOT, "gnomix_amd", "libgnomix_hip.so")
    if os.path.exists(so):
        lib = ctypes.CDLL(so)
        for name in ("gnx_ancestry_assoc_logit", "gnx_ancestry_assoc_logit_dev", "gnx_ancestry_assoc_logit_gt2"):
            assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    assert "GNX_ASSOC_LOGIT_MAX_Q 47" in hdr and "GNX_ASSOC_LOGIT_TOL 1e-10" in hdr and "GNX_ASSOC_LOGIT_MAX_ITER 25" in hdr
    from gnomix_amd import assoc
    assert (assoc.LOGIT_TOL, assoc.LOGIT_MAX_ITER, assoc.LOGIT_MAX_Q) == (1e-10, 25, 47)
    SF, SI, Q, WF, WI = assoc.logit_layout(7, 5)
    assert (SF, SI, Q, WF, WI) == (15, 17, 18, 12, 11) and assoc.logit_snps_per_chunk(7, 5) * ((SF + Q) * 8 + SI * 4) <= assoc.STATS_CHUNK_BYTES
