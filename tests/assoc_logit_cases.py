"""Inputs the logistic association tests share (tests/test_assoc_logit_host.py on the CPU, tests/test_gpu_assoc_logit.py on the GPU).
Not a test.

logit_case(A): assoc_cases.regression_case's geometry (257 individuals, C = 130, M = 20, W = 6 with the last window wider, K = 3, 2 %
missing calls, ALT frequency uniform in [0.2, 0.8]) with a case / control phenotype
    y ~ Bernoulli(sigmoid(-0.2 + 0.3 z1 - 0.2 z2 + 0.4 (dosage_7 - 1)))
and two individuals with use = 0.

TOLERANCE.  Results are compared as max_j |d theta_j| / se_j.  MEASURED is the largest such distance of the numpy restatement
(tests/assoc_logit_exact.py) from two references that share none of its iteration: scikit-learn's newton-cholesky solver at tol = 1e-12
on the explicit design of every 13th SNP, and the same Newton iteration run on to lambda2 <= 1e-26 with math.fsum sums
(test_assoc_logit_host.py::test_restatement_against_sklearn_and_the_converged_run prints and checks it).  TOL_SE = 8 x MEASURED rounded
up; the factor 8 is the margin for the device's exp and log1p.  It is measured against those references, never against the device."""
import numpy as np

import assoc_logit_exact as LE

N_IND, C, M, W, K = 257, 130, 20, 6, 3
KAPPA_MAX = 1e3              # SNPs whose unit-diagonal Hessian is worse conditioned are left out; they must stay below 5 % of the SNPs
MEASURED = 1.1e-11           # the largest distance measured on the CPU: 1.07e-11 (A = 7, against scikit-learn), rounded up
TOL_SE = 9e-11               # = 8 * MEASURED, rounded up
_cache, _fits = {}, {}


def logit_case(A):
    if A not in _cache:
        rng = np.random.RandomState(200 + A)
        N = 2 * N_IND
        lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
        freq = rng.uniform(0.2, 0.8, size=(A, C))
        win = np.minimum(np.arange(C) // M, W - 1)
        a = lab[:, win]
        X = (rng.uniform(size=(N, C)) < freq[a, np.arange(C)[None, :]]).astype(np.int8)
        X[rng.uniform(size=(N, C)) < 0.02] = 2
        Z = np.concatenate([np.ones((N_IND, 1)), rng.normal(size=(N_IND, K - 1))], 1)
        dos = (X[0::2] == 1).astype(np.float64) + (X[1::2] == 1)
        eta = -0.2 + 0.3 * Z[:, 1] - 0.2 * Z[:, 2] + 0.4 * (dos[:, 7] - 1.0)
        y = (rng.uniform(size=N_IND) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        use = np.ones(N_IND, np.uint8)
        use[[3, 100]] = 0
        _cache[A] = (X, lab, y, Z, use)
    return _cache[A]


def logit_fit(A):
    """the restatement's results of logit_case(A), computed once"""
    if A not in _fits:
        X, lab, y, Z, use = logit_case(A)
        _fits[A] = LE.fit(X, lab, M, A, y, Z, use)
    return _fits[A]


def compared(want):
    """-> the SNPs compared (restatement status 0 and kappa <= KAPPA_MAX), the share left out"""
    ok = (want["status"] == 0) & (want["kappa"] <= KAPPA_MAX)
    return ok, 1.0 - ok.sum() / max(len(ok), 1)


def distance(got_beta, got_se, got_theta, want, rows):
    """largest |got - want| / se_want over beta, se and theta of the SNPs `rows` (bool or indices); NaN patterns must agree"""
    worst = 0.0
    for c in np.flatnonzero(rows) if np.asarray(rows).dtype == bool else rows:
        wb, ws = want["beta"][c], want["se"][c]
        assert np.array_equal(np.isnan(got_beta[c]), np.isnan(wb)) and np.array_equal(np.isnan(got_se[c]), np.isnan(ws)), c
        k = ~np.isnan(wb)
        if k.any():
            worst = max(worst, float(np.max(np.abs(got_beta[c][k] - wb[k]) / ws[k])), float(np.max(np.abs(got_se[c][k] - ws[k]) / ws[k])))
        if got_theta is not None:
            kt = want["kept"][c]
            assert not np.isnan(got_theta[c]).any() and np.all(got_theta[c][~kt] == 0.0), c
            worst = max(worst, float(np.max(np.abs(got_theta[c][kt] - want["theta"][c][kt]) / want["se_theta"][c][kt])))
    return worst
