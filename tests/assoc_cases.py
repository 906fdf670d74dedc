"""Inputs the association tests share (tests/test_assoc_host.py on the CPU, tests/test_gpu_assoc.py on the GPU).  Not a test.

regression_case(A): real-valued y and Z at N / 2 = 257 individuals, C = 130 SNPs, M = 20, W = 6 (the last window is wider), K = 3.
Every ancestry is drawn with equal probability per (haplotype, window) (1 / A >= 14 % of the haplotypes: the designs stay well
conditioned), the ALT frequency of every (SNP, ancestry) is uniform in [0.2, 0.8], 2 % of the calls are missing.

TOLERANCE of the regression results against numpy.linalg.lstsq on the full design, per SNP:
    |got - want| <= C_TOL * p_kept * kappa^2 * 2^-53 * max_a |beta_want[c, a]|        for beta, se and t alike
kappa = the 2-norm condition number of the column-scaled kept design (the normal equations lose kappa^2).  C_TOL is not fitted to the
device: test_assoc_host.py measures the largest ratio err / (p kappa^2 2^-53 max|beta|) of the HOST FINISH FED THE RESTATEMENT'S BLOCKS
(math.fsum sums) over these inputs (A = 2, 3, 7) and asserts it stays below C_TOL / 8 = 50; the factor 8 is the margin for a different
summation order of the same length on the device.  Measured: MEASURED_RATIO below."""
import numpy as np

import assoc_exact as XE

N_IND, C, M, W, K = 257, 130, 20, 6, 3
KAPPA_MAX = 1e3              # SNPs above it are left out; they must stay below 5 % of the SNPs (asserted on the CPU and on the GPU)
MEASURED_RATIO = 45.7        # test_assoc_host.py::test_finish_against_lstsq_and_the_constant on the CPU: 45.7 (A = 2), 4.46 (A = 3), 0.41
#                              (A = 7); the largest is t's error (|t| is about ten times |beta| here and the bound is relative to |beta|)
C_TOL = 400.0                # = 8 * 50: MEASURED_RATIO rounded up to 50 (slack for another numpy / LAPACK build), times the margin of 8
_cache = {}


def regression_case(A):
    if A not in _cache:
        rng = np.random.RandomState(100 + A)
        N = 2 * N_IND
        lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
        freq = rng.uniform(0.2, 0.8, size=(A, C))
        win = np.minimum(np.arange(C) // M, W - 1)
        a = lab[:, win]
        X = (rng.uniform(size=(N, C)) < freq[a, np.arange(C)[None, :]]).astype(np.int8)
        X[rng.uniform(size=(N, C)) < 0.02] = 2
        Z = np.concatenate([np.ones((N_IND, 1)), rng.normal(size=(N_IND, K - 1))], 1)
        dos = (X[0::2] == 1).astype(np.float64) + (X[1::2] == 1)
        y = 0.5 + Z[:, 1] * 0.3 - Z[:, 2] * 0.2 + 0.4 * dos[:, 7] + rng.normal(size=N_IND)
        use = np.ones(N_IND, np.uint8)
        use[[3, 100]] = 0
        _cache[A] = (X, lab, y, Z, use)
    return _cache[A]


_fits = {}


def regression_fit(A):
    """the restatement's lstsq results of regression_case(A), computed once"""
    if A not in _fits:
        X, lab, y, Z, use = regression_case(A)
        _fits[A] = XE.fit(X, lab, M, A, y, Z, use)
    return _fits[A]


def ratios(got_beta, got_se, got_t, want):
    """-> (largest err / (p kappa^2 2^-53 max|beta|) over the SNPs with status 0 and kappa <= KAPPA_MAX, fraction of SNPs left out).
    NaN patterns must agree exactly."""
    ok = (want["status"] == 0) & (want["kappa"] <= KAPPA_MAX)
    left_out = 1.0 - ok.sum() / len(ok)
    worst = 0.0
    for g, name in ((got_beta, "beta"), (got_se, "se"), (got_t, "t")):
        w = want[name]
        assert np.array_equal(np.isnan(g[ok]), np.isnan(w[ok])), name
        scale = want["p_kept"][ok] * want["kappa"][ok] ** 2 * 2.0 ** -53 * np.nanmax(np.abs(want["beta"][ok]), axis=1)
        err = np.nanmax(np.abs(g[ok] - w[ok]), axis=1)
        worst = max(worst, float(np.max(err / scale)))
    return worst, left_out
