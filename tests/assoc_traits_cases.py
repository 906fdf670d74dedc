"""Inputs the many-trait association tests share (tests/test_assoc_traits_host.py on the CPU, tests/test_gpu_assoc_traits.py on the GPU).
Not a test.

small_case(n_ind, T, A, K): C = 37 SNPs, M = 8, W = 4 (an unaligned SNP tail: 37 = 2 * 16 + 5, and a long last window of 13 SNPs), with
    missing calls (bytes 2 and -1);
    use = 0 on individual 1; a NaN in Y on individual 2; +inf and -inf in Y on individual 3 (all otherwise usable);
    a monomorphic SNP (5); a SNP (6) whose only ALT call gives a dosage column below min_ac = MIN_AC = 2;
    window 1: every individual but the first carries a label out of range (A, -1 or 2^20), so n <= 1 and df < 1 there, and the count of
      such labels comes back;
    window 2: nobody carries ancestry A - 1 (status 1 for every trait where df >= 1);
    trait T // 3 spans 1e-8 .. 1e8 in magnitude.
GRID: a thinned cross product of n_ind in {5, 8, 9} (a multiple of 4 and not), T in {1, 15, 16, 17, 33} (one trait tile, a padded one,
a full one, two, three), A in {2, 3, 7, 9} (9 = one more than the 8 ancestries a wave carries at once) and K in {1, 3}: every value of
every axis appears.

regression_traits(A): assoc_cases.regression_case(A) with T = 3 traits: its y, and two more with their own signal; one NaN."""
import numpy as np

import assoc_cases as AC

C, M, W = 37, 8, 4
MIN_AC = 2
WAVE_ANCESTRIES = 8
GRID = [(5, 1, 2, 1), (8, 15, 3, 3), (9, 16, 7, 1), (5, 17, 9, 3), (8, 33, 2, 3), (9, 33, 7, 3), (9, 1, 9, 1), (8, 16, 3, 1), (9, 17, 2, 1),
        (5, 15, 7, 1)]
_cache = {}


def small_case(n_ind, T, A, K):
    """-> X (N, C) int8, labels (N, W) int32 (WITH the labels out of range), Y (n_ind, T), Z (n_ind, K), use (n_ind,) uint8"""
    key = (n_ind, T, A, K)
    if key not in _cache:
        rng = np.random.RandomState(1000 * n_ind + 37 * T + 5 * A + K)
        N = 2 * n_ind
        X = rng.choice([0, 1, 2, -1], size=(N, C), p=[0.45, 0.45, 0.06, 0.04]).astype(np.int8)
        X[:, 5] = 0
        X[:, 6] = 0
        X[0, 6] = 1
        lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
        lab[:, 2] = np.where(lab[:, 2] == A - 1, 0, lab[:, 2])
        for i in range(1, n_ind):
            lab[2 * i + (i & 1), 1] = (A, -1, 1 << 20)[i % 3]
        Y = rng.normal(size=(n_ind, T))
        Y[:, T // 3] = rng.choice([-1.0, 1.0], size=n_ind) * 10.0 ** rng.uniform(-8, 8, size=n_ind)
        Y[2, T // 2] = np.nan
        Y[3, 0] = np.inf
        Y[3, T - 1] = -np.inf
        Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, K - 1))], 1)
        use = np.ones(n_ind, np.uint8)
        use[1] = 0
        _cache[key] = (X, lab, Y, Z, use)
    return _cache[key]


_reg = {}


def regression_traits(A):
    """-> X, labels, Y (257, 3), Z, use of assoc_cases.regression_case(A)"""
    if A not in _reg:
        X, lab, y, Z, use = AC.regression_case(A)
        rng = np.random.RandomState(500 + A)
        dos = (X[0::2] == 1).astype(np.float64) + (X[1::2] == 1)
        Y = np.stack([y, 2.0 - 0.5 * Z[:, 1] + 0.3 * dos[:, 40] + rng.normal(size=len(y)), 1e3 * rng.normal(size=len(y))], 1)
        Y[11, 1] = np.nan
        _reg[A] = (X, lab, Y, Z, use)
    return _reg[A]
