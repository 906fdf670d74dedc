"""Inputs and the shape grid of the pair-count tests (tests/test_pairs_host.py, tests/test_gpu_pairs.py).  Not a test.

The kernel's sizes the grid is chosen by (csrc/summary/k_ancestry_pairs.hip): an MFMA tile is 16 individuals, a macro-tile 64, the
MFMA's K is 64 SNPs, a staging chunk 128 SNPs, a staged group 16 SNPs; a packed byte holds 4 SNPs."""
import numpy as np

NS = (2, 6, 34, 130, 258)              # haplotypes: one individual; a partial 16-row tile; a partial macro-tile; two tile pairs + one
#                                        ragged (65 individuals); a diagonal plus an off-diagonal block with a ragged edge (129)
CS = (1, 3, 63, 65, 200, 1031)         # SNPs: below, at and across the MFMA's K and the chunk; 1031 and 3, 63, 65: a partial last packed byte
MS = (1, 7, 64, None)                  # window sizes (None = C: one window); 7 and 64 leave a remainder in the last window at most C
AS = (1, 3, 32)


def geometry(C, M):
    """-> M, W with M <= C and W = C // M (the last window takes C - M W more SNPs)"""
    M = C if M is None else min(M, C)
    return M, C // M


def case(N, C, M, W, A, seed=0, bad=0):
    """-> X (N, C) int8: codes 0 and 1, the missing codes 2 and -1 (3 in packed rows) and, where the row form allows, other bytes (7,
    -128: missing as well), with row 1 (where N > 2) ALL missing; labels (N, W) int32 in [0, A) that change every other window.  bad > 0:
    that many labels are set outside [0, A) (to A, -1, 2^31 - 1 in turn)"""
    rng = np.random.RandomState(1000 * seed + N + 7 * C + 31 * A + 3 * M)
    X = rng.choice([0, 1, 2, -1, 7, -128], size=(N, C), p=[0.45, 0.4, 0.05, 0.04, 0.03, 0.03]).astype(np.int8)
    if N > 2:
        X[1, :] = rng.choice([2, -1], size=C)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 2 + 1)), 2, axis=1)[:, :W].astype(np.int32)
    if bad:
        at = rng.choice(N * W, size=min(bad, N * W), replace=False)
        lab.reshape(-1)[at] = np.array([A, -1, 2 ** 31 - 1], np.int64)[np.arange(len(at)) % 3].astype(np.int32)
    return X, np.ascontiguousarray(lab)


def codes(X):
    """int8 bytes -> 2-bit codes: -1 becomes 3, every other missing byte 2"""
    return np.where((X == 0) | (X == 1), X, np.where(X == -1, 3, 2)).astype(np.uint8)


def planted(n_ind, C, seed=0):
    """a cohort of two sub-populations: SNP c has ALT frequency 0.5 + 0.35 s[c] in the first half of the individuals and 0.5 - 0.35 s[c]
    in the second, s[c] = +-1 drawn per SNP; 2 % missing calls -> X (2 n_ind, C) int8, group (n_ind,) in {0, 1}"""
    rng = np.random.RandomState(seed)
    group = (np.arange(n_ind) >= n_ind // 2).astype(np.int64)
    side = rng.choice([-1.0, 1.0], size=C)
    p = 0.5 + 0.35 * side[None, :] * np.where(np.repeat(group, 2) == 0, 1.0, -1.0)[:, None]
    X = (rng.random_sample((2 * n_ind, C)) < p).astype(np.int8)
    X[rng.random_sample(X.shape) < 0.02] = 2
    return X, group
