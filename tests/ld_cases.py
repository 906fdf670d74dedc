"""Inputs and the shape grid of the LD tests (tests/test_ld_host.py, tests/test_gpu_ld.py).  Not a test.

The kernel's sizes the grid is chosen by (csrc/summary/k_ancestry_ld.hip): an MFMA tile is 16 SNPs, a SNP tile 64, the MFMA's K is 64
haplotypes, a staging chunk 128 haplotypes, a staged item 4 haplotypes x a group of 16 SNPs; a packed byte holds 4 SNPs."""
import numpy as np

NS = (1, 2, 3, 4, 5, 63, 65, 127, 129, 257)     # haplotypes (odd ones too): partial items of 4, either side of K = 64 and of the chunk, two chunks + 1
CS = (1, 15, 17, 63, 65, 130, 200)              # SNPs: either side of a group of 16 and of a tile; three and four tiles with a ragged edge
MS = (1, 5, 24, None)                           # window sizes (None = C: one window); 5 and 24 put boundaries inside groups of 16
AS = (2, 3, 7)
BANDS = (1, 2, 15, 16, 17, 63, 64, 65, 130)     # and C + 3, a band wider than everything (bands_for)
RANGES = ((3, 197), (17, 131), (65, 66), (70, 130), (0, 200))     # of C = 200: off every multiple of 16 and 64, one SNP, and everything


def bands_for(C):
    return BANDS + (C + 3,)


def geometry(C, M):
    """-> M, W with M <= C and W = C // M (the last window takes C - M W more SNPs)"""
    M = C if M is None else min(M, C)
    return M, C // M


def case(N, C, M, W, A, seed=0, bad=0):
    """-> X (N, C) int8: codes 0 and 1 with an ALT frequency that differs from SNP to SNP (so that n1o != no1), the missing codes 2 and -1
    (3 in packed rows) and other bytes (7, -128: missing as well) in every row, with row 1 (where N > 2) ALL missing; labels (N, W) int32
    in [0, A) that change every other window.  bad > 0: that many labels are set outside [0, A) (to A, -1, 2^31 - 1 in turn)"""
    rng = np.random.RandomState(1000 * seed + N + 7 * C + 31 * A + 3 * M)
    freq = rng.uniform(0.15, 0.85, size=C)
    X = (rng.random_sample((N, C)) < freq[None, :]).astype(np.int8)
    miss = rng.random_sample((N, C)) < 0.15
    X[miss] = rng.choice([2, -1, 7, -128], size=int(miss.sum())).astype(np.int8)
    X[np.arange(N), rng.randint(0, C, size=N)] = 2          # a missing code in every row
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


def linked(N, C, seed=0, block=6, flip=0.08, miss=0.02):
    """haplotypes with LD: the SNPs come in blocks of `block` that copy one founder allele per haplotype and block, each copy flipped
    with probability `flip`; `miss` of the calls are missing -> X (N, C) int8"""
    rng = np.random.RandomState(seed)
    founder = rng.random_sample((N, (C + block - 1) // block)) < 0.5
    X = np.repeat(founder, block, axis=1)[:, :C]
    X = (X ^ (rng.random_sample((N, C)) < flip)).astype(np.int8)
    X[rng.random_sample((N, C)) < miss] = 2
    return X
