"""The numpy restatement of gnx_ancestry_pair_counts (include/gnomix_hip.h), straight from the definitions.  Not a test.

For ancestry a, individual i = haplotype rows 2 i, 2 i + 1 and SNP c with window win(c) = min(c // M, W - 1):
  o[i, c] = the haplotypes h of i with labels[h, win(c)] == a and X[h, c] in {0, 1}
  d[i, c] = those of them with X[h, c] == 1
and over the SNPs [c0, c1): DD = d d^T, DO = d o^T, OO = o o^T, formed with int64 `@`."""
import numpy as np


def window_of(C, M, W):
    return np.minimum(np.arange(C) // M, W - 1)


def hap_masks(X, lab, M, a):
    """-> (carries a and observed, carries a and ALT), (N, C) booleans.  X int8: 0 REF, 1 ALT, any other byte missing"""
    X, lab = np.asarray(X), np.asarray(lab)
    carry = lab[:, window_of(X.shape[1], M, lab.shape[1])] == a
    return carry & ((X == 0) | (X == 1)), carry & (X == 1)


def d_o(X, lab, M, a):
    """-> d, o (N / 2, C) int64"""
    obs, alt = hap_masks(X, lab, M, a)
    return alt[0::2].astype(np.int64) + alt[1::2], obs[0::2].astype(np.int64) + obs[1::2]


def tables(X, lab, M, A, a, c0=0, c1=None):
    """-> DD, DO, OO (N / 2, N / 2) int64 over the SNPs [c0, c1), and n_bad = the labels outside [0, A) in the windows that meet the
    range (such a label equals no ancestry, so the tables ignore it by construction)"""
    C = np.asarray(X).shape[1]
    c1 = C if c1 is None else c1
    d, o = d_o(X, lab, M, a)
    d, o = d[:, c0:c1], o[:, c0:c1]
    win = window_of(C, M, np.asarray(lab).shape[1])
    k0, k1 = win[c0], win[c1 - 1] + 1
    part = np.asarray(lab)[:, k0:k1]
    return d @ d.T, d @ o.T, o @ o.T, int(((part < 0) | (part >= A)).sum())


def tables_loop(X, lab, M, A, a, c0=0, c1=None):
    """the same by a plain triple loop over (i, j, c) and the four haplotype pairs' definitions (tiny shapes only)"""
    X, lab = np.asarray(X), np.asarray(lab)
    N, C = X.shape
    W = lab.shape[1]
    c1 = C if c1 is None else c1
    n = N // 2
    DD, DO, OO = (np.zeros((n, n), np.int64) for _ in range(3))

    def od(i, c):
        o = d = 0
        for h in (2 * i, 2 * i + 1):
            if lab[h, min(c // M, W - 1)] == a and X[h, c] in (0, 1):
                o += 1
                d += int(X[h, c] == 1)
        return o, d
    for i in range(n):
        for j in range(n):
            for c in range(c0, c1):
                oi, di = od(i, c)
                oj, dj = od(j, c)
                DD[i, j] += di * dj
                DO[i, j] += di * oj
                OO[i, j] += oi * oj
    return DD, DO, OO


def hap_pair_counts(X, lab, M, a, c0=0, c1=None):
    """direct counting over haplotype pairs: for individuals i, j (any, i == j included) and the four (or, for i == j, all four ordered)
    pairs (h of i, g of j): compared = both carry a and both are observed, mismatch = compared and the codes differ -> mism, comp int64"""
    X = np.asarray(X)
    obs, alt = hap_masks(X, lab, M, a)
    c1 = X.shape[1] if c1 is None else c1
    obs, alt = obs[:, c0:c1], alt[:, c0:c1]
    n = X.shape[0] // 2
    mism, comp = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(n):
            for h in (2 * i, 2 * i + 1):
                for g in (2 * j, 2 * j + 1):
                    both = obs[h] & obs[g]
                    comp[i, j] += both.sum()
                    mism[i, j] += (both & (alt[h] != alt[g])).sum()
    return mism, comp
