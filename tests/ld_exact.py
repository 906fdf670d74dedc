"""The numpy restatement of gnx_ancestry_ld_counts (include/gnomix_hip.h) and of gnomix_amd.ld.clump, straight from the definitions.
Not a test.

For ancestry a, haplotype h and SNP c with window win(c) = min(c // M, W - 1):
  o[h, c] = 1 if labels[h, win(c)] == a and X[h, c] in {0, 1}, else 0          d[h, c] = 1 if o[h, c] and X[h, c] == 1, else 0
and for the SNPs c of [c0, c1) and the offsets k < band, c' = c + k < C (0 beyond):
  n11 = sum_h d[h, c] d[h, c']   n1o = sum_h d[h, c] o[h, c']   no1 = sum_h o[h, c] d[h, c']   noo = sum_h o[h, c] o[h, c']"""
import math

import numpy as np


def window_of(C, M, W):
    return np.minimum(np.arange(C) // M, W - 1)


def o_d(X, lab, M, a):
    """-> o, d (N, C) int64.  X int8: 0 REF, 1 ALT, any other byte missing"""
    X, lab = np.asarray(X), np.asarray(lab)
    carry = lab[:, window_of(X.shape[1], M, lab.shape[1])] == a
    return (carry & ((X == 0) | (X == 1))).astype(np.int64), (carry & (X == 1)).astype(np.int64)


def banded(full, c0, c1, band):
    """the (C, C) table of all pairs -> its band (c1 - c0, band): [c - c0, k] = full[c, c + k], 0 where c + k >= C"""
    C = full.shape[0]
    out = np.zeros((c1 - c0, band), np.int64)
    for k in range(min(band, C)):
        n = min(c1, C - k) - c0
        if n > 0:
            out[:n, k] = full[np.arange(c0, c0 + n), np.arange(c0, c0 + n) + k]
    return out


def full_tables(X, lab, M, a):
    """-> the four (C, C) int64 tables of every pair (c, c'), formed with int64 `@`"""
    o, d = o_d(X, lab, M, a)
    return d.T @ d, d.T @ o, o.T @ d, o.T @ o


def n_bad(lab, M, A, C, c0, c1, band):
    """the labels outside [0, A) in the windows the range and its band reach"""
    lab = np.asarray(lab)
    win = window_of(C, M, lab.shape[1])
    part = lab[:, win[c0]:win[min(c1 - 1 + band - 1, C - 1)] + 1]
    return int(((part < 0) | (part >= A)).sum())


def tables(X, lab, M, A, a, c0=0, c1=None, band=1, full=None):
    """-> n11, n1o, no1, noo (c1 - c0, band) int64 and n_bad (such a label equals no ancestry, so the tables ignore it by construction).
    full: full_tables(X, lab, M, a) where the caller has them already"""
    C = np.asarray(X).shape[1]
    c1 = C if c1 is None else c1
    bad = n_bad(lab, M, A, C, c0, c1, band)
    if full is not None:
        return tuple(banded(t, c0, c1, band) for t in full) + (bad,)
    o, d = o_d(X, lab, M, a)
    out = [np.zeros((c1 - c0, band), np.int64) for _ in range(4)]
    for k in range(min(band, C)):              # offset by offset: sums over the haplotypes of the products of two columns
        n = min(c1, C - k) - c0
        if n > 0:
            for t, (u, v) in zip(out, ((d, d), (d, o), (o, d), (o, o))):
                t[:n, k] = (u[:, c0:c0 + n] * v[:, c0 + k:c0 + k + n]).sum(axis=0)
    return tuple(out) + (bad,)


def tables_loop(X, lab, M, A, a, c0, c1, band):
    """the same by a plain loop over (c, k, h) (tiny shapes only)"""
    X, lab = np.asarray(X), np.asarray(lab)
    N, C = X.shape
    W = lab.shape[1]
    out = [np.zeros((c1 - c0, band), np.int64) for _ in range(4)]

    def od(h, c):
        o = int(lab[h, min(c // M, W - 1)] == a and X[h, c] in (0, 1))
        return o, int(o and X[h, c] == 1)
    for c in range(c0, c1):
        for k in range(band):
            if c + k >= C:
                continue
            for h in range(N):
                o1, d1 = od(h, c)
                o2, d2 = od(h, c + k)
                out[0][c - c0, k] += d1 * d2
                out[1][c - c0, k] += d1 * o2
                out[2][c - c0, k] += o1 * d2
                out[3][c - c0, k] += o1 * o2
    return tuple(out)


def r2_literal(n11, n1o, no1, noo):
    """r^2 of one pair from Python ints, NaN where a variance is 0"""
    num, v, v2 = noo * n11 - n1o * no1, n1o * (noo - n1o), no1 * (noo - no1)
    if v == 0 or v2 == 0:
        return math.nan
    r = float(num) / math.sqrt(float(v) * float(v2))
    return r * r


def clump_literal(p, pos, tabs, band, p1=1e-4, p2=1e-2, r2=0.5, kb=250):
    """gnomix_amd.ld.clump's definition as plain loops; tabs = the four (C, band) tables of the whole range (row c, offset k)"""
    C = len(p)
    index_of = [-1] * C
    cand = [c for c in range(C) if math.isfinite(p[c]) and p[c] <= p1]
    cand.sort(key=lambda c: (p[c], c))
    for c in cand:
        if index_of[c] != -1:
            continue
        index_of[c] = c
        for e in range(C):
            if index_of[e] != -1 or abs(int(pos[e]) - int(pos[c])) > kb * 1000 or not (math.isfinite(p[e]) and p[e] <= p2):
                continue
            lo, k = min(c, e), abs(e - c)
            assert k < band, "the tables do not reach a SNP within kb"
            v = r2_literal(*(int(t[lo, k]) for t in tabs))
            if v >= r2:            # (False for NaN)
                index_of[e] = c
    return np.array(index_of, np.int64)
