"""Plain-numpy restatement of the many-trait form of the ancestry-specific association model (gnx_ancestry_assoc_traits of
include/gnomix_hip.h, gnomix_amd.assoc.finish_traits).  Not a test.

THE CONTRACT.  Everything is assoc_exact.py's (X, labels, win(c), h, d, Z, use, min_ac, the model, the column rule, status 1 and 2, n,
df, n_alt, n_hap, n_miss) with Y (N / 2, T) in place of y, T >= 1, and ONE change: individual i takes part at window k when use[i] != 0,
Z[i, :] is finite, EVERY entry of Y[i, :] is finite and both labels at k lie in [0, A): complete cases across the batch of traits.  For
T = 1 that is assoc_exact.participation.  The integer quantities, the column rule and the status do not depend on the trait.  Only
these blocks do, for the SNPs [c0, c1) and the windows win(c0) .. win(c1 - 1), sums over the participants of the window:
    snp_y  (c1 - c0, A, T)          sum_i d[i, a] Y[i, t]
    win_y  (nw, K + A - 1, T)       sum_i u[i, p] Y[i, t],  u = [Z, h_0 .. h_{A-2}]
    win_yy (nw, T)                  sum_i Y[i, t]^2
Labels outside [0, A) are only compared: the individual is left out at that window, and they are counted among ALL rows.

fit() is assoc_exact.fit per trait (numpy.linalg.lstsq on the full kept design) under that participation.  blocks() sums with
math.fsum.  worst_excess() measures a device result against the exact rational sums, for the bound that holds for ANY summation order."""
import math
from fractions import Fraction

import numpy as np

import allele_counts_exact as AE
import assoc_exact as XE


def base_participation(Y, Z, use):
    """(N / 2,) bool: what use, Z and Y say"""
    Y, Z = np.asarray(Y, np.float64), np.asarray(Z, np.float64)
    base = np.isfinite(Y).all(1) & np.isfinite(Z).all(1)
    if use is not None:
        base &= np.asarray(use) != 0
    return base


def participation(labels, A, Y, Z, use):
    """-> (N / 2, W) bool"""
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 0) & (lab < A)
    return base_participation(Y, Z, use)[:, None] & ok[0::2] & ok[1::2]


def fit(X, labels, M, A, Y, Z, use=None, min_ac=1, cols=None):
    """-> list over the traits of assoc_exact.fit's dict, each under the complete-case participation of the whole batch"""
    Y = np.asarray(Y, np.float64)
    use2 = base_participation(Y, Z, use).astype(np.uint8)
    return [XE.fit(X, labels, M, A, np.where(use2 != 0, Y[:, t], 0.0), Z, use2, min_ac=min_ac, cols=cols) for t in range(Y.shape[1])]


def terms(X, labels, M, A, Y, Z, use, c0, c1):
    """the terms of every sum, non-participants as zeros: dterm (nc, A, n_ind) int64 = d[i, c, a] at the participants of win(c); u
    (nw, K + A - 1, n_ind) float64 = [Z, h_0 .. h_{A-2}] at the participants of the window; Yc (n_ind, T) = Y with the rows that never
    take part zeroed; pw (nw, n_ind) bool: who takes part at the window; n_bad; the row of the window blocks of every SNP"""
    X = np.asarray(X)
    Y, Z = np.asarray(Y, np.float64), np.asarray(Z, np.float64)
    lab = np.asarray(labels).astype(np.int64)
    C, W = X.shape[1], lab.shape[1]
    K = Z.shape[1]
    win = AE.windows(C, M, W)
    partw = participation(labels, A, Y, Z, use)
    base = base_participation(Y, Z, use)
    Yc = np.where(base[:, None], Y, 0.0)
    Zc = np.where(base[:, None], Z, 0.0)
    d, _ = XE.dosages(X, labels, M, A)
    w0, w1 = int(win[c0]), int(win[c1 - 1])
    dterm = (d[:, c0:c1] * partw[:, win[c0:c1], None]).transpose(1, 2, 0)
    u = np.zeros((w1 - w0 + 1, K + A - 1, len(Yc)))
    for w in range(w0, w1 + 1):
        r = partw[:, w]
        u[w - w0, :K] = (Zc * r[:, None]).T
        for a in range(A - 1):
            u[w - w0, K + a] = ((lab[0::2, w] == a).astype(np.float64) + (lab[1::2, w] == a)) * r
    n_bad = int(((lab[:, w0:w1 + 1] < 0) | (lab[:, w0:w1 + 1] >= A)).sum())
    return dterm, u, Yc, partw[:, w0:w1 + 1].T.copy(), n_bad, win[c0:c1] - w0


def blocks(X, labels, M, A, Y, Z, use, c0, c1):
    """snp_y, win_y, win_yy of [c0, c1) by math.fsum (d * y is exact; u * y and y * y are rounded once before the sum), and n_bad"""
    dterm, u, Yc, pw, n_bad, _ = terms(X, labels, M, A, Y, Z, use, c0, c1)
    T = Yc.shape[1]
    snp_y = np.zeros(dterm.shape[:2] + (T,))
    win_y = np.zeros(u.shape[:2] + (T,))
    win_yy = np.zeros((u.shape[0], T))
    for t in range(T):
        y = Yc[:, t]
        for c in range(dterm.shape[0]):
            for a in range(A):
                snp_y[c, a, t] = math.fsum(dterm[c, a].astype(np.float64) * y)
        for w in range(u.shape[0]):
            for p in range(u.shape[1]):
                win_y[w, p, t] = math.fsum(u[w, p] * y)
            win_yy[w, t] = math.fsum((y * y)[pw[w]])
    return snp_y, win_y, win_yy, n_bad


def worst_excess(got, X, labels, M, A, Y, Z, use, c0, c1):
    """got = (snp_y, win_y, win_yy) of the device -> the largest |got - exact| / (gamma_n sum_i |term_i|) over the entries with a
    non-zero term (exact rational arithmetic: no rounding in the reference), n = the participants of the entry's window and
    gamma_n = n 2^-53 / (1 - n 2^-53); and whether every entry whose terms are all zero is exactly 0.0"""
    dterm, u, Yc, pw, _, wof = terms(X, labels, M, A, Y, Z, use, c0, c1)
    n_part = pw.sum(1)
    n_ind, T = Yc.shape
    fy = [[Fraction(float(v)) for v in Yc[:, t]] for t in range(T)]
    eps = Fraction(1, 2 ** 53)
    worst, zeros_ok = Fraction(0), True

    def one(g, tl, n):
        nonlocal worst, zeros_ok
        s_abs = sum(abs(v) for v in tl)
        if s_abs == 0:
            zeros_ok = zeros_ok and (g == 0.0)
            return
        if not np.isfinite(g):
            worst = Fraction(10 ** 9)
            return
        gam = n * eps / (1 - n * eps)
        worst = max(worst, abs(Fraction(float(g)) - sum(tl)) / (gam * s_abs))

    snp_y, win_y, win_yy = got
    for t in range(T):
        for c in range(dterm.shape[0]):
            for a in range(A):
                idx = np.flatnonzero(dterm[c, a])
                one(snp_y[c, a, t], [int(dterm[c, a, i]) * fy[t][i] for i in idx], int(n_part[wof[c]]))
        for w in range(u.shape[0]):
            for p in range(u.shape[1]):
                idx = np.flatnonzero(u[w, p])
                one(win_y[w, p, t], [Fraction(float(u[w, p, i])) * fy[t][i] for i in idx], int(n_part[w]))
            one(win_yy[w, t], [fy[t][i] * fy[t][i] for i in np.flatnonzero(pw[w])], int(n_part[w]))
    return float(worst), zeros_ok
