"""Plain-numpy float64 restatement of gnx_ancestry_score (include/gnomix_hip.h; csrc/summary/k_ancestry_score.hip).  Not a test.

X (N, C) int8: 0 = REF, 1 = ALT, any other byte = a missing call.  labels (N, W) int32; win(c) = min(c // M, W - 1).  weights (C, A, S)
float64; effect (C,) uint8: 1 = the effect allele is ALT, 0 = REF, 255 = the SNP is not scored.  Individual i is rows 2 i, 2 i + 1.

THE ORDER of every float64 sum (one rounding per add, no fused multiply-add, terms that do not apply are skipped):
  1. per haplotype h and window k with a = labels[h, k] in [0, A): a partial p[h, k, s] starts at +0.0 and adds weights[c, a, s] over the
     SNPs c of window k with effect[c] != 255 and X[h, c] == effect[c], in ASCENDING c;
  2. per (i, a, s): score starts at +0.0 and adds, in ASCENDING k, first p[2 i, k, s] if labels[2 i, k] == a, then p[2 i + 1, k, s] if
     labels[2 i + 1, k] == a  (a partial that met no SNP is +0.0 and is added all the same: it changes no bit).
A label outside [0, A) counts for no ancestry at its window.

scores_literal: loops, one add at a time.  scores: the same order vectorised over haplotypes and scores (bit for bit the literal one).
score_fsum: math.fsum of the same terms per output, the order-free reference."""
import math

import numpy as np


def windows(C, M, W):
    """[(first column, one past the last)] of the W windows: the last one takes the remainder"""
    return [(k * M, C if k == W - 1 else (k + 1) * M) for k in range(W)]


def scores_literal(X, labels, M, A, weights, effect):
    """-> score (N / 2, A, S) float64, n_effect, n_scored, n_miss (N / 2, A) int32, n_bad"""
    X, labels = np.asarray(X), np.asarray(labels)
    N, C = X.shape
    W, S = labels.shape[1], weights.shape[2]
    score = np.zeros((N // 2, A, S))
    ne, ns, nm = (np.zeros((N // 2, A), np.int32) for _ in range(3))
    n_bad = 0
    for i in range(N // 2):
        for k, (c0, c1) in enumerate(windows(C, M, W)):
            for h in (2 * i, 2 * i + 1):
                a = int(labels[h, k])
                if a < 0 or a >= A:
                    n_bad += 1
                    continue
                p = [0.0] * S
                for c in range(c0, c1):
                    if effect[c] == 255:
                        continue
                    x = int(X[h, c])
                    if x not in (0, 1):
                        nm[i, a] += 1
                        continue
                    ns[i, a] += 1
                    if x == int(effect[c]):
                        ne[i, a] += 1
                        for s in range(S):
                            p[s] = p[s] + float(weights[c, a, s])
                for s in range(S):
                    score[i, a, s] = score[i, a, s] + p[s]
    return score, ne, ns, nm, n_bad


def scores(X, labels, M, A, weights, effect):
    """the same values in the same order, vectorised over haplotypes and scores"""
    X, labels = np.asarray(X), np.asarray(labels)
    weights = np.asarray(weights, dtype=np.float64)
    N, C = X.shape
    W, S = labels.shape[1], weights.shape[2]
    score = np.zeros((N // 2, A, S))
    ne, ns, nm = (np.zeros((N // 2, A), np.int32) for _ in range(3))
    ok_lab = (labels >= 0) & (labels < A)
    n_bad = int((~ok_lab).sum())
    ind = np.arange(N // 2)
    for k, (c0, c1) in enumerate(windows(C, M, W)):
        valid = ok_lab[:, k]
        a_h = np.where(valid, labels[:, k], 0)
        p = np.zeros((N, S))
        cnt = np.zeros((N, 3), np.int32)
        for c in range(c0, c1):
            if effect[c] == 255:
                continue
            x = X[:, c]
            called = (x == 0) | (x == 1)
            hit = valid & called & (x == int(effect[c]))
            cnt[:, 0] += hit
            cnt[:, 1] += valid & called
            cnt[:, 2] += valid & ~called
            rows = np.nonzero(hit)[0]
            p[rows] = p[rows] + weights[c, a_h[rows], :]
        for par in (0, 1):                                   # row 2 i before row 2 i + 1
            rows = np.nonzero(valid[par::2])[0]
            h = 2 * rows + par
            score[ind[rows], a_h[h]] = score[ind[rows], a_h[h]] + p[h]
            ne[ind[rows], a_h[h]] += cnt[h, 0]
            ns[ind[rows], a_h[h]] += cnt[h, 1]
            nm[ind[rows], a_h[h]] += cnt[h, 2]
    return score, ne, ns, nm, n_bad


def score_fsum(X, labels, M, A, weights, effect):
    """-> (score by math.fsum per output, n_terms (N / 2, A) = the number of weights each output sums, sum of |weights| per output
    (N / 2, A, S), also by fsum)"""
    X, labels = np.asarray(X), np.asarray(labels)
    N, C = X.shape
    W, S = labels.shape[1], weights.shape[2]
    win = np.minimum(np.arange(C) // M, W - 1)
    eff = np.asarray(effect).astype(np.int16)
    score, mag = np.zeros((N // 2, A, S)), np.zeros((N // 2, A, S))
    n_terms = np.zeros((N // 2, A), np.int64)
    for i in range(N // 2):
        for a in range(A):
            terms = []
            for h in (2 * i, 2 * i + 1):
                sel = (labels[h, win] == a) & (eff != 255) & (X[h].astype(np.int16) == eff)
                terms.append(np.nonzero(sel)[0])
            cols = np.concatenate(terms)
            n_terms[i, a] = len(cols)
            for s in range(S):
                score[i, a, s] = math.fsum(weights[cols, a, s].tolist())
                mag[i, a, s] = math.fsum(np.abs(weights[cols, a, s]).tolist())
    return score, n_terms, mag


def bound(n_terms, mag):
    """the standard bound of summing n terms in ANY order, one rounding per add, against their exact sum: (n - 1) u sum |terms| with
    u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, to first order in u), padded by (1 + 2^-40) for the
    higher-order terms.  Derived, not measured.  (One term: the sum is the term, the bound is 0.)"""
    return np.maximum(n_terms - 1, 0)[:, :, None] * 2.0 ** -53 * mag * (1 + 2.0 ** -40)
