"""A numpy restatement of libsvm's probability prediction for an RBF SVC on SNP codes, in the arithmetic the device uses: the
integer squared distance d2, the kernel value from a table T[k] = exp(-gamma k) built with the C library's exp (math.exp), the
pairwise decision sums in libsvm's order (class-major, support-vector order inside a class, multiply then add, no fused
multiply-add), sigmoid_predict and multiclass_probability (Wu, Lin, Weng).  tests/test_svm_rbf_host.py pins it to the reference's
own SVMBase output (G21) within 1e-12; the GPU tests lean on it where scikit-learn has no say (query code 3)."""
import math

import numpy as np


def window_columns(C, M, context, w):
    W, rem = C // M, C - M * (C // M)
    width = M + 2 * context + (rem if w == W - 1 else 0)
    p = w * M + np.arange(width)
    return np.where(p < context, context - 1 - p, np.where(p < context + C, p - context, C - 1 - (p - context - C)))


def rbf_table(gamma, n):
    return np.array([math.exp(-gamma * k) for k in range(int(n))], dtype=np.float64)


def decision_values(win, Xw):
    """win: dict with xfit (n_sv, width) int8 support rows, dual_coef (A-1, n_sv), intercept (P,), n_support (A,), gamma;
    Xw (n, width) -> (n, P) ovo decision values"""
    sv = np.asarray(win["xfit"], dtype=np.int64)[np.asarray(win["support"])]
    Xw = np.asarray(Xw, dtype=np.int64)
    d2 = (Xw * Xw).sum(1)[:, None] + (sv * sv).sum(1)[None, :] - 2 * Xw @ sv.T
    K = rbf_table(float(win["gamma"]), 9 * Xw.shape[1] + 1)[d2]
    coef = np.asarray(win["dual_coef"], dtype=np.float64)
    start = np.concatenate([[0], np.cumsum(np.asarray(win["n_support"]))])
    A = len(start) - 1
    out = []
    for i in range(A):
        for j in range(i + 1, A):
            si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
            prod = np.concatenate([coef[j - 1, si][None, :] * K[:, si], coef[i, sj][None, :] * K[:, sj]], axis=1)
            acc = np.zeros(Xw.shape[0])
            for t in range(prod.shape[1]):   # sequential, one rounding per add
                acc = acc + prod[:, t]
            out.append(acc + np.asarray(win["intercept"])[len(out)])
    return np.stack(out, axis=1)


def sigmoid_predict(dec, pa, pb):
    f = dec * pa + pb
    if f >= 0:
        return math.exp(-f) / (1.0 + math.exp(-f))
    return 1.0 / (1.0 + math.exp(f))


def multiclass_probability(k, r):
    max_iter = max(100, k)
    Q = np.zeros((k, k))
    Qp = np.zeros(k)
    p = np.full(k, 1.0 / k)
    eps = 0.005 / k
    for t in range(k):
        Q[t, t] = 0.0
        for j in range(t):
            Q[t, t] += r[j][t] * r[j][t]
            Q[t, j] = Q[j, t]
        for j in range(t + 1, k):
            Q[t, t] += r[j][t] * r[j][t]
            Q[t, j] = -r[j][t] * r[t][j]
    for _ in range(max_iter):
        pQp = 0.0
        for t in range(k):
            Qp[t] = 0.0
            for j in range(k):
                Qp[t] += Q[t, j] * p[j]
            pQp += p[t] * Qp[t]
        max_error = 0.0
        for t in range(k):
            max_error = max(max_error, abs(Qp[t] - pQp))
        if max_error < eps:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t, j]) / (1 + diff)
                p[j] /= (1 + diff)
    return p


def predict_proba_window(win, Xw):
    dec = decision_values(win, Xw)
    A = len(win["n_support"])
    pa, pb = np.asarray(win["prob_a"]), np.asarray(win["prob_b"])
    out = np.zeros((dec.shape[0], A))
    min_prob = 1e-7
    for n in range(dec.shape[0]):
        r = [[0.0] * A for _ in range(A)]
        k = 0
        for i in range(A):
            for j in range(i + 1, A):
                r[i][j] = min(max(sigmoid_predict(float(dec[n, k]), float(pa[k]), float(pb[k])), min_prob), 1 - min_prob)
                r[j][i] = 1 - r[i][j]
                k += 1
        out[n] = multiclass_probability(A, r)
    return out


def predict_proba(svc, X, C, M, context):
    """svc: list of window dicts -> B (N, W, A)"""
    X = np.asarray(X)
    return np.stack([predict_proba_window(win, X[:, window_columns(C, M, context, w)]) for w, win in enumerate(svc)], axis=1)


def golden_windows(g):
    """G21's per-window arrays as the dicts GnxModelData.svc holds (support rows only)"""
    C, M, ctx = int(g["C"]), int(g["M"]), int(g["ctx"])
    svc = []
    for w in range(C // M):
        sup = g["w%d_support" % w]
        svc.append(dict(xfit=np.ascontiguousarray(g["Xt"][sup][:, window_columns(C, M, ctx, w)]), support=np.arange(len(sup), dtype=np.int32),
                        dual_coef=g["w%d_dual" % w], intercept=g["w%d_intercept" % w], prob_a=g["w%d_probA" % w],
                        prob_b=g["w%d_probB" % w], n_support=g["w%d_n_support" % w], kernel=np.array("rbf"),
                        gamma=np.float64(g["w%d_gamma" % w])))
    return svc
