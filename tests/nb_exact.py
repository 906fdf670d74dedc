"""A numpy restatement of the Naive-Bayes bases (include/gnomix_hip.h, gnx_nb_window): tables from the fitted attributes, a plain
sequential float64 sum that starts at the bias and walks the window's positions in order, and the kernel's normalisation.
Independent of gnomix_amd.convert: the tables are rebuilt here from scikit-learn's formulas."""
import os

import numpy as np


def window_columns(C, M, ctx, w):
    W, rem = C // M, C - M * (C // M)
    width = M + 2 * ctx + (rem if w == W - 1 else 0)
    p = w * M + np.arange(width)
    return np.where(p < ctx, ctx - 1 - p, np.where(p < ctx + C, p - ctx, C - 1 - (p - ctx - C)))


def tables(kind, attrs, A):
    """-> (table (width, 4, A), bias (A,)); classes absent from classes_ get zero rows and bias -inf"""
    cols = np.asarray(attrs["classes_"]).astype(np.int64)
    v = np.arange(4, dtype=np.float64)
    if kind == "gaussian":
        theta, var = np.asarray(attrs["theta_"], np.float64), np.asarray(attrs["var_"], np.float64)
        t = np.stack([-0.5 * (c - theta) ** 2 / var for c in v])
        b = np.log(np.asarray(attrs["class_prior_"], np.float64)) - 0.5 * np.sum(np.log(2.0 * np.pi * var), axis=1)
    else:
        flp = np.asarray(attrs["feature_log_prob_"], np.float64)
        t = np.stack([np.log(1.0 - np.exp(flp)), flp, flp, flp]) if kind == "bernoulli" else np.stack([c * flp for c in v])
        b = np.asarray(attrs["class_log_prior_"], np.float64)
    table = np.zeros((t.shape[2], 4, A))
    bias = np.full(A, -np.inf)
    table[:, :, cols] = np.transpose(t, (2, 0, 1))
    bias[cols] = b
    return table, bias


def jll_window(Xw, table, bias):
    """Xw (N, width) codes 0..3 -> jll (N, A): bias, then one addition per position, in position order"""
    acc = np.tile(np.where(np.isfinite(bias), bias, 0.0), (Xw.shape[0], 1))
    for p in range(Xw.shape[1]):
        acc = acc + table[p][Xw[:, p].astype(np.int64) & 3]
    acc[:, ~np.isfinite(bias)] = -np.inf
    return acc


def softmax(jll):
    m = jll.max(axis=1, keepdims=True)
    e = np.where(np.isfinite(jll), np.exp(np.maximum(jll - m, -746.0)), 0.0)
    return e / e.sum(axis=1, keepdims=True)


def predict(X, wins, C, M, ctx, A):
    """X (N, C) codes; wins: per window (table, bias) -> (B (N, W, A) float64, jll (N, W, A))"""
    W = C // M
    B, J = np.zeros((X.shape[0], W, A)), np.zeros((X.shape[0], W, A))
    for w in range(W):
        table, bias = wins[w]
        cols = window_columns(C, M, ctx, w)
        J[:, w] = jll_window(X[:, cols], table[:len(cols)], bias)
        B[:, w] = softmax(J[:, w])
    return B, J


def tolerance(J):
    """the bar on B for rows whose restated jll is J (..., A): 1e-12 where max |jll| <= 512, else 8 ulp(max |jll|), the spacing that
    scikit-learn's own jll - logsumexp carries"""
    big = np.max(np.abs(np.where(np.isfinite(J), J, 0.0)), axis=-1)
    return np.where(big <= 512.0, 1e-12, 8.0 * np.spacing(big))


# ---- what the host and the GPU tests share: fixtures, live scikit-learn estimators, counts in numpy, panels ----
KINDS = ("bernoulli", "multinomial", "gaussian")
ATTRS = {"bernoulli": ("feature_log_prob_", "class_log_prior_"), "multinomial": ("feature_log_prob_", "class_log_prior_"),
         "gaussian": ("theta_", "var_", "class_prior_")}


def golden_attrs(g, kind, w):
    d = {nm: g["%s_w%d_%s" % (kind, w, nm)] for nm in ATTRS[kind]}
    d["classes_"] = np.arange(int(g["A"]))
    return d


def golden_windows(g, kind):
    return [tables(kind, golden_attrs(g, kind, w), int(g["A"])) for w in range(int(g["C"]) // int(g["M"]))]


def sk_estimator(kind, alpha=1e-10):
    from sklearn.naive_bayes import BernoulliNB, GaussianNB, MultinomialNB
    return {"bernoulli": lambda: BernoulliNB(alpha=alpha), "multinomial": lambda: MultinomialNB(alpha=alpha), "gaussian": GaussianNB}[kind]()


def numpy_counts(X, y, C, M, ctx, A):
    W = C // M
    ldw = M + 2 * ctx + C - M * W
    n1, n2, cc = np.zeros((W, A, ldw), np.int32), np.zeros((W, A, ldw), np.int32), np.zeros((W, A), np.int32)
    for w in range(W):
        cols = window_columns(C, M, ctx, w)
        for c in range(A):
            rows = X[y[:, w] == c][:, cols]
            n1[w, c, :len(cols)], n2[w, c, :len(cols)], cc[w, c] = (rows == 1).sum(0), (rows == 2).sum(0), len(rows)
    return n1, n2, cc


def degenerate_panel():
    """A = 3, 120 rows, freq ~ U(0.05, 0.95): has class-monomorphic cells"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden_knn import panel
    rng = np.random.RandomState(5)
    C, M, A, ctx = 131, 20, 3, 5
    freq = rng.uniform(0.05, 0.95, size=(A, C))
    X, y = panel(rng, freq, 120, C // M, M, 0.01)
    Xq, _ = panel(rng, freq, 40, C // M, M, 0.01)
    return C, M, A, ctx, X, y.astype(np.int32), Xq


def e2e_data(seed):
    """three splits at C = 295, M = 24 (W = 12, remainder 7), context 5, A = 3: ancestry-dependent allele frequencies, labels in
    tracts"""
    C, M, cx, A = 295, 24, 5, 3
    W = C // M
    rng = np.random.RandomState(seed)
    f = rng.uniform(0.05, 0.95, (A, C))

    def split(n):
        y = np.empty((n, W), np.int32)
        for i in range(n):
            cut = rng.randint(0, W + 1)
            y[i, :cut], y[i, cut:] = rng.randint(A), rng.randint(A)
        y[:A] = np.arange(A)[:, None]
        anc = np.repeat(y, M, axis=1)
        anc = np.concatenate([anc, np.repeat(anc[:, -1:], C - W * M, axis=1)], axis=1)
        X = (rng.uniform(size=(n, C)) < f[anc, np.arange(C)[None, :]]).astype(np.int8)
        X[rng.uniform(size=X.shape) < 0.01] = 2
        return X, y

    return (C, M, cx, A), (split(80), split(60), split(40))
