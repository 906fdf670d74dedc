"""The LDA base (LDABase) restated in plain numpy: the integers of the fit (int64 Gram matrix, class sums, class counts), the fit from
them (gnomix_amd.train.lda_finish, the package's one host function), scikit-learn's own svd steps on the data matrix (for the ranks),
the decision and predict_proba, and the panels the host and GPU tests share."""
import numpy as np

from gnomix_amd.train import lda_finish, window_columns

SIXTH = dict(C=203, M=24, cx=12, A=3, N=96)   # W = 8, widths 48 and 59 (remainder 11)
# N, width, A, duplicated / constant columns: the single-window shapes the Gram route was first checked on
TABLE = ((96, 24, 3, 0), (96, 24, 3, 2), (300, 48, 7, 3), (40, 48, 3, 0), (300, 48, 2, 2))


def draw(rng, n, C, W, M, A, freq, miss=0.02):
    """n haplotypes with per-class allele frequencies freq (A, C), labels constant per row except for one switch; the first 2 A rows
    are single-ancestry so that every window holds every class at least twice"""
    y = np.empty((n, W), np.int32)
    for i in range(n):
        cut = rng.randint(0, W + 1)
        y[i, :cut], y[i, cut:] = rng.randint(A), rng.randint(A)
    k = min(n, 2 * A)
    y[:k] = (np.arange(k) % A)[:, None]
    anc = np.repeat(y, M, axis=1)
    anc = np.concatenate([anc, np.repeat(anc[:, -1:], C - W * M, axis=1)], axis=1)
    X = (rng.uniform(size=(n, C)) < freq[anc, np.arange(C)[None, :]]).astype(np.int8)
    X[rng.uniform(size=X.shape) < miss] = 2
    return X, y


def sixth_panel(A=3, N=96, seed=25, n_query=64):
    """the sixth shape: window 0 holds two duplicated and two constant columns (beside the duplicates its reflected edge makes), window
    3 two columns that are constant within every class but not overall -> (C, M, cx, A), X, y, Xq"""
    C, M, cx = SIXTH["C"], SIXTH["M"], SIXTH["cx"]
    W = C // M
    rng = np.random.RandomState(seed + A)
    freq = rng.uniform(0.1, 0.9, (A, C))
    X, y = draw(rng, N, C, W, M, A, freq)
    Xq, _ = draw(rng, n_query, C, W, M, A, freq)
    X[:, 5], X[:, 9] = X[:, 4], X[:, 8]           # columns 0..11 are window 0's alone
    X[:, 3], X[:, 7] = 1, 0
    for j in (80, 85):                            # columns 72..95 are window 3's alone
        X[:, j] = (y[:, 3] + j) % 3
    return (C, M, cx, A), X, y, Xq


def table_panel(i, n_query=64):
    """shape i of TABLE as a one-window model (C = M = width, no context) -> (C, M, cx, A), X, y, Xq"""
    N, width, A, nd = TABLE[i]
    rng = np.random.RandomState(100 + i)
    freq = rng.uniform(0.1, 0.9, (A, width))
    X, y = draw(rng, N, width, 1, width, A, freq)
    Xq, _ = draw(rng, n_query, width, 1, width, A, freq)
    for d in range(nd):
        X[:, 2 * d + 1] = X[:, 2 * d]             # duplicates
        X[:, width - 1 - d] = d % 3               # constants
    return (width, width, 0, A), X, y, Xq


def numpy_gram(X, y, C, M, cx, A, w0=0, w1=None):
    """int64 G (nw, ldw, ldw), S (nw, A, ldw), n (nw, A) of the windows [w0, w1): what gnx_train_lda_gram must return, exactly"""
    W = C // M
    w1 = W if w1 is None else w1
    ldw = M + 2 * cx + C - M * W
    G, S, n = np.zeros((w1 - w0, ldw, ldw), np.int64), np.zeros((w1 - w0, A, ldw), np.int64), np.zeros((w1 - w0, A), np.int64)
    for w in range(w0, w1):
        Xw = X[:, window_columns(C, M, cx, w)].astype(np.int64)
        k = Xw.shape[1]
        G[w - w0, :k, :k] = Xw.T @ Xw
        for a in range(A):
            rows = y[:, w] == a
            S[w - w0, a, :k], n[w - w0, a] = Xw[rows].sum(axis=0), rows.sum()
    return G, S, n


def fit(X, y, C, M, cx, A, tol=1e-4):
    """every window's fit from the int64 integers through lda_finish -> coef (W, R, ldw), intercept (W, R), infos"""
    W, R = C // M, (1 if A == 2 else A)
    G, S, n = numpy_gram(X, y, C, M, cx, A)
    coef, icpt, infos = np.zeros((W, R, G.shape[1])), np.zeros((W, R)), []
    for w in range(W):
        k = len(window_columns(C, M, cx, w))
        c, b, info = lda_finish(G[w, :k, :k], S[w, :, :k], n[w], X.shape[0], tol)
        coef[w, :, :k], icpt[w] = c, b
        infos.append(info)
    return coef, icpt, infos


def sklearn_svd_steps(Xw, yw, tol=1e-4):
    """scikit-learn's LinearDiscriminantAnalysis._solve_svd on the data matrix itself, step by step as its source documents them ->
    rank, rank2, the singular values of both SVDs (what the Gram route's ranks are compared with)"""
    Xw = np.asarray(Xw, dtype=np.float64)
    classes = np.unique(yw)
    N, K = len(Xw), len(classes)
    means = np.stack([Xw[yw == k].mean(axis=0) for k in classes])
    priors = np.array([(yw == k).sum() for k in classes]) / float(N)
    Xc = np.concatenate([Xw[yw == k] - means[i] for i, k in enumerate(classes)], axis=0)
    xbar = priors @ means
    std = Xc.std(axis=0)
    std[std == 0] = 1.0
    Xs = np.sqrt(1.0 / (N - K)) * (Xc / std)
    _, sv, Vt = np.linalg.svd(Xs, full_matrices=False)
    rank = int(np.sum(sv > tol))
    scalings = (Vt[:rank] / std).T / sv[:rank]
    Xb = (np.sqrt((N * priors) * (1.0 / (K - 1))) * (means - xbar).T).T @ scalings
    _, sv2, _ = np.linalg.svd(Xb, full_matrices=False)
    return rank, int(np.sum(sv2 > tol * sv2[0])), sv, sv2


def decision(Xq, coef, icpt, C, M, cx):
    """(Nq, W, R) float64: Xw @ coef_w.T + intercept_w"""
    W = C // M
    D = np.zeros((len(Xq), W, coef.shape[1]))
    for w in range(W):
        cols = window_columns(C, M, cx, w)
        D[:, w] = Xq[:, cols].astype(np.float64) @ coef[w, :, :len(cols)].T + icpt[w]
    return D


def proba(D, A):
    """scikit-learn's predict_proba of the decision: softmax for A > 2, [1 - expit(d), expit(d)] for A == 2"""
    if A == 2:
        p = 1.0 / (1.0 + np.exp(-D[..., 0]))
        return np.stack([1.0 - p, p], axis=-1)
    e = np.exp(D - D.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def predict(Xq, coef, icpt, C, M, cx, A):
    return proba(decision(Xq, coef, icpt, C, M, cx), A)


def decision_bound(Xq, coef, icpt, C, M, cx):
    """per (row, window): the bound on |d - d_numpy| of a float64 sum in any order, (width + 2) 2^-53 (sum_p |c_p x_p| + |b|), maximum
    over the decision rows"""
    W = C // M
    Bd = np.zeros((len(Xq), W))
    for w in range(W):
        cols = window_columns(C, M, cx, w)
        mag = np.abs(Xq[:, cols].astype(np.float64)) @ np.abs(coef[w, :, :len(cols)]).T + np.abs(icpt[w])
        Bd[:, w] = ((len(cols) + 2) * 2.0 ** -53 * mag).max(axis=1)
    return Bd


def e2e_data(seed):
    """three splits at the sixth shape, A = 3: ancestry-dependent allele frequencies, labels in tracts"""
    C, M, cx, A = SIXTH["C"], SIXTH["M"], SIXTH["cx"], 3
    rng = np.random.RandomState(seed)
    f = rng.uniform(0.05, 0.95, (A, C))
    return (C, M, cx, A), tuple(draw(rng, n, C, C // M, M, A, f, miss=0.01) for n in (96, 60, 40))
