"""The 1-nearest-neighbour base restated in numpy: integer squared distances, ties to the lowest fit-row index.

What gnomix_amd/csrc/knn/k_base_knn.hip must reproduce EXACTLY (its header states the same rules):
  B[n, w, c] = 1.0 if c == y_w[argmin_i |x_nw - fit_wi|^2] else 0.0, the argmin taking the lowest index among equal distances;
  x_nw = the window's slice of the reflect-padded query (base.py:41-44, :146-164); codes are numbers (2 = missing is 2, 3 is 3).
Nothing here imports the package under test."""
import numpy as np


def window_columns(C, M, ctx, w):
    """columns of X that window w reads, in order (reflect padding by ctx on both ends; the last window takes the remainder)"""
    W = C // M
    width = M + 2 * ctx + ((C - M * W) if w == W - 1 else 0)
    p = w * M + np.arange(width)
    return np.where(p < ctx, ctx - 1 - p, np.where(p < ctx + C, p - ctx, C - 1 - (p - ctx - C)))


def shared_windows(X, y, C, M, ctx):
    """the per-window (xfit, labels) pairs of a fit on X (n, C), y (n, W)"""
    return [(np.ascontiguousarray(X[:, window_columns(C, M, ctx, w)]), np.asarray(y[:, w])) for w in range(C // M)]


def d2_matrix(xq, xf):
    """(n_query, n_fit) int64 squared Euclidean distances of integer rows"""
    q, f = np.asarray(xq, dtype=np.int64), np.asarray(xf, dtype=np.int64)
    return (q * q).sum(1)[:, None] + (f * f).sum(1)[None, :] - 2 * (q @ f.T)


def predict(Xq, wins, C, M, ctx, A):
    """-> B (N, W, A) float64 one-hot, idx (N, W) the chosen fit row, amb (N, W) bool: the minimum-distance rows carry > 1 label"""
    N, W = Xq.shape[0], C // M
    B = np.zeros((N, W, A), np.float64)
    idx = np.zeros((N, W), np.int64)
    amb = np.zeros((N, W), bool)
    for w, (xf, yw) in enumerate(wins):
        d2 = d2_matrix(Xq[:, window_columns(C, M, ctx, w)], xf)
        i = np.argmin(d2, axis=1)          # numpy's argmin returns the FIRST minimum: the lowest index
        idx[:, w] = i
        yw = np.asarray(yw)
        B[np.arange(N), w, yw[i]] = 1.0
        tied = d2 == d2.min(axis=1, keepdims=True)
        lo = np.where(tied, yw[None, :], A).min(axis=1)
        hi = np.where(tied, yw[None, :], -1).max(axis=1)
        amb[:, w] = lo != hi
    return B, idx, amb


def tied_classes(xq_w, xf, yw):
    """per query row: the set of labels among the minimum-distance fit rows"""
    d2 = d2_matrix(xq_w, xf)
    tied = d2 == d2.min(axis=1, keepdims=True)
    return [set(np.asarray(yw)[t].tolist()) for t in tied]
