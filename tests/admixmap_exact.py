"""The contract of admixture mapping restated (gnx_ancestry_admixmap and gnomix_amd/admixmap.py), independent of both: the
blocks summed in rational arithmetic, the fits by numpy.linalg.lstsq on the explicit kept design, F also from Fraction arithmetic, the
Freedman-Lane permutations.  Not a test.

INPUTS.  labels (N, W) int32, rows 2 i and 2 i + 1 are individual i; Y (N / 2, T) float64, T >= 1; Z (N / 2, K) float64 with the caller's
intercept column; use (N / 2,) bytes or None.  There is no X.
PARTICIPATION.  Individual i takes part at window k when use[i] != 0, Z[i, :] is finite, every entry of Y[i, :] is finite and both labels at k
lie in [0, A).  Labels out of range are only compared; they are counted over ALL rows (n_bad).
COUNTS.  h_a[i, k] in {0, 1, 2}: i's haplotypes labelled a at k; n_k the participants; hs[k, a] = sum_i h_a.  Ancestry a is KEPT at k when
hs[k, a] >= min_hap and 2 n_k - hs[k, a] >= min_hap.
PER-ANCESTRY TEST.  For every kept a: y = Z g + alpha_a h_a by OLS over the participants -> beta, se, t (df = n_k - K - 1); NaN for a cell that
is not kept or whose design [Z, h_a] is rank deficient.
JOINT TEST.  Reference = the kept ancestry with the largest hs (ties: the lowest index); columns = the other kept ancestries; q = kept - 1;
F = ((RSS0 - RSS1) / q) / (RSS1 / df2), df1 = q, df2 = n_k - K - q; NaN when q < 1, df2 < 1 or the full design is rank deficient.
STATUS.  2: n_k - K - 1 < 1;  1: Z^T Z singular;  3: q < 1 (the kept cells are still fitted);  0 otherwise.  2 and 1: every float is NaN.
BLOCKS of the windows [w0, w1): win_i = n, hs[a], sum h_a h_b (a <= b); win_g = the upper triangle of Z^T Z row by row, then Z^T H;
win_y = [Z, h_0 .. h_{A-1}]^T Y; win_yy = diag(Y^T Y)."""
from fractions import Fraction

import numpy as np

_F = np.frompyfunc(Fraction, 1, 1)


def participation(labels, A, Y, Z, use):
    """-> takes (n_ind, W) bool, H (n_ind, W, A) int64 (zero where the individual takes no part), n_bad"""
    n_ind = labels.shape[0] // 2
    use = np.ones(n_ind, np.uint8) if use is None else np.asarray(use)
    base = (use != 0) & np.isfinite(Z).all(1) & np.isfinite(Y).all(1)
    lab = labels.astype(np.int64)
    ok = (lab >= 0) & (lab < A)
    takes = base[:, None] & ok[0::2] & ok[1::2]
    a = np.arange(A)
    H = ((lab[0::2, :, None] == a) * 1 + (lab[1::2, :, None] == a) * 1) * takes[:, :, None]
    return takes, H, int((~ok).sum())


def blocks(labels, A, Y, Z, use, w0, w1):
    """-> dict: win_i (nw, NI) int64 exact; g, y, yy: the exact values as object arrays of Fractions shaped as win_g (nw, NG), win_y
    (nw, K + A, T), win_yy (nw, T); g_abs, y_abs, yy_abs: the sums of |term|; n_bad (over the windows of the range)"""
    takes, H, _ = participation(labels, A, Y, Z, use)
    K, T = Z.shape[1], Y.shape[1]
    nw = w1 - w0
    iu, ku = np.triu_indices(A), np.triu_indices(K)
    win_i = np.zeros((nw, 1 + A + len(iu[0])), np.int64)
    out = {k: [] for k in ("g", "g_abs", "y", "y_abs", "yy", "yy_abs")}
    for k in range(w0, w1):
        idx = np.flatnonzero(takes[:, k])
        Hk = H[idx, k]
        win_i[k - w0, 0] = len(idx)
        win_i[k - w0, 1:1 + A] = Hk.sum(0)
        win_i[k - w0, 1 + A:] = (Hk.T @ Hk)[iu]
        Zf, Yf, Hf = _F(Z[idx]), _F(Y[idx]), _F(Hk)
        U = np.concatenate([Zf, Hf], 1) if len(idx) else np.zeros((0, K + A), object)
        zero = Fraction(0)
        for name, L, R in (("y", U, Yf), ("yy", None, None), ("g", Zf, U)):
            if name == "yy":
                e = (Yf * Yf).sum(0) if len(idx) else np.full(T, zero, object)
                out["yy"].append(e + zero)
                out["yy_abs"].append(e + zero)
                continue
            e = L.T.dot(R) + zero if len(idx) else np.full((L.shape[1], R.shape[1]), zero, object)
            ea = np.abs(L).T.dot(np.abs(R)) + zero if len(idx) else e
            if name == "g":
                e, ea = (np.concatenate([m[:, :K][ku], m[:, K:].reshape(-1)]) for m in (e, ea))
            out[name].append(e)
            out[name + "_abs"].append(ea)
    lab = labels[:, w0:w1].astype(np.int64)
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(win_i=win_i, n_bad=int(((lab < 0) | (lab >= A)).sum()))
    return res


def float_blocks(labels, A, Y, Z, use, w0, w1):
    """the blocks rounded to float64 once each, in the arrays of the C ABI without the trait padding: win_i, win_g, win_y, win_yy"""
    b = blocks(labels, A, Y, Z, use, w0, w1)
    return b["win_i"].astype(np.int32), b["g"].astype(np.float64), b["y"].astype(np.float64), b["yy"].astype(np.float64)


def _rss_exact(X, y):
    """X (n, p), y (n,) floats -> the residual sum of squares of the least-squares fit as a Fraction; None when X^T X is singular"""
    Xf, yf = _F(X), _F(y)
    p = X.shape[1]
    N = [[Fraction(v) for v in row] for row in Xf.T.dot(Xf)]
    b = [Fraction(v) for v in Xf.T.dot(yf)]
    M = [N[i] + [b[i]] for i in range(p)]
    for c in range(p):
        piv = next((r for r in range(c, p) if M[r][c] != 0), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        for r in range(c + 1, p):
            if M[r][c] != 0:
                f = M[r][c] / M[c][c]
                M[r] = [x - f * z for x, z in zip(M[r], M[c])]
    beta = [Fraction(0)] * p
    for c in range(p - 1, -1, -1):
        beta[c] = (M[c][p] - sum(M[c][j] * beta[j] for j in range(c + 1, p))) / M[c][c]
    return Fraction((yf * yf).sum()) - sum(bi * be for bi, be in zip(b, beta))


def _rank_full(X):
    """the design has full column rank, decided exactly"""
    return X.shape[0] >= X.shape[1] and _rss_exact(X, np.zeros(X.shape[0])) is not None


def _kappa(X):
    s = np.linalg.svd(X / np.sqrt((X * X).sum(0)), compute_uv=False)
    return float(s[0] / s[-1])


def fit(labels, A, Y, Z, use, min_hap=1, exact_F=True):
    """-> dict: beta, se, t (W, A, T), F (W, T) by float64 lstsq; F_exact (W, T) from Fraction arithmetic (NaN where F is; only with
    exact_F); df1, df2, n (W,), hs (W, A), kept (W, A) bool, status (W,); kappa (W,): the largest 2-norm condition number of the
    column-scaled designs fitted at the window; p_kept (W,): the columns of the largest design fitted there"""
    takes, H, _ = participation(labels, A, Y, Z, use)
    n_ind, W = takes.shape
    K, T = Z.shape[1], Y.shape[1]
    r = dict(beta=np.full((W, A, T), np.nan), se=np.full((W, A, T), np.nan), t=np.full((W, A, T), np.nan), F=np.full((W, T), np.nan),
             F_exact=np.full((W, T), np.nan), df1=np.zeros(W, np.int32), df2=np.zeros(W, np.int32), n=np.zeros(W, np.int32),
             hs=np.zeros((W, A), np.int32), kept=np.zeros((W, A), bool), status=np.zeros(W, np.int32), kappa=np.ones(W), p_kept=np.full(W, K + 1))
    for k in range(W):
        idx = np.flatnonzero(takes[:, k])
        n, Zk, Yk, Hk = len(idx), Z[idx], Y[idx], H[idx, k].astype(np.float64)
        hs = H[idx, k].sum(0)
        kept = (hs >= min_hap) & (2 * n - hs >= min_hap)
        q = int(kept.sum()) - 1
        r["n"][k], r["hs"][k], r["kept"][k], r["df1"][k], r["df2"][k] = n, hs, kept, q, n - K - q
        df = n - K - 1
        if df < 1:
            r["status"][k] = 2
            continue
        if not _rank_full(Zk):
            r["status"][k] = 1
            continue
        r["status"][k] = 3 if q < 1 else 0
        kap = _kappa(Zk)
        for a in np.flatnonzero(kept):
            X = np.concatenate([Zk, Hk[:, a:a + 1]], 1)
            if not _rank_full(X):
                continue
            kap = max(kap, _kappa(X))
            beta, _, _, _ = np.linalg.lstsq(X, Yk, rcond=None)
            res = Yk - X @ beta
            s2 = (res * res).sum(0) / df
            se = np.sqrt(s2 * np.linalg.inv(X.T @ X)[K, K])
            r["beta"][k, a], r["se"][k, a], r["t"][k, a] = beta[K], se, beta[K] / se
        if q >= 1 and n - K - q >= 1:
            ref = int(np.argmax(np.where(kept, hs, -1)))
            cols = [a for a in np.flatnonzero(kept) if a != ref]
            X = np.concatenate([Zk, Hk[:, cols]], 1)
            if _rank_full(X):
                kap = max(kap, _kappa(X))
                r["p_kept"][k] = K + q
                df2 = n - K - q
                res0 = Yk - Zk @ np.linalg.lstsq(Zk, Yk, rcond=None)[0]
                res1 = Yk - X @ np.linalg.lstsq(X, Yk, rcond=None)[0]
                rss0, rss1 = (res0 * res0).sum(0), (res1 * res1).sum(0)
                r["F"][k] = ((rss0 - rss1) / q) / (rss1 / df2)
                if exact_F:
                    for t in range(T):
                        e0, e1 = _rss_exact(Zk, Yk[:, t]), _rss_exact(X, Yk[:, t])
                        r["F_exact"][k, t] = float(((e0 - e1) / q) / (e1 / df2)) if e1 != 0 else np.nan
        r["kappa"][k] = kap
    return r


def permutation_columns(Y, Z, use, seed, j0, j1):
    """Freedman-Lane: per trait g = lstsq(Z, y) over the base participants (those use, Z and Y admit), e = y - Z g; permutation j is
    numpy.random.Generator(PCG64([seed, j])).permutation(n_base) applied to e -> (n_ind, (j1 - j0) * T), column (j - j0) * T + t; NaN
    rows for the others"""
    n_ind, T = Y.shape
    base = (np.asarray(use) != 0) & np.isfinite(Z).all(1) & np.isfinite(Y).all(1)
    Zb, Yb = Z[base], Y[base]
    fitted = Zb @ np.linalg.lstsq(Zb, Yb, rcond=None)[0]
    e = Yb - fitted
    out = np.full((n_ind, (j1 - j0) * T), np.nan)
    for j in range(j0, j1):
        pi = np.random.Generator(np.random.PCG64([seed, j])).permutation(int(base.sum()))
        out[base, (j - j0) * T:(j - j0 + 1) * T] = fitted + e[pi]
    return out


def permutation_maxima(labels, A, Y, Z, use, min_hap, n_perm, seed, want_scale=False):
    """-> perm_max_t, perm_max_F (T, n_perm) by lstsq on every permuted column; want_scale: also p kappa^2 2^-53 max_a |beta| of the window
    and column where perm_max_t is attained (the scale of the results' bound there)"""
    T = Y.shape[1]
    Yp = permutation_columns(Y, Z, use, seed, 0, n_perm)
    base = ~np.isnan(Yp).any(1)
    f = fit(labels, A, np.where(base[:, None], Yp, 0.0), Z, base.astype(np.uint8), min_hap, exact_F=False)
    with np.errstate(invalid="ignore"):
        mt = np.nanmax(np.abs(f["t"]).reshape(-1, n_perm, T), axis=0).T
        mF = np.nanmax(f["F"].reshape(-1, n_perm, T), axis=0).T
        if want_scale:
            W = labels.shape[1]
            at = np.nanargmax(np.abs(f["t"]).reshape(W * A, n_perm * T), axis=0) // A
            bmax = np.nanmax(np.abs(f["beta"]), axis=1)[at, np.arange(n_perm * T)]
            return mt, mF, (f["p_kept"][at] * f["kappa"][at] ** 2 * 2.0 ** -53 * bmax).reshape(n_perm, T).T
    return mt, mF


def adjusted(obs, perm_max):
    """(1 + #{j: perm_max[t, j] >= obs[..., t]}) / (1 + n_perm), NaN where obs is"""
    n_perm = perm_max.shape[1]
    with np.errstate(invalid="ignore"):
        cnt = (perm_max.T[(None,) * (obs.ndim - 1)] >= obs[..., None, :]).sum(-2)
    return np.where(np.isnan(obs), np.nan, (1.0 + cnt) / (1.0 + n_perm))
