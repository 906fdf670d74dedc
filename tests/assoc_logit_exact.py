"""Plain-numpy float64 restatement of the logistic ancestry-specific association of include/gnomix_hip.h (gnx_ancestry_assoc_logit).
Not a test.

The same rule as the device's, step for step: the column rule, the window's null model from theta = 0, the SNP's fit from the null theta,
the evaluation (e = exp(-|eta|), q = 1 / (1 + e), w = (e q) q, deviance term 2 (max(t, 0) + log1p(e))), the unit-diagonal Cholesky with
the 2^-40 pivot rule, lambda2 = g^T delta <= tol -> full step and one more H, else halving at most 10 times, max_iter steps, the
statuses.  Every sum over individuals runs in ascending i (numpy.cumsum cannot reassociate), one product per term rounded once.  What
differs from the device is libm's exp / log1p against csrc/gnx_exp.h's exp and the device library's log1p, ulps apart.

fit() returns the arrays of AncestryAssocLogit's raw side for the SNPs in `cols` (default all); converge() runs the same Newton
iteration on an explicit design with math.fsum sums down to lambda2 <= 1e-26 (the reference the tolerance is measured against)."""
import math

import numpy as np

import allele_counts_exact as AE
import assoc_exact as XE

PIVOT_MIN = 2.0 ** -40
W_MIN = 2.0 ** -40
TOL, MAX_ITER, MAX_HALVINGS = 1e-10, 25, 10


def _seq_sum(terms):
    """sum over axis 0 in ascending order"""
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1:])
    return np.cumsum(terms, axis=0)[-1]


def evaluate(X, y, theta):
    """-> dev, g, H (lower triangle filled both ways), wmin at theta; X (n, q) with dropped columns zeroed"""
    n, q = X.shape
    eta = np.zeros(n)
    for j in range(q):
        eta = eta + X[:, j] * theta[j]
    e = np.exp(-np.abs(eta))
    qq = 1.0 / (1.0 + e)
    eq = e * qq
    case = y == 1.0
    r = np.where(case, np.where(eta >= 0, eq, qq), np.where(eta >= 0, -qq, -eq))
    w = eq * qq
    t = np.where(case, -eta, eta)
    dev = float(_seq_sum(2.0 * (np.where(t > 0, t, 0.0) + np.log1p(e))))
    g = _seq_sum(r[:, None] * X)
    wx = w[:, None] * X
    T = wx[:, :, None] * X[:, None, :]          # [i, j, k] = (w x_j) x_k: used for j >= k
    H = np.tril(_seq_sum(T))
    H = H + np.tril(H, -1).T
    return dev, g, H, (float(w.min()) if n else 1.0)


def factor(H, kept):
    """H to unit diagonal, Cholesky row by row -> L, s, notpd"""
    q = len(kept)
    d = np.diag(H)
    notpd = bool((kept & ~(d > 0)).any())
    s = np.where(d > 0, np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
    L = np.zeros((q, q))
    for j in range(q):
        for k in range(j + 1):
            sm = H[j, k] / (s[j] * s[k]) if k < j else 1.0
            for m in range(k):
                sm = sm - L[j, m] * L[k, m]
            if k < j:
                L[j, k] = sm / L[k, k]
            else:
                ok = sm > PIVOT_MIN and np.isfinite(sm)
                notpd = notpd or not ok
                L[j, j] = math.sqrt(sm if ok else 1.0)
    return L, s, notpd


def solve(L, s, g):
    q = len(g)
    z = np.zeros(q)
    for j in range(q):
        sm = g[j] / s[j]
        for k in range(j):
            sm = sm - L[j, k] * z[k]
        z[j] = sm / L[j, j]
    for j in range(q - 1, -1, -1):
        sm = z[j]
        for k in range(j + 1, q):
            sm = sm - L[k, j] * z[k]
        z[j] = sm / L[j, j]
    delta = z / s
    lam = 0.0
    for j in range(q):
        lam = lam + g[j] * delta[j]
    return delta, lam


def inverse_diag(L, s, j):
    """sqrt((H^-1)_jj) through the factor of the scaled matrix"""
    q = L.shape[0]
    x = np.zeros(q)
    ss = 0.0
    for k in range(j, q):
        sm = 1.0 if k == j else 0.0
        for m in range(j, k):
            sm = sm - L[k, m] * x[m]
        x[k] = sm / L[k, k]
        ss = ss + x[k] * x[k]
    return math.sqrt(ss) / s[j]


def newton(X, y, kept, theta, tol=TOL, max_iter=MAX_ITER):
    """the iteration rule -> dict(status, iters, theta, dev, L, s) (status 0, 1 or 3)"""
    theta = theta.copy()
    dev, g, H, wmin = evaluate(X, y, theta)
    it = 0
    while True:
        if it == max_iter:
            return dict(status=3, iters=it)
        L, s, notpd = factor(H, kept)
        if notpd:
            return dict(status=1, iters=it)
        delta, lam = solve(L, s, g)
        it += 1
        if lam <= tol:
            theta = theta + delta
            dev, g, H, wmin = evaluate(X, y, theta)
            L, s, notpd = factor(H, kept)
            if notpd:
                return dict(status=1, iters=it)
            if wmin < W_MIN:
                return dict(status=3, iters=it)
            return dict(status=0, iters=it, theta=theta, dev=dev, L=L, s=s, H=H)
        t = 1.0
        for h in range(MAX_HALVINGS + 1):
            cand = theta + t * delta
            dev_c, g_c, H_c, _ = evaluate(X, y, cand)
            if dev_c < dev or h == MAX_HALVINGS:
                break
            t *= 0.5
        theta, dev, g, H = cand, dev_c, g_c, H_c


def design(X, labels, M, A, y, Z, use, c):
    """the explicit design of SNP c over its participants -> rows (indices), [Z, h_0..h_{A-2}, d_0..d_{A-1}] float64, y"""
    X = np.asarray(X)
    C, W = X.shape[1], np.asarray(labels).shape[1]
    win = AE.windows(C, M, W)
    part = XE.participation(labels, A, y, Z, use)[:, win[c]]
    lab = np.asarray(labels).astype(np.int64)[:, win[c]]
    la, lb = lab[0::2], lab[1::2]
    xa, xb = (X[0::2, c] == 1), (X[1::2, c] == 1)
    h = np.stack([(la == a).astype(np.float64) + (lb == a) for a in range(A)], 1)
    d = np.stack([((la == a) & xa).astype(np.float64) + ((lb == a) & xb) for a in range(A)], 1)
    D = np.concatenate([np.asarray(Z, np.float64), h[:, :A - 1], d], 1)
    return part, D[part], np.asarray(y, np.float64)[part]


def fit(X, labels, M, A, y, Z, use=None, min_ac=1, cols=None, tol=TOL, max_iter=MAX_ITER):
    """-> dict: beta, se (C, A), dev (C,), theta (C, Q) float64; n_alt, n_alt_case (C, A), n_miss, iters, status (C,) int32 (status -1:
    not in cols); per window theta0 (W, P), dev0, n, n_case, sum_h (W, A), iters0, status0; kept (C, Q) bool; se_theta (C, Q): the standard error of every kept column; kappa (C,): condition number
    of the unit-diagonal Hessian at the optimum (NaN where status != 0)"""
    X = np.asarray(X)
    y, Z = np.asarray(y, np.float64), np.asarray(Z, np.float64)
    N, C = X.shape
    lab = np.asarray(labels).astype(np.int64)
    W = lab.shape[1]
    K = Z.shape[1]
    P, Q = K + A - 1, K + 2 * A - 1
    win = AE.windows(C, M, W)
    partw = XE.participation(labels, A, y, Z, use)
    out = dict(beta=np.full((C, A), np.nan), se=np.full((C, A), np.nan), dev=np.full(C, np.nan), theta=np.full((C, Q), np.nan),
               n_alt=np.zeros((C, A), np.int32), n_alt_case=np.zeros((C, A), np.int32), n_miss=np.zeros(C, np.int32), iters=np.zeros(C, np.int32),
               status=np.full(C, -1, np.int32), theta0=np.full((W, P), np.nan), dev0=np.full(W, np.nan), n=np.zeros(W, np.int32),
               n_case=np.zeros(W, np.int32), sum_h=np.zeros((W, A), np.int32), iters0=np.zeros(W, np.int32), status0=np.zeros(W, np.int32),
               kept=np.zeros((C, Q), bool), kappa=np.full(C, np.nan), se_theta=np.full((C, Q), np.nan))
    Xi = X.astype(np.int64)
    missing = ~((Xi == 0) | (Xi == 1))
    miss2 = missing[0::2].astype(np.int64) + missing[1::2]
    null = {}
    for w in range(W):
        r = partw[:, w]
        la, lb = lab[0::2, w][r], lab[1::2, w][r]
        yy = y[r]
        h = np.stack([(la == a).astype(np.float64) + (lb == a) for a in range(A)], 1) if r.any() else np.zeros((0, A))
        out["n"][w], out["n_case"][w], out["sum_h"][w] = r.sum(), (yy == 1.0).sum(), h.sum(0)
        kept = np.concatenate([np.ones(K, bool), out["sum_h"][w, :A - 1] > 0])
        U = np.concatenate([Z[r], h[:, :A - 1]], 1)
        if out["n"][w] - kept.sum() < 1:
            out["status0"][w] = 2
        else:
            res = newton(U, yy, kept, np.zeros(P), tol, max_iter)
            out["status0"][w], out["iters0"][w] = res["status"], res["iters"]
            if res["status"] == 0:
                out["theta0"][w], out["dev0"][w] = res["theta"], res["dev"]
        null[w] = (r, U, yy, kept, la, lb)
    for c in range(C):
        w = win[c]
        r, U, yy, kept0, la, lb = null[w]
        xa, xb = (X[0::2, c] == 1)[r], (X[1::2, c] == 1)[r]
        d = np.stack([((la == a) & xa).astype(np.float64) + ((lb == a) & xb) for a in range(A)], 1) if r.any() else np.zeros((0, A))
        out["n_alt"][c] = d.sum(0)
        out["n_alt_case"][c] = (d * yy[:, None]).sum(0)
        out["n_miss"][c] = (miss2[:, c] * r).sum()
        keep_d = (out["n_alt"][c] >= min_ac) & (out["n_alt_case"][c] > 0) & (out["n_alt_case"][c] < out["n_alt"][c])
        kept = np.concatenate([kept0, keep_d])
        out["kept"][c] = kept
        if cols is not None and c not in cols:
            continue
        if out["status0"][w] != 0:
            out["status"][c] = 4
            continue
        if out["n"][w] - kept.sum() < 1:
            out["status"][c] = 2
            continue
        D = np.concatenate([U, d * keep_d[None, :]], 1)
        res = newton(D, yy, kept, np.concatenate([out["theta0"][w], np.zeros(A)]), tol, max_iter)
        out["status"][c], out["iters"][c] = res["status"], res["iters"]
        if res["status"] != 0:
            continue
        out["theta"][c], out["dev"][c] = res["theta"], res["dev"]
        for j in np.flatnonzero(kept):
            out["se_theta"][c, j] = inverse_diag(res["L"], res["s"], j)
        out["beta"][c, keep_d] = res["theta"][P:][keep_d]
        out["se"][c, keep_d] = out["se_theta"][c, P:][keep_d]
        Hk = res["H"][np.ix_(kept, kept)]
        sk = np.sqrt(np.diag(Hk))
        out["kappa"][c] = np.linalg.cond(Hk / np.outer(sk, sk))
    return out


def converge(D, y, theta, lam_tol=1e-26, max_iter=60):
    """the Newton iteration on the explicit kept design D (n, p) with math.fsum sums, on to lambda2 <= lam_tol -> theta, se"""
    D = np.asarray(D, np.float64)
    n, p = D.shape
    theta = np.array(theta, np.float64)
    for _ in range(max_iter):
        eta = np.array([math.fsum(D[i] * theta) for i in range(n)])
        e = np.exp(-np.abs(eta))
        qq = 1.0 / (1.0 + e)
        mu1 = np.where(eta >= 0, qq, e * qq)
        r = np.where(y == 1.0, np.where(eta >= 0, e * qq, qq), -mu1)
        w = e * qq * qq
        g = np.array([math.fsum(r * D[:, j]) for j in range(p)])
        H = np.array([[math.fsum(w * D[:, j] * D[:, k]) for k in range(p)] for j in range(p)])
        delta = np.linalg.solve(H, g)
        theta = theta + delta
        if float(g @ delta) <= lam_tol:
            break
    eta = D @ theta
    e = np.exp(-np.abs(eta))
    w = e / (1.0 + e) ** 2
    H = np.array([[math.fsum(w * D[:, j] * D[:, k]) for k in range(p)] for j in range(p)])
    return theta, np.sqrt(np.diag(np.linalg.inv(H)))


def logit_text(chm, pos, M, W, res, populations):
    """the bytes of query_results.assoc.logistic.tsv from an AncestryAssocLogit-like object"""
    C = len(pos)
    win = AE.windows(C, M, W)
    fmt = lambda v: "nan" if not np.isfinite(v) else format(float(v), ".6g")
    lines = ["\t".join(["chm", "pos", "window", "n", "n_case", "df", "status", "iters", "n_miss", "lrt", "lrt_df", "lrt_p"] +
                       [q + s for q in populations for s in (".n_hap", ".n_alt", ".n_alt_case", ".beta", ".se", ".z", ".p")])]
    for c in range(C):
        cells = [str(chm), str(int(pos[c])), str(int(win[c])), str(int(res.n[c])), str(int(res.n_case[c])), str(int(res.df[c])), str(int(res.status[c])),
                 str(int(res.iters[c])), str(int(res.n_miss[c])), fmt(res.lrt[c]), str(int(res.lrt_df[c])), fmt(res.lrt_p[c])]
        for a in range(len(populations)):
            cells += [str(int(res.n_hap[c, a])), str(int(res.n_alt[c, a])), str(int(res.n_alt_case[c, a])), fmt(res.beta[c, a]), fmt(res.se[c, a]),
                      fmt(res.z[c, a]), fmt(res.p[c, a])]
        lines.append("\t".join(cells))
    return "\n".join(lines) + "\n"
