"""Plain-numpy restatement of the ancestry-specific association model (the Tractor model) of include/gnomix_hip.h
(gnx_ancestry_assoc_stats) and gnomix_amd/assoc.py.  Not a test.

THE MODEL.  X (N, C): 0 REF, 1 ALT, anything else missing; labels (N, W); win(c) = min(c // M, W - 1).  Individual i = rows 2 i, 2 i + 1
with a phenotype y[i], covariates Z[i, :K] (the caller supplies the intercept) and a byte use[i].  Per SNP c and ancestry a, h[i, a] and
d[i, a] are hapcount and dosage of allele_counts_exact.dosage: a missing call carries its label in h and adds nothing to d.
Individual i takes part at window k when use[i] != 0, y[i] and Z[i, :] are finite and both its labels at k lie in [0, A).
At SNP c over the n participants:  y = Z g + sum_{a < A-1} alpha_a h_a + sum_a beta_a d_a + e, ordinary least squares.
Column rule (integers): a hapcount column with sum_i h[i, a] == 0 is dropped; a dosage column with sum_i d[i, a] < min_ac is dropped
and reports NaN.  df = n - p_kept < 1: status 2, NaN.  The kept design rank-deficient: status 1, NaN.  Else status 0 and per (c, a)
beta, se = sqrt(RSS / df * (X^T X)^-1_jj), t = beta / se; n_alt = sum d, n_hap = sum h; per c: n, df, n_miss (missing calls on the
participants' haplotypes), status.

fit() solves every SNP with numpy.linalg.lstsq on the full kept design (no normal equations).  blocks() returns the sufficient
statistics in the layout of the C ABI; blocks_slow() is the literal form (Python ints, math.fsum) for small cases."""
import math

import numpy as np

import allele_counts_exact as AE

RANK_TOL = 2.0 ** -20      # smallest / largest singular value of the column-scaled design at or below this: rank-deficient


def participation(labels, A, y, Z, use):
    """-> (N / 2, W) bool"""
    lab = np.asarray(labels).astype(np.int64)
    y, Z = np.asarray(y, np.float64), np.asarray(Z, np.float64)
    base = np.isfinite(y) & np.isfinite(Z).all(1)
    if use is not None:
        base &= np.asarray(use) != 0
    ok = (lab >= 0) & (lab < A)
    return base[:, None] & ok[0::2] & ok[1::2]


def dosages(X, labels, M, A):
    """-> d, h: (N / 2, C, A) int64 (allele_counts_exact.dosage per ancestry), part (N / 2, C) bool needs participation()"""
    dh = [AE.dosage(X, labels, M, A, a) for a in range(A)]
    return np.stack([v[0] for v in dh], 2).astype(np.int64), np.stack([v[1] for v in dh], 2).astype(np.int64)


def fit(X, labels, M, A, y, Z, use=None, min_ac=1, cols=None):
    """-> dict of beta, se, t (C, A) float64; n_alt, n_hap (C, A) int32; n, df, n_miss, status (C,) int32; kappa (C,) float64 (2-norm
    condition number of the column-scaled kept design, NaN where status != 0); p_kept (C,).  cols: the SNPs to solve (default all);
    the others keep NaN / status -1 but their integer columns are filled."""
    X = np.asarray(X)
    y, Z = np.asarray(y, np.float64), np.asarray(Z, np.float64)
    N, C = X.shape
    W = np.asarray(labels).shape[1]
    K = Z.shape[1]
    win = AE.windows(C, M, W)
    part = participation(labels, A, y, Z, use)[:, win]            # (n_ind, C)
    d, h = dosages(X, labels, M, A)
    d, h = d * part[:, :, None], h * part[:, :, None]
    Xi = X.astype(np.int64)
    missing = ~((Xi == 0) | (Xi == 1))
    out = dict(beta=np.full((C, A), np.nan), se=np.full((C, A), np.nan), t=np.full((C, A), np.nan), kappa=np.full(C, np.nan),
               n_alt=d.sum(0).astype(np.int32), n_hap=h.sum(0).astype(np.int32), n=part.sum(0).astype(np.int32),
               n_miss=((missing[0::2].astype(np.int64) + missing[1::2]) * part).sum(0).astype(np.int32),
               df=np.zeros(C, np.int32), status=np.full(C, -1, np.int32), p_kept=np.zeros(C, np.int32))
    for c in range(C):
        keep_h = out["n_hap"][c, :A - 1] > 0
        keep_d = out["n_alt"][c] >= min_ac
        p = K + int(keep_h.sum()) + int(keep_d.sum())
        out["p_kept"][c] = p
        out["df"][c] = out["n"][c] - p
        if cols is not None and c not in cols:
            continue
        if out["df"][c] < 1:
            out["status"][c] = 2
            continue
        r = part[:, c]
        D = np.concatenate([Z[r], h[r, c, :A - 1][:, keep_h].astype(np.float64), d[r, c][:, keep_d].astype(np.float64)], 1)
        yy = y[r]
        s = np.sqrt((D * D).sum(0))
        if (s == 0).any():
            out["status"][c] = 1
            continue
        U, S, Vt = np.linalg.svd(D / s, full_matrices=False)
        if S[-1] <= RANK_TOL * S[0]:
            out["status"][c] = 1
            continue
        out["status"][c] = 0
        out["kappa"][c] = S[0] / S[-1]
        coef = np.linalg.lstsq(D, yy, rcond=None)[0]
        res = yy - D @ coef
        rss = float(res @ res)
        cov = ((Vt / S[:, None]) ** 2).sum(0) / (s * s)
        se = np.sqrt(rss / out["df"][c] * cov)
        j = p - int(keep_d.sum())
        out["beta"][c, keep_d] = coef[j:]
        out["se"][c, keep_d] = se[j:]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["t"][c, keep_d] = coef[j:] / se[j:]
    return out


def _layout(A, K):
    nDD, nDH = A * (A + 1) // 2, A * (A - 1)
    return nDD, nDH, nDD + nDH + A + 1


def _prepared(X, labels, M, A, y, Z, use):
    X = np.asarray(X)
    y, Z = np.asarray(y, np.float64), np.asarray(Z, np.float64)
    lab = np.asarray(labels).astype(np.int64)
    C, W = X.shape[1], lab.shape[1]
    win = AE.windows(C, M, W)
    partw = participation(labels, A, y, Z, use)
    d, h = dosages(X, labels, M, A)
    Xi = X.astype(np.int64)
    missing = ~((Xi == 0) | (Xi == 1))
    miss2 = missing[0::2].astype(np.int64) + missing[1::2]
    return y, Z, lab, win, partw, d, h, miss2


def blocks_slow(X, labels, M, A, y, Z, use, c0, c1):
    """the four arrays of gnx_ancestry_assoc_stats for the SNPs [c0, c1) and n_bad: integers with Python ints, float64 sums with
    math.fsum (correctly rounded: equal to ANY summation order whenever every partial sum is exact, as for small integer-valued y, Z)"""
    y, Z, lab, win, partw, d, h, miss2 = _prepared(X, labels, M, A, y, Z, use)
    K = Z.shape[1]
    nDD, nDH, NI = _layout(A, K)
    n_ind = len(y)
    w0, w1 = int(win[c0]), int(win[c1 - 1])
    snp_f = np.zeros((c1 - c0, A, K + 1))
    snp_i = np.zeros((c1 - c0, NI), np.int32)
    zy = np.concatenate([Z, y[:, None]], 1)
    for c in range(c0, c1):
        ids = [i for i in range(n_ind) if partw[i, win[c]]]
        dc = [[int(d[i, c, a]) for a in range(A)] for i in ids]
        hc = [[int(h[i, c, a]) for a in range(A)] for i in ids]
        row = []
        for a in range(A):
            for b in range(a, A):
                row.append(sum(r[a] * r[b] for r in dc))
        for a in range(A):
            for b in range(A - 1):
                row.append(sum(r[a] * g[b] for r, g in zip(dc, hc)))
        for a in range(A):
            row.append(sum(r[a] for r in dc))
        row.append(sum(int(miss2[i, c]) for i in ids))
        snp_i[c - c0] = row
        for a in range(A):
            for k in range(K + 1):
                snp_f[c - c0, a, k] = math.fsum(r[a] * float(zy[i, k]) for r, i in zip(dc, ids))
    P1 = K + A
    win_f = np.zeros((w1 - w0 + 1, P1, P1))
    win_i = np.zeros((w1 - w0 + 1, 1 + A), np.int32)
    for w in range(w0, w1 + 1):
        ids = [i for i in range(n_ind) if partw[i, w]]
        hw = [[int(lab[2 * i, w] == a) + int(lab[2 * i + 1, w] == a) for a in range(A)] for i in ids]
        U = [[float(v) for v in Z[i]] + [float(v) for v in g[:A - 1]] + [float(y[i])] for i, g in zip(ids, hw)]
        for p in range(P1):
            for q in range(P1):
                win_f[w - w0, p, q] = math.fsum(u[p] * u[q] for u in U)
        win_i[w - w0] = [len(ids)] + [sum(g[a] for g in hw) for a in range(A)]
    n_bad = int(((lab[:, w0:w1 + 1] < 0) | (lab[:, w0:w1 + 1] >= A)).sum())
    return snp_f.reshape(c1 - c0, -1), snp_i, win_f.reshape(w1 - w0 + 1, -1), win_i, n_bad


def blocks(X, labels, M, A, y, Z, use, c0, c1):
    """the same as blocks_slow for integer-valued y and Z (non-finite values allowed on individuals, which then take no part), by
    float64 matrix products of integers: every product and every partial sum is an integer below 2^53 (asserted), hence exact in any
    order and equal to the Python-int / math.fsum form."""
    y, Z, lab, win, partw, d, h, miss2 = _prepared(X, labels, M, A, y, Z, use)
    K = Z.shape[1]
    nDD, nDH, NI = _layout(A, K)
    n_ind = len(y)
    fin = np.isfinite(y) & np.isfinite(Z).all(1)
    zy = np.where(fin[:, None], np.concatenate([Z, y[:, None]], 1), 0.0)          # rows that never take part: any finite value
    assert np.array_equal(zy, np.round(zy)), "blocks(): y and Z must be integer-valued (use blocks_slow)"
    big = float(np.abs(zy).max()) if zy.size else 0.0
    assert 4.0 * n_ind * max(big, 2.0) ** 2 < 2.0 ** 53
    w0, w1 = int(win[c0]), int(win[c1 - 1])
    nc = c1 - c0
    pc = partw[:, win[c0:c1]]                                                     # (n_ind, nc)
    dc = (d[:, c0:c1] * pc[:, :, None]).transpose(1, 0, 2).astype(np.float64)     # (nc, n_ind, A)
    hc = (h[:, c0:c1] * pc[:, :, None]).transpose(1, 0, 2).astype(np.float64)
    dT = dc.transpose(0, 2, 1)
    DD = np.matmul(dT, dc)
    DH = np.matmul(dT, hc[:, :, :A - 1])
    DZ = np.matmul(dT, zy[None])                                                  # (nc, A, K + 1)
    iu = np.triu_indices(A)
    snp_i = np.concatenate([DD[:, iu[0], iu[1]], DH.reshape(nc, -1), dc.sum(1), (miss2[:, c0:c1] * pc).sum(0)[:, None]], 1)
    assert snp_i.shape[1] == NI
    P1 = K + A
    win_f = np.zeros((w1 - w0 + 1, P1, P1))
    win_i = np.zeros((w1 - w0 + 1, 1 + A), np.int32)
    for w in range(w0, w1 + 1):
        r = partw[:, w]
        hw = np.stack([(lab[0::2, w] == a).astype(np.float64) + (lab[1::2, w] == a) for a in range(A)], 1)[r]
        U = np.concatenate([zy[r, :K], hw[:, :A - 1], zy[r, K:]], 1)
        win_f[w - w0] = U.T @ U
        win_i[w - w0, 0] = r.sum()
        win_i[w - w0, 1:] = hw.sum(0)
    n_bad = int(((lab[:, w0:w1 + 1] < 0) | (lab[:, w0:w1 + 1] >= A)).sum())
    return DZ.reshape(nc, -1), snp_i.astype(np.int32), win_f.reshape(w1 - w0 + 1, -1), win_i, n_bad


def assoc_text(chm, pos, M, W, res, p, populations):
    """the bytes of query_results.assoc.tsv: chm pos window n df status n_miss, then <pop>.n_hap .n_alt .beta .se .t .p per population;
    floats as %.6g, NaN as 'nan'"""
    C = len(pos)
    win = AE.windows(C, M, W)
    fmt = lambda v: "nan" if not np.isfinite(v) else format(float(v), ".6g")
    lines = ["\t".join(["chm", "pos", "window", "n", "df", "status", "n_miss"] +
                       [q + s for q in populations for s in (".n_hap", ".n_alt", ".beta", ".se", ".t", ".p")])]
    for c in range(C):
        cells = [str(chm), str(int(pos[c])), str(int(win[c])), str(int(res["n"][c])), str(int(res["df"][c])), str(int(res["status"][c])),
                 str(int(res["n_miss"][c]))]
        for a in range(len(populations)):
            cells += [str(int(res["n_hap"][c, a])), str(int(res["n_alt"][c, a])), fmt(res["beta"][c, a]), fmt(res["se"][c, a]), fmt(res["t"][c, a]),
                      fmt(p[c, a])]
        lines.append("\t".join(cells))
    return "\n".join(lines) + "\n"


def float_blocks_in_order(X, labels, M, A, y, Z, use, c0, c1):
    """snp_f64 and win_f64 of [c0, c1) for ANY finite y and Z, summed as the contract states: over the individuals in ascending i, one
    product per individual rounded once and then added to the running sum (numpy float64 elementwise: no fused multiply-add).  The
    device's float blocks must equal these bit for bit."""
    y, Z, lab, win, partw, d, h, miss2 = _prepared(X, labels, M, A, y, Z, use)
    K = Z.shape[1]
    zy = np.concatenate([Z, y[:, None]], 1)
    w0, w1 = int(win[c0]), int(win[c1 - 1])
    snp_f = np.zeros((c1 - c0, A, K + 1))
    win_f = np.zeros((w1 - w0 + 1, K + A, K + A))
    for i in range(len(y)):
        pc = partw[i, win[c0:c1]]
        if pc.any():
            term = d[i, c0:c1].astype(np.float64)[:, :, None] * zy[i][None, None, :]
            snp_f[pc] = snp_f[pc] + term[pc]
        for w in range(w0, w1 + 1):
            if partw[i, w]:
                hw = [float(int(lab[2 * i, w] == a) + int(lab[2 * i + 1, w] == a)) for a in range(A - 1)]
                u = np.concatenate([Z[i], hw, y[i:i + 1]])
                win_f[w - w0] = win_f[w - w0] + u[:, None] * u[None, :]
    return snp_f.reshape(c1 - c0, -1), win_f.reshape(w1 - w0 + 1, -1)
