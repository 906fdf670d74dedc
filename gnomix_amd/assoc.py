"""Ancestry-specific association (the Tractor model) from the device's sufficient statistics (gnx_ancestry_assoc_stats,
include/gnomix_hip.h states the model and the blocks).  The device reduces X and the labels to per-SNP and
per-window blocks; this module assembles the normal equations of the kept columns, factors them (a batched Cholesky, numpy float64)
and returns beta, se, t and p per (SNP, ancestry).  scipy is imported here only, and only for the p-values."""
import collections

import numpy as np

STATS_CHUNK_BYTES = 64 << 20      # the statistics of one chunk of SNPs (the blocks that leave the device per call) stay below this
FINISH_CHUNK_BYTES = 64 << 20     # ... and so do the assembled normal matrices of one batched factorisation
PIVOT_MIN = 2.0 ** -40            # a pivot of the unit-diagonal normal matrix at or below this: not positive definite (status 1)

AncestryAssoc = collections.namedtuple("AncestryAssoc", "beta se t p n_alt n_hap n df n_miss status")
AncestryAssoc.__doc__ = """what ancestry_assoc returns.  beta, se, t, p: (C, A) float64, NaN for a dropped dosage term and for a SNP with status != 0;
n_alt = sum d, n_hap = sum h: (C, A) int32; n, df, n_miss, status: (C,) int32 (status 0 fitted, 1 not positive definite, 2 df < 1)"""

AncestryAssocLogit = collections.namedtuple("AncestryAssocLogit", "beta se z p lrt lrt_df lrt_p n_alt n_alt_case n_hap n n_case df n_miss iters status")
AncestryAssocLogit.__doc__ = """what ancestry_assoc_logit returns (the logistic Tractor model of gnx_ancestry_assoc_logit, fitted on the device).  beta, se,
z = beta / se, p (two-sided normal): (C, A) float64, NaN for a dropped dosage term and for a SNP with status != 0; lrt = dev0[window] - dev
(the null model is fitted on the same participants: the joint test of the SNP's kept dosage terms), lrt_df = the number of kept dosage
terms, lrt_p = chi2.sf(lrt, lrt_df): (C,); n_alt, n_alt_case, n_hap: (C, A) int32; n, n_case, df, n_miss, iters, status: (C,) int32 (status
0 fitted, 1 not positive definite, 2 df < 1, 3 no finite optimum, 4 the window's null model failed)"""

LogitFit = collections.namedtuple("LogitFit", "beta se dev theta n_alt n_alt_case n_miss iters status theta0 dev0 n n_case sum_h iters0 status0 window n_bad")
LogitFit.__doc__ = """the raw outputs of gnx_ancestry_assoc_logit for SNPs [c0, c1): beta, se (nc, A), dev (nc,), theta (nc, Q) or None; n_alt,
n_alt_case (nc, A), n_miss, iters, status (nc,) int32; per window of the range theta0 (nw, P), dev0 (nw,), n, n_case (nw,), sum_h (nw, A), iters0,
status0 (nw,); window (nc,): the row of the window arrays a SNP uses; n_bad: labels outside [0, A)"""

LOGIT_TOL, LOGIT_MAX_ITER, LOGIT_MAX_Q = 1e-10, 25, 47     # GNX_ASSOC_LOGIT_TOL / _MAX_ITER / _MAX_Q of include/gnomix_hip.h

AssocStats = collections.namedtuple("AssocStats", "dtz dty dtd dth sum_d n_miss gram n sum_h window n_bad")
AssocStats.__doc__ = """the raw blocks of SNPs [c0, c1): dtz (nc, A, K), dty (nc, A) float64; dtd (nc, A (A + 1) / 2), dth (nc, A, A - 1), sum_d (nc, A),
n_miss (nc,) int32; per window of the range: gram (nw, K + A, K + A) float64 of [Z, h_0 .. h_{A-2}, y], n (nw,), sum_h (nw, A) int32;
window (nc,): the row of the window blocks a SNP uses; n_bad: labels outside [0, A)"""


def layout(A, K):
    """sizes of the blocks: NF float64 and NI int32 per SNP, NWF float64 and NWI int32 per window"""
    return A * (K + 1), A * (A + 1) // 2 + A * (A - 1) + A + 1, (K + A) ** 2, 1 + A


def snps_per_chunk(A, K, max_bytes=STATS_CHUNK_BYTES):
    NF, NI, _, _ = layout(A, K)
    return max(1, max_bytes // (NF * 8 + NI * 4))


def window_span(c0, c1, M, W):
    """the number of windows the SNPs [c0, c1) touch (the window of SNP c is min(c // M, W - 1)); 1 for a range that is empty or not valid"""
    return int(min((c1 - 1) // M, W - 1) - min(c0 // M, W - 1) + 1) if 0 <= c0 < c1 and M >= 1 else 1


def stats_buffers(A, K, c0, c1, M, W, empty=None):
    """zeroed (or empty(shape, dtype)) arrays of one call, in the order of the C ABI: snp_f64, snp_i32, win_f64, win_i32"""
    NF, NI, NWF, NWI = layout(A, K)
    nc, nw = max(c1 - c0, 0), window_span(c0, c1, M, W)
    new = empty or (lambda shape, dtype: np.zeros(shape, dtype))
    return new((nc, NF), np.float64), new((nc, NI), np.int32), new((nw, NWF), np.float64), new((nw, NWI), np.int32)


def split_blocks(snp_f, snp_i, win_f, win_i, A, K, c0, c1, M, W, n_bad=0):
    """the four arrays of the C ABI -> AssocStats (views)"""
    nc = c1 - c0
    nDD, nDH = A * (A + 1) // 2, A * (A - 1)
    snp_f = snp_f.reshape(nc, A, K + 1)
    snp_i = snp_i.reshape(nc, -1)
    w = np.minimum(np.arange(c0, c1) // M, W - 1)
    nw = int(w[-1] - w[0] + 1)
    win_i = win_i.reshape(nw, 1 + A)
    return AssocStats(snp_f[:, :, :K], snp_f[:, :, K], snp_i[:, :nDD], snp_i[:, nDD:nDD + nDH].reshape(nc, A, A - 1), snp_i[:, nDD + nDH:nDD + nDH + A],
                      snp_i[:, nDD + nDH + A], win_f.reshape(nw, K + A, K + A), win_i[:, 0], win_i[:, 1:], w - w[0], int(n_bad))


def _cholesky_batched(G):
    """G (B, Q, Q) symmetric with unit diagonal -> L (lower, B, Q, Q), bad (B,): a pivot <= PIVOT_MIN (or not finite) was met"""
    B, Q, _ = G.shape
    L = np.zeros_like(G)
    bad = np.zeros(B, bool)
    for j in range(Q):
        piv = G[:, j, j] - np.einsum("bk,bk->b", L[:, j, :j], L[:, j, :j])
        bad |= ~(piv > PIVOT_MIN)
        piv = np.where(piv > PIVOT_MIN, piv, 1.0)
        d = np.sqrt(piv)
        L[:, j, j] = d
        if j + 1 < Q:
            L[:, j + 1:, j] = (G[:, j + 1:, j] - np.einsum("bik,bk->bi", L[:, j + 1:, :j], L[:, j, :j])) / d[:, None]
    return L, bad


def _lower_inverse_batched(L):
    B, Q, _ = L.shape
    Li = np.zeros_like(L)
    for j in range(Q):       # row j of L^-1: (e_j - L[j, :j] Li[:j]) / L[j, j]
        Li[:, j, :] = -np.einsum("bk,bkq->bq", L[:, j, :j], Li[:, :j, :])
        Li[:, j, j] += 1.0
        Li[:, j, :] /= L[:, j, j][:, None]
    return Li


def _factor_chunk(st, sl, A, K, min_ac):
    """the trait-independent half of a chunk's finish: the kept columns, the unit-diagonal normal matrix of every SNP and its Cholesky
    factor -> w, keep (nc, Q), n, df (int64), s (the column scales), Li (L^-1, (nc, Q, Q)), bad (nc,)"""
    P, Q = K + A - 1, K + 2 * A - 1
    w = st.window[sl]
    nc = len(w)
    gram = st.gram[w]                                  # (nc, P + 1, P + 1)
    G = np.zeros((nc, Q, Q))
    G[:, :P, :P] = gram[:, :P, :P]
    G[:, P:, :K] = st.dtz[sl]
    G[:, P:, K:P] = st.dth[sl]
    G[:, :P, P:] = np.transpose(G[:, P:, :P], (0, 2, 1))
    iu = np.triu_indices(A)
    DD = np.zeros((nc, A, A))
    DD[:, iu[0], iu[1]] = st.dtd[sl]
    DD[:, iu[1], iu[0]] = st.dtd[sl]
    G[:, P:, P:] = DD
    keep = np.ones((nc, Q), bool)
    keep[:, K:P] = st.sum_h[w][:, :A - 1] > 0
    keep[:, P:] = st.sum_d[sl] >= min_ac
    n = st.n[w].astype(np.int64)
    df = n - keep.sum(1)
    # a dropped column becomes a unit row / column with a zero right-hand side: one batch shape for every SNP
    kk = keep[:, :, None] & keep[:, None, :]
    G = np.where(kk, G, 0.0)
    diag = np.einsum("bqq->bq", G)
    s = np.sqrt(np.where(keep & (diag > 0), diag, 1.0))
    zero_col = keep & ~(diag > 0)                       # a kept column of zeros (a covariate): never positive definite
    Gs = G / (s[:, :, None] * s[:, None, :])
    Gs[:, np.arange(Q), np.arange(Q)] = np.where(keep & (diag > 0), 1.0, np.where(keep, 0.0, 1.0))
    L, bad = _cholesky_batched(Gs)
    bad |= zero_col.any(1)
    return w, keep, n, df, s, _lower_inverse_batched(L), bad


def _finish_chunk(st, sl, A, K, min_ac):
    P, Q = K + A - 1, K + 2 * A - 1
    w, keep, n, df, s, Li, bad = _factor_chunk(st, sl, A, K, min_ac)
    gram = st.gram[w]
    b = np.zeros((len(w), Q))
    b[:, :P] = gram[:, :P, P]
    yty = gram[:, P, P]
    b[:, P:] = st.dty[sl]
    b = np.where(keep, b, 0.0)
    inv = np.einsum("bkq,bkr->bqr", Li, Li)
    beta_s = np.einsum("bqr,br->bq", inv, b / s)
    beta = beta_s / s
    rss = np.maximum(yty - np.einsum("bq,bq->b", b, beta), 0.0)
    status = np.where(df < 1, 2, np.where(bad, 1, 0)).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = rss / df
        se = np.sqrt(s2[:, None] * np.einsum("bqq->bq", inv)) / s
        tt = beta / se
    dead = (status != 0)[:, None] | ~keep
    beta, se, tt = (np.where(dead, np.nan, v)[:, P:] for v in (beta, se, tt))
    return beta, se, tt, n.astype(np.int32), df.astype(np.int32), status


def finish(st, A, K, min_ac=1, max_bytes=FINISH_CHUNK_BYTES):
    """AssocStats of a range of SNPs -> (beta, se, t, n_alt, n_hap, n, df, n_miss, status) of that range"""
    if min_ac < 1:
        raise ValueError("min_ac must be >= 1")
    nc = len(st.window)
    Q = K + 2 * A - 1
    step = max(1, max_bytes // (Q * Q * 8 * 6))
    parts = [_finish_chunk(st, slice(i, min(i + step, nc)), A, K, min_ac) for i in range(0, nc, step)]
    beta, se, tt, n, df, status = (np.concatenate([p[i] for p in parts]) for i in range(6))
    return beta, se, tt, np.asarray(st.sum_d, np.int32).copy(), np.asarray(st.sum_h[st.window], np.int32), n, df, np.asarray(st.n_miss, np.int32).copy(), status


def p_values(t, df):
    """two-sided p of t with df degrees of freedom ((C, A) and (C,)); NaN where t is"""
    from scipy import stats
    with np.errstate(invalid="ignore"):
        return 2.0 * stats.t.sf(np.abs(t), np.maximum(df, 1)[:, None].astype(np.float64))


def assoc_from_stats(stats_fn, C, A, K, min_ac=1):
    """stats_fn(c0, c1) -> AssocStats; walks the SNPs in chunks of snps_per_chunk(A, K) and finishes each -> AncestryAssoc.  A
    GNX_EINVAL for labels out of range is stats_fn's to raise."""
    step = snps_per_chunk(A, K)
    parts = [finish(stats_fn(c0, min(c0 + step, C)), A, K, min_ac) for c0 in range(0, C, step)]
    beta, se, tt, n_alt, n_hap, n, df, n_miss, status = (np.concatenate([p[i] for p in parts]) for i in range(9))
    return AncestryAssoc(beta, se, tt, p_values(tt, df), n_alt, n_hap, n, df, n_miss, status)


AncestryAssocTraits = collections.namedtuple("AncestryAssocTraits", "beta se t p n_alt n_hap n df n_miss status")
AncestryAssocTraits.__doc__ = """what ancestry_assoc_traits returns for T quantitative traits.  beta, se, t, p: (C, A, T) float64, NaN for a dropped
dosage term and for a SNP with status != 0; the integer fields and status do not depend on the trait and are shaped as in AncestryAssoc:
n_alt, n_hap (C, A) int32; n, df, n_miss, status (C,) int32"""

TraitStats = collections.namedtuple("TraitStats", "dty ry yty window n_bad")
TraitStats.__doc__ = """the trait-dependent blocks of SNPs [c0, c1) (gnx_ancestry_assoc_traits): dty (nc, A, T) = D^T Y; per window of the range ry
(nw, K + A - 1, T) = [Z, h_0 .. h_{A-2}]^T Y and yty (nw, T) = diag(Y^T Y); window (nc,): the row of the window blocks a SNP uses;
n_bad: labels outside [0, A).  Views of the padded arrays of the C ABI (their last axis is T rounded up to a multiple of 16)."""

MAX_T = 65536                     # GNX_ASSOC_MAX_T of include/gnomix_hip.h
TRAITS_MAX_BYTES = 2 << 30        # what ancestry_assoc_traits agrees to concatenate by default


def trait_ldt(T):
    return (int(T) + 15) // 16 * 16


def trait_buffers(A, K, T, c0, c1, M, W, empty=None):
    """zeroed (or empty(shape, dtype)) arrays of one call, in the order of the C ABI: snp_y, win_y, win_yy"""
    ldt = trait_ldt(T)
    nc, nw = max(c1 - c0, 0), window_span(c0, c1, M, W)
    new = empty or (lambda shape, dtype: np.zeros(shape, dtype))
    return new((nc, A, ldt), np.float64), new((nw, K + A - 1, ldt), np.float64), new((nw, ldt), np.float64)


def split_traits(sy, wy, wyy, T, c0, c1, M, W, n_bad=0):
    """the three arrays of the C ABI -> TraitStats (views)"""
    w = np.minimum(np.arange(c0, c1) // M, W - 1)
    return TraitStats(sy[:, :, :T], wy[:, :, :T], wyy[:, :T], w - w[0], int(n_bad))


def trait_covariates(n_ind, Y, Z=None, use=None):
    """Y (n_ind, T), Z (n_ind, K) or None (the intercept only), use (n_ind,) or None -> contiguous float64 / float64 / uint8 arrays and
    use2 = use & (every entry of Y[i, :] finite): the participation byte of the trait-independent blocks (complete cases across the
    batch of traits; traits with different missingness patterns go in separate calls)"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[0] != n_ind or Y.shape[1] < 1:
        raise ValueError(f"Y must be (n_ind={n_ind}, T >= 1), got {Y.shape}")
    if Y.shape[1] > MAX_T:
        raise ValueError(f"at most {MAX_T} traits per call, got {Y.shape[1]}")
    _, Z, use = covariates(n_ind, np.zeros(n_ind), Z, use)
    use2 = np.ascontiguousarray(use & np.isfinite(Y).all(1), dtype=np.uint8)
    return Y, Z, use, use2


def traits_snps_per_chunk(A, K, T, max_bytes=STATS_CHUNK_BYTES):
    """SNPs per chunk such that the device blocks of the chunk (both entries) and its four (nc, A, T) float64 results each stay below
    max_bytes"""
    NF, NI, _, _ = layout(A, K)
    return max(1, max_bytes // max(NF * 8 + NI * 4 + A * trait_ldt(T) * 8, 4 * A * T * 8))


def traits_result_bytes(C, A, T):
    """bytes of an AncestryAssocTraits of C SNPs"""
    return C * (4 * A * T * 8 + 2 * A * 4 + 4 * 4)


def _finish_traits_chunk(st, ts, sl, A, K, min_ac):
    P, Q = K + A - 1, K + 2 * A - 1
    w, keep, n, df, s, Li, bad = _factor_chunk(st, sl, A, K, min_ac)     # one factorisation per SNP, whatever T
    nc, T = len(w), ts.dty.shape[2]
    b = np.empty((nc, Q, T))
    b[:, :P] = ts.ry[w]
    b[:, P:] = ts.dty[sl]
    b = np.where(keep[:, :, None], b, 0.0)
    v = np.matmul(Li, b / s[:, :, None])                                 # L v = b / s, then L^T beta_s = v: two triangular products
    beta = np.matmul(np.transpose(Li, (0, 2, 1)), v) / s[:, :, None]
    rss = np.maximum(ts.yty[w] - np.einsum("bqt,bqt->bt", b, beta), 0.0)
    status = np.where(df < 1, 2, np.where(bad, 1, 0)).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = rss / df[:, None]
        se = np.sqrt(s2[:, None, :] * np.einsum("bkq,bkq->bq", Li, Li)[:, :, None]) / s[:, :, None]
        tt = beta / se
    dead = ((status != 0)[:, None] | ~keep)[:, :, None]
    beta, se, tt = (np.where(dead, np.nan, x)[:, P:] for x in (beta, se, tt))
    return beta, se, tt, n.astype(np.int32), df.astype(np.int32), status


def finish_traits(st, ts, A, K, min_ac=1, max_bytes=FINISH_CHUNK_BYTES):
    """AssocStats (the trait-independent blocks: gnx_ancestry_assoc_stats under the traits' participation, its phenotype ignored) and
    TraitStats of the same range of SNPs -> (beta, se, t (nc, A, T), n_alt, n_hap, n, df, n_miss, status): per chunk of SNPs the normal
    matrix is assembled and factored ONCE, all T right-hand sides are solved with batched triangular products, RSS_t = Y^T Y_t - b_t^T beta_t"""
    if min_ac < 1:
        raise ValueError("min_ac must be >= 1")
    nc = len(st.window)
    Q, T = K + 2 * A - 1, ts.dty.shape[2]
    step = max(1, max_bytes // (Q * Q * 8 * 6 + Q * T * 8 * 4))
    parts = [_finish_traits_chunk(st, ts, slice(i, min(i + step, nc)), A, K, min_ac) for i in range(0, nc, step)]
    beta, se, tt, n, df, status = (np.concatenate([p[i] for p in parts]) for i in range(6))
    return beta, se, tt, np.asarray(st.sum_d, np.int32).copy(), np.asarray(st.sum_h[st.window], np.int32), n, df, np.asarray(st.n_miss, np.int32).copy(), status


def p_values_traits(t, df):
    """two-sided p of t (C, A, T) with df (C,) degrees of freedom; NaN where t is"""
    from scipy import stats
    with np.errstate(invalid="ignore"):
        return 2.0 * stats.t.sf(np.abs(t), np.maximum(df, 1)[:, None, None].astype(np.float64))


def traits_chunks(blocks_fn, C, A, K, T, min_ac=1, p_max=None, chunk_bytes=None):
    """blocks_fn(c0, c1) -> (AssocStats, TraitStats); a generator of (c0, c1, AncestryAssocTraits) per chunk of
    traits_snps_per_chunk(A, K, T, chunk_bytes) SNPs.  p_max: the float results of every (SNP, ancestry, trait) whose p is not <= p_max
    are set to NaN (what remains is the list of hits)."""
    step = traits_snps_per_chunk(A, K, T, STATS_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes))
    for c0 in range(0, C, step):
        c1 = min(c0 + step, C)
        st, ts = blocks_fn(c0, c1)
        beta, se, tt, n_alt, n_hap, n, df, n_miss, status = finish_traits(st, ts, A, K, min_ac)
        p = p_values_traits(tt, df)
        if p_max is not None:
            with np.errstate(invalid="ignore"):
                drop = ~(p <= p_max)
            beta, se, tt, p = (np.where(drop, np.nan, x) for x in (beta, se, tt, p))
        yield c0, c1, AncestryAssocTraits(beta, se, tt, p, n_alt, n_hap, n, df, n_miss, status)


def traits_concat(chunks, C, A, T, max_bytes=TRAITS_MAX_BYTES):
    """the chunks of traits_chunks -> one AncestryAssocTraits; ValueError before any work when it would exceed max_bytes"""
    need = traits_result_bytes(C, A, T)
    if max_bytes is not None and need > max_bytes:
        raise ValueError(f"the result of {C} SNPs x {A} ancestries x {T} traits takes {need} bytes, above max_bytes = {max_bytes}: "
                         "walk ancestry_assoc_traits_chunks instead, or pass fewer traits")
    parts = [r for _, _, r in chunks]
    return AncestryAssocTraits(*(np.concatenate([getattr(r, f) for r in parts]) for f in AncestryAssocTraits._fields))


def traits_host(ctx, X, labels, M, A, Y, Z, use, c0, c1, min_ac=1, check=True):
    """gnx_ancestry_assoc_traits on host arrays: X (N, C) int8 (any row stride), labels (N, W) int32, Y (N / 2, T) -> TraitStats of [c0, c1)"""
    from . import ancestry_ops as ops
    return ops.assoc_traits(ops.host_front(ctx, X, labels, M, A, strided=True), Y, Z, use, c0, c1, min_ac, check)


def read_table(path, samples, what="trait"):
    """a TSV with the header `sample<TAB>name...` matched to `samples` by name, as read_phenotypes matches -> (values (n, len(names))
    float64, present (n,) bool, names).  A query sample the file lacks has present = False and NaN values; a cell that is empty, NA, NaN
    or '.' is NaN; file samples the query lacks are ignored; a sample listed twice is an error."""
    with open(path) as f:
        lines = [ln.rstrip("\n").rstrip("\r") for ln in f if ln.strip()]
    if not lines:
        raise ValueError(f"{path}: empty {what} file")
    head = lines[0].split("\t")
    if len(head) < 2 or head[0] != "sample":
        raise ValueError(f"{path}: the header must be 'sample<TAB>name...', got {head[:2]}")
    names = head[1:]
    if len(set(names)) != len(names):
        raise ValueError(f"{path}: a {what} name is listed twice in the header")

    def num(cell):
        cell = cell.strip()
        if cell == "" or cell.upper() in ("NA", "NAN", "."):
            return np.nan
        try:
            return float(cell)
        except ValueError:
            raise ValueError(f"{path}: '{cell}' is not a number") from None

    rows = {}
    for ln in lines[1:]:
        cells = ln.split("\t")
        if len(cells) != len(head):
            raise ValueError(f"{path}: a line has {len(cells)} cells, the header {len(head)}")
        if cells[0] in rows:
            raise ValueError(f"{path}: sample '{cells[0]}' is listed twice")
        rows[cells[0]] = [num(c) for c in cells[1:]]
    vals = np.full((len(samples), len(names)), np.nan)
    present = np.zeros(len(samples), bool)
    for i, name in enumerate(samples):
        r = rows.get(str(name))
        if r is not None:
            vals[i] = r
            present[i] = True
    return vals, present, names


def read_traits(trait_file, samples, covariate_file=None):
    """inference.trait_file (header `sample<TAB>name...`, one column per trait) and the optional inference.covariate_file (header
    `sample<TAB>cov...`) -> (Y (n, T), Z (n, 1 + covariates) with the intercept in front, use (n,) uint8, trait names, covariate names).
    A sample absent from the trait file (or, where one is given, from the covariate file) has use = 0.  NA cells stay NaN: the model's
    participation rule (complete cases across the traits, finite covariates) drops those individuals."""
    Y, present, names = read_table(trait_file, samples, "trait")
    n = len(samples)
    Z = np.ones((n, 1))
    cov_names = []
    if covariate_file:
        cov, cpresent, cov_names = read_table(covariate_file, samples, "covariate")
        Z = np.concatenate([Z, cov], 1)
        present = present & cpresent
    return Y, Z, present.astype(np.uint8), names, ["intercept"] + cov_names


def logit_layout(A, K):
    """columns of snp_f64, snp_i32, theta, win_f64, win_i32 of gnx_ancestry_assoc_logit"""
    return 2 * A + 1, 2 * A + 3, K + 2 * A - 1, K + A, A + 4


def logit_snps_per_chunk(A, K, max_bytes=STATS_CHUNK_BYTES):
    SF, SI, Q, _, _ = logit_layout(A, K)
    return max(1, max_bytes // ((SF + Q) * 8 + SI * 4))


def logit_buffers(A, K, c0, c1, M, W, want_theta=True, empty=None):
    """zeroed (or empty(shape, dtype)) arrays of one call, in the order of the C ABI: snp_f64, snp_i32, theta or None, win_f64, win_i32"""
    SF, SI, Q, WF, WI = logit_layout(A, K)
    nc, nw = max(c1 - c0, 0), window_span(c0, c1, M, W)
    new = empty or (lambda shape, dtype: np.zeros(shape, dtype))
    return new((nc, SF), np.float64), new((nc, SI), np.int32), new((nc, Q), np.float64) if want_theta else None, new((nw, WF), np.float64), new((nw, WI), np.int32)


def split_logit(sf, si, th, wf, wi, A, K, c0, c1, M, W, n_bad=0):
    """the arrays of the C ABI -> LogitFit (views)"""
    w = np.minimum(np.arange(c0, c1) // M, W - 1)
    P = K + A - 1
    return LogitFit(sf[:, :A], sf[:, A:2 * A], sf[:, 2 * A], th, si[:, :A], si[:, A:2 * A], si[:, 2 * A], si[:, 2 * A + 1], si[:, 2 * A + 2],
                    wf[:, :P], wf[:, P], wi[:, 0], wi[:, 1], wi[:, 2:2 + A], wi[:, 2 + A], wi[:, 3 + A], w - w[0], int(n_bad))


def logit_p_values(beta, se, lrt, lrt_df):
    """-> z, p (two-sided normal), lrt_p (chi-square with lrt_df degrees of freedom; NaN where lrt is or lrt_df is 0)"""
    from scipy import stats
    with np.errstate(divide="ignore", invalid="ignore"):
        z = beta / se
        p = 2.0 * stats.norm.sf(np.abs(z))
        lrt_p = np.where(lrt_df > 0, stats.chi2.sf(lrt, np.maximum(lrt_df, 1)), np.nan)
    return z, p, lrt_p


def finish_logit(fit, K):
    """one LogitFit -> the columns of AncestryAssocLogit but z, p and lrt_p (added once over all chunks)"""
    w = fit.window
    A = fit.beta.shape[1]
    kept_d = ~np.isnan(fit.beta) if len(fit.beta) else np.zeros((0, A), bool)
    ok = fit.status == 0
    lrt = np.where(ok, fit.dev0[w] - fit.dev, np.nan)
    lrt_df = np.where(ok, kept_d.sum(1), 0).astype(np.int32)
    n = fit.n[w].astype(np.int32)
    # p_kept of the column rule: the covariates, the hapcount columns with a positive sum, the kept dosage columns (known where the SNP
    # was fitted; elsewhere df counts the null model's columns)
    p_kept = K + (fit.sum_h[w][:, :A - 1] > 0).sum(1) + lrt_df
    return (np.array(fit.beta), np.array(fit.se), lrt, lrt_df, np.array(fit.n_alt, np.int32), np.array(fit.n_alt_case, np.int32),
            np.array(fit.sum_h[w], np.int32), n, fit.n_case[w].astype(np.int32), (n - p_kept).astype(np.int32), np.array(fit.n_miss, np.int32),
            np.array(fit.iters, np.int32), np.array(fit.status, np.int32))


def logit_from_fits(fit_fn, C, A, K):
    """fit_fn(c0, c1) -> LogitFit; walks the SNPs in chunks of logit_snps_per_chunk(A, K) -> AncestryAssocLogit.  A GNX_EINVAL (labels out of
    range, a phenotype that is not 0 / 1) is fit_fn's to raise."""
    step = logit_snps_per_chunk(A, K)
    parts = [finish_logit(fit_fn(c0, min(c0 + step, C)), K) for c0 in range(0, C, step)]
    beta, se, lrt, lrt_df, n_alt, n_alt_case, n_hap, n, n_case, df, n_miss, iters, status = (np.concatenate([p[i] for p in parts]) for i in range(13))
    z, p, lrt_p = logit_p_values(beta, se, lrt, lrt_df)
    return AncestryAssocLogit(beta, se, z, p, lrt, lrt_df, lrt_p, n_alt, n_alt_case, n_hap, n, n_case, df, n_miss, iters, status)


def check_binary(y, use, names=None):
    """ValueError when a used individual's finite phenotype is neither 0 nor 1 (names: the sample names for the message)"""
    y = np.asarray(y, np.float64)
    bad = np.isfinite(y) & (y != 0.0) & (y != 1.0)
    if use is not None:
        bad &= np.asarray(use) != 0
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        who = f"sample '{names[i]}'" if names is not None else f"individual {i}"
        raise ValueError(f"a logistic association needs phenotypes coded 0 / 1: {who} has {y[i]:g} ({int(bad.sum())} such in all)")


def logit_host(ctx, X, labels, M, A, y, Z, use, c0, c1, min_ac=1, tol=LOGIT_TOL, max_iter=LOGIT_MAX_ITER, check=True, want_theta=True):
    """gnx_ancestry_assoc_logit on host arrays: X (N, C) int8 (any row stride), labels (N, W) int32 -> LogitFit of [c0, c1)"""
    from . import ancestry_ops as ops
    return ops.assoc_logit(ops.host_front(ctx, X, labels, M, A, strided=True), y, Z, use, c0, c1, min_ac, tol, max_iter, check, want_theta)


def covariates(n_ind, y, Z=None, use=None):
    """y (n_ind,), Z (n_ind, K) or None (the intercept only), use (n_ind,) or None -> contiguous float64 / float64 / uint8 arrays"""
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if y.shape[0] != n_ind:
        raise ValueError(f"y must have one value per individual ({n_ind}), got {y.shape[0]}")
    Z = np.ones((n_ind, 1)) if Z is None else np.ascontiguousarray(Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[0] != n_ind or Z.shape[1] < 1:
        raise ValueError(f"Z must be (n_ind={n_ind}, K >= 1), got {Z.shape}")
    use = np.ones(n_ind, np.uint8) if use is None else np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
    if use.shape != (n_ind,):
        raise ValueError(f"use must have one byte per individual ({n_ind}), got {use.shape}")
    return y, Z, use


def read_phenotypes(path, samples):
    """the phenotype file: a TSV with a header `sample  pheno  [covariate ...]`, matched to `samples` by name -> (y, Z, use, names).
    Z gets an intercept column in front of the file's covariates.  A query sample the file lacks, or whose phenotype is empty / NA, has
    use = 0 (y = NaN); a covariate that is empty, NA or not finite stays non-finite in Z, which the model's participation rule drops.
    File samples the query lacks are ignored.  A sample listed twice is an error."""
    with open(path) as f:
        lines = [ln.rstrip("\n").rstrip("\r") for ln in f if ln.strip()]
    if not lines:
        raise ValueError(f"{path}: empty phenotype file")
    head = lines[0].split("\t")
    if len(head) < 2 or head[0] != "sample" or head[1] != "pheno":
        raise ValueError(f"{path}: the header must start with 'sample<TAB>pheno', got {head[:2]}")
    cov_names = head[2:]

    def num(cell):
        cell = cell.strip()
        if cell == "" or cell.upper() in ("NA", "NAN", "."):
            return np.nan
        try:
            return float(cell)
        except ValueError:
            raise ValueError(f"{path}: '{cell}' is not a number") from None

    rows = {}
    for ln in lines[1:]:
        cells = ln.split("\t")
        if len(cells) != len(head):
            raise ValueError(f"{path}: a line has {len(cells)} cells, the header {len(head)}")
        if cells[0] in rows:
            raise ValueError(f"{path}: sample '{cells[0]}' is listed twice")
        rows[cells[0]] = [num(c) for c in cells[1:]]
    n = len(samples)
    y = np.full(n, np.nan)
    Z = np.ones((n, 1 + len(cov_names)))
    use = np.zeros(n, np.uint8)
    for i, name in enumerate(samples):
        r = rows.get(str(name))
        if r is None:
            Z[i, 1:] = np.nan
            continue
        y[i] = r[0]
        Z[i, 1:] = r[1:]
        use[i] = 1 if np.isfinite(r[0]) else 0
    return y, Z, use, ["intercept"] + cov_names


def stats_host(ctx, X, labels, M, A, y, Z, use, c0, c1, min_ac=1, check=True):
    """gnx_ancestry_assoc_stats on host arrays: X (N, C) int8 (any row stride), labels (N, W) int32 -> AssocStats of [c0, c1)"""
    from . import ancestry_ops as ops
    return ops.assoc_stats(ops.host_front(ctx, X, labels, M, A, strided=True), y, Z, use, c0, c1, min_ac, check)
