"""Admixture mapping: the regression of T quantitative traits on the local ancestry itself, window by window, from the labels alone
(no genotypes), with a genome-wide threshold by max-T permutation.  The device reduces the labels, Y and Z to per-window blocks on the
float64 matrix cores (gnx_ancestry_admixmap; include/gnomix_hip.h states the blocks, DESIGN.md section 4.24 the contract); this module
factors them (numpy float64, section 4.18's Cholesky) and runs the permutations through the same device entry.

THE MODEL.  labels (N, W) int32, rows 2 i and 2 i + 1 are individual i; Y (N / 2, T); Z (N / 2, K) with the intercept column supplied by the
caller; use (N / 2,) or None.  Individual i takes part at window k when use[i] != 0, Z[i, :] is finite, every entry of Y[i, :] is finite and
both labels at k lie in [0, A).  h_a[i, k] in {0, 1, 2} counts i's haplotypes labelled a at k; n_k the participants; hs[k, a] = sum_i h_a.
Ancestry a is KEPT at window k when hs[k, a] >= min_hap and 2 n_k - hs[k, a] >= min_hap (min_hap >= 1).
  Per-ancestry test, for every kept a: y = Z g + alpha_a h_a by OLS over the participants -> beta, se, t, p (two-sided Student t with
    df = n_k - K - 1), each (W, A, T); NaN where a is not kept, and where h_a is a linear function of Z among the participants (the pivot
    of the rank-one extension of the unit-diagonal normal matrix is <= assoc.PIVOT_MIN).
  Joint test: the reference ancestry is the kept one with the largest hs (ties: the lowest index); the columns are the OTHER kept
    ancestries (ancestries that are not kept fall into the reference); q = kept - 1; full model y = Z g + sum alpha_a h_a, null model
    y = Z g; F = ((RSS0 - RSS1) / q) / (RSS1 / df2), df1 = q, df2 = n_k - K - q, p_joint = scipy.special.fdtrc(df1, df2, F).
STATUS per window (one int32; the first rule that applies):
    2   df = n_k - K - 1 < 1 (section 4.18's number): every float of the window is NaN;
    1   Z^T Z is not positive definite in the host's Cholesky (section 4.18's number): every float of the window is NaN;
    3   q < 1, nothing to test jointly: F and p_joint are NaN and df1 = q <= 0; the per-ancestry cells of the kept ancestries (there is at
        most one) ARE fitted: read them from `kept` and the NaN pattern, not from status;
    0   fitted.
  With status 0, F and p_joint are still NaN where df2 < 1 or the full model's normal matrix is not positive definite; df1 and df2 say
  which.  df1, df2 are q and n_k - K - q in every window."""
import collections
import ctypes

import numpy as np

from . import assoc
from .assoc import PIVOT_MIN, STATS_CHUNK_BYTES, _cholesky_batched, _lower_inverse_batched

STATUS_OK, STATUS_SINGULAR, STATUS_NO_DF, STATUS_NOTHING = 0, 1, 2, 3

AdmixStats = collections.namedtuple("AdmixStats", "n hs hh ztz zth ry yty n_bad")
AdmixStats.__doc__ = """the blocks of the windows [w0, w1) (gnx_ancestry_admixmap): n (nw,), hs (nw, A) int32; hh (nw, A, A) int64, symmetric;
ztz (nw, K, K), symmetric, zth (nw, K, A), ry (nw, K + A, T) = [Z, h_0 .. h_{A-1}]^T Y, yty (nw, T) float64; n_bad: labels outside [0, A)"""

AdmixMap = collections.namedtuple("AdmixMap", "beta se t p F df1 df2 p_joint n n_hap kept status perm_max_t perm_max_F p_adj_t p_adj_F")
AdmixMap.__doc__ = """what admixture_mapping returns.  beta, se, t, p: (W, A, T) float64; F, p_joint: (W, T); df1, df2, n, status: (W,) int32;
n_hap = hs (W, A) int32; kept (W, A) bool.  perm_max_t, perm_max_F: (T, n_perm), the maximum over the kept (window, ancestry) cells of |t| and
over the windows of F in permutation j; p_adj_t (W, A, T), p_adj_F (W, T): (1 + #{j: perm_max >= observed}) / (1 + n_perm), NaN where the
observed statistic is.  The four permutation fields are None when n_perm = 0.  The module docstring states the status codes."""


def layout(A, K):
    """columns of win_i (int32) and win_g (float64) of the C ABI"""
    return 1 + A + A * (A + 1) // 2, K * (K + 1) // 2 + K * A


def stats_buffers(A, K, T, w0, w1, empty=None):
    """zeroed (or empty(shape, dtype)) arrays of one call, in the order of the C ABI: win_i, win_g, win_y, win_yy"""
    NI, NG = layout(A, K)
    nw, ldt = max(w1 - w0, 0), assoc.trait_ldt(T)
    new = empty or (lambda shape, dtype: np.zeros(shape, dtype))
    return new((nw, NI), np.int32), new((nw, NG), np.float64), new((nw, K + A, ldt), np.float64), new((nw, ldt), np.float64)


def split_blocks(win_i, win_g, win_y, win_yy, A, K, T, n_bad=0):
    """the four arrays of the C ABI -> AdmixStats (the triangles unfolded; ry and yty are views)"""
    nw = win_i.shape[0]
    iu = np.triu_indices(A)
    hh = np.zeros((nw, A, A), np.int64)
    hh[:, iu[0], iu[1]] = win_i[:, 1 + A:]
    hh[:, iu[1], iu[0]] = win_i[:, 1 + A:]
    ku = np.triu_indices(K)
    nzz = K * (K + 1) // 2
    ztz = np.zeros((nw, K, K))
    ztz[:, ku[0], ku[1]] = win_g[:, :nzz]
    ztz[:, ku[1], ku[0]] = win_g[:, :nzz]
    return AdmixStats(win_i[:, 0], win_i[:, 1:1 + A], hh, ztz, win_g[:, nzz:].reshape(nw, K, A), win_y[:, :, :T], win_yy[:, :T], int(n_bad))


Factor = collections.namedtuple("Factor", "n hs kept ref cols q df df1 df2 status sz Li0 C sh d_rel aliased Lij sj joint_bad")


def factor(st, K, min_hap=1):
    """the trait-independent half of the finish: the column rule, Z^T Z's Cholesky (once per window), the rank-one extension of every
    ancestry and the factorisation of the joint model's Schur complement -> Factor"""
    if min_hap < 1:
        raise ValueError("min_hap must be >= 1")
    n = np.asarray(st.n, np.int64)
    hs = np.asarray(st.hs, np.int64)
    nw, A = hs.shape
    kept = (hs >= min_hap) & (2 * n[:, None] - hs >= min_hap)
    ref = np.argmax(np.where(kept, hs, -1), axis=1)                     # the first of the largest
    cols = kept.copy()
    cols[np.arange(nw), ref] = False
    q = kept.sum(1) - 1
    df, df2 = n - K - 1, n - K - q
    # Z^T Z with a unit diagonal
    dz = np.einsum("wkk->wk", st.ztz)
    zero_col = ~(dz > 0)
    sz = np.sqrt(np.where(zero_col, 1.0, dz))
    G0 = st.ztz / (sz[:, :, None] * sz[:, None, :])
    G0[:, np.arange(K), np.arange(K)] = np.where(zero_col, 0.0, 1.0)
    L0, bad0 = _cholesky_batched(G0)
    bad0 |= zero_col.any(1)
    Li0 = _lower_inverse_batched(L0)
    status = np.where(df < 1, STATUS_NO_DF, np.where(bad0, STATUS_SINGULAR, np.where(q < 1, STATUS_NOTHING, STATUS_OK))).astype(np.int32)
    # every ancestry column scaled to unit length, then reduced against Z: C = L0^-1 Z^T h / |h|
    dh = np.einsum("waa->wa", st.hh).astype(np.float64)
    sh = np.sqrt(np.where(dh > 0, dh, 1.0))
    C = np.matmul(Li0, st.zth / (sz[:, :, None] * sh[:, None, :]))     # (nw, K, A)
    d_rel = 1.0 - np.einsum("wka,wka->wa", C, C)                        # the pivot of [Z, h_a]'s unit-diagonal normal matrix
    aliased = ~(d_rel > PIVOT_MIN)
    # the joint model: the Schur complement of the kept columns but the reference; a dropped column is a unit row / column
    S = st.hh / (sh[:, :, None] * sh[:, None, :]) - np.einsum("wka,wkb->wab", C, C)
    S = np.where(cols[:, :, None] & cols[:, None, :], S, 0.0)
    ds = np.einsum("waa->wa", S)
    live = cols & (ds > PIVOT_MIN)
    sj = np.sqrt(np.where(live, ds, 1.0))
    Sj = S / (sj[:, :, None] * sj[:, None, :])
    Sj[:, np.arange(A), np.arange(A)] = np.where(cols, np.where(live, 1.0, 0.0), 1.0)
    Lj, jbad = _cholesky_batched(Sj)
    return Factor(n, hs, kept, ref, cols, q, df, q, df2, status, sz, Li0, C, sh, d_rel, aliased, _lower_inverse_batched(Lj), sj, jbad)


def _bmm(L, B):
    """L (w, i, k) times B (w, k, t) -> (w, i, t), the sum over k in ascending order, term by term: every element is the same chain of
    float64 operations whatever t's extent is (a BLAS product may round a column differently in a wider matrix), so a run cut into
    column chunks equals the uncut run bit for bit"""
    out = np.zeros((L.shape[0], L.shape[1], B.shape[2]))
    for k in range(L.shape[2]):
        out += L[:, :, k, None] * B[:, None, k, :]
    return out


def _sumsq(v):
    """(w, k, t) -> (w, t): sum_k v^2 in ascending k, term by term (as _bmm)"""
    out = np.zeros((v.shape[0], v.shape[2]))
    for k in range(v.shape[1]):
        out += v[:, k] * v[:, k]
    return out


def solve(f, ry, yty, K):
    """the trait-dependent half: all right-hand sides as batched products -> beta, se, t (nw, A, T) and F (nw, T), NaN as the module states"""
    with np.errstate(divide="ignore", invalid="ignore"):
        v0 = _bmm(f.Li0, ry[:, :K] / f.sz[:, :, None])                                        # (nw, K, T)
        rss0 = yty - _sumsq(v0)
        R = ry[:, K:] / f.sh[:, :, None] - _bmm(np.transpose(f.C, (0, 2, 1)), v0)             # h_a / |h_a| reduced against Z, times y
        beta_s = R / f.d_rel[:, :, None]
        rss = np.maximum(rss0[:, None, :] - R * beta_s, 0.0)
        se_s = np.sqrt(rss / f.df[:, None, None] / f.d_rel[:, :, None])
        beta, se = beta_s / f.sh[:, :, None], se_s / f.sh[:, :, None]
        tt = beta / se
        dead = ((f.status == STATUS_NO_DF) | (f.status == STATUS_SINGULAR))[:, None] | ~f.kept | f.aliased
        beta, se, tt = (np.where(dead[:, :, None], np.nan, x) for x in (beta, se, tt))
        u = _bmm(f.Lij, np.where(f.cols[:, :, None], R, 0.0) / f.sj[:, :, None])
        ess = _sumsq(u)
        rss1 = np.maximum(rss0 - ess, 0.0)
        F = (ess / f.df1[:, None]) / (rss1 / f.df2[:, None])
        jdead = (f.status != STATUS_OK) | (f.df2 < 1) | f.joint_bad
        F = np.where(jdead[:, None], np.nan, F)
    return beta, se, tt, F


def p_values(t, df, F, df1, df2):
    """two-sided Student p of t (W, A, T) with df (W,), and the F distribution's upper tail of F (W, T); NaN where the statistic is"""
    from scipy import special
    with np.errstate(invalid="ignore"):
        p = 2.0 * special.stdtr(np.maximum(df, 1)[:, None, None].astype(np.float64), -np.abs(t))
        pj = special.fdtrc(np.maximum(df1, 1)[:, None].astype(np.float64), np.maximum(df2, 1)[:, None].astype(np.float64), F)
    return np.where(np.isnan(t), np.nan, p), np.where(np.isnan(F), np.nan, pj)


def finish(st, K, min_hap=1):
    """AdmixStats -> AdmixMap without permutation fields"""
    f = factor(st, K, min_hap)
    beta, se, tt, F = solve(f, st.ry, st.yty, K)
    p, pj = p_values(tt, f.df, F, f.df1, f.df2)
    return AdmixMap(beta, se, tt, p, F, f.df1.astype(np.int32), f.df2.astype(np.int32), pj, f.n.astype(np.int32), f.hs.astype(np.int32), f.kept, f.status,
                    None, None, None, None)


def base_participants(Y, Z, use):
    """those that use, Z and Y admit, independent of the window -> (n_ind,) bool"""
    return (np.asarray(use) != 0) & np.isfinite(Z).all(1) & np.isfinite(Y).all(1)


def permutation_columns(Y, Z, use, seed, j0, j1):
    """the Freedman-Lane columns of the permutations j0 .. j1 - 1 -> (n_ind, (j1 - j0) * T) float64, column (j - j0) * T + t.  Per trait t:
    g = lstsq(Z, y) over the base participants, e = y - Z g; permutation j is numpy.random.Generator(PCG64([seed, j])).permutation(n_base)
    applied to e: Y*[:, t, j] = Z g + e[pi_j].  pi_j depends on (seed, j, n_base) alone, so runs on different chromosomes with the same
    samples draw the same permutations.  Rows of individuals outside the base are NaN (they take no part)."""
    Y, Z = np.asarray(Y, np.float64), np.asarray(Z, np.float64)
    n_ind, T = Y.shape
    base = base_participants(Y, Z, np.ones(n_ind, np.uint8) if use is None else use)
    Zb, Yb = Z[base], Y[base]
    fitted = Zb @ np.linalg.lstsq(Zb, Yb, rcond=None)[0]
    e = Yb - fitted
    out = np.full((n_ind, j1 - j0, T), np.nan)
    for j in range(j0, j1):
        pi = np.random.Generator(np.random.PCG64([int(seed), j])).permutation(len(Zb))
        out[base, j - j0] = fitted + e[pi]
    return out.reshape(n_ind, (j1 - j0) * T)


def columns_per_chunk(W, A, K, max_bytes=STATS_CHUNK_BYTES):
    """trait columns per call such that the call's blocks (win_y, win_yy) and the three (W, A, cols) results stay below max_bytes; a
    multiple of 16 (the device pads a call's columns to that), at least 16"""
    per_col = W * ((K + A + 1) * 8 + (3 * A + 1) * 8)
    return max(16, int(max_bytes) // per_col // 16 * 16)


def adjusted_p(obs, perm_max):
    """obs (..., T) the observed statistic (|t| or F), perm_max (T, n_perm) -> (1 + #{j: perm_max[t, j] >= obs}) / (1 + n_perm); NaN where obs is"""
    T, n_perm = perm_max.shape
    srt = np.sort(np.where(np.isnan(perm_max), -np.inf, perm_max), axis=1)
    out = np.full(obs.shape, np.nan)
    for t in range(T):
        o = obs[..., t]
        ok = ~np.isnan(o)
        ge = n_perm - np.searchsorted(srt[t], o[ok], side="left")
        out[..., t][ok] = (1.0 + ge) / (1.0 + n_perm)
    return out


def run(stats_fn, W, A, Y, Z=None, use=None, min_hap=1, n_perm=0, seed=0, chunk_bytes=None):
    """stats_fn(Ycols, Z, use) -> AdmixStats of all W windows for the trait columns Ycols; the observed fit and the permutations -> AdmixMap.
    A GNX_EINVAL for labels out of range is stats_fn's to raise."""
    if min_hap < 1:
        raise ValueError("min_hap must be >= 1")
    if n_perm < 0:
        raise ValueError("n_perm must be >= 0")
    n_ind = np.asarray(Y).shape[0]
    Y, Z, use, _ = assoc.trait_covariates(n_ind, Y, Z, use)
    K, T = Z.shape[1], Y.shape[1]
    # the participation of the whole batch of traits, applied once: a chunk of columns then takes part exactly as all of them would
    base = base_participants(Y, Z, use)
    use_b = np.ascontiguousarray(base, dtype=np.uint8)
    Yb = np.where(base[:, None], Y, 0.0)
    step = columns_per_chunk(W, A, K, STATS_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
    f, parts = None, []
    for t0 in range(0, T, step):
        st = stats_fn(np.ascontiguousarray(Yb[:, t0:t0 + step]), Z, use_b)
        f = f or factor(st, K, min_hap)
        parts.append(solve(f, st.ry, st.yty, K))
    beta, se, tt, F = (np.concatenate([p[i] for p in parts], axis=-1) for i in range(4))
    p, pj = p_values(tt, f.df, F, f.df1, f.df2)
    perm = [None] * 4
    if n_perm > 0:
        pmt, pmF = np.full((T, n_perm), np.nan), np.full((T, n_perm), np.nan)
        jstep = max(1, step // T)                       # whole permutations per call; T > step: one permutation, its traits in column chunks
        for j0 in range(0, n_perm, jstep):
            j1 = min(j0 + jstep, n_perm)
            nj = j1 - j0
            Yp = np.where(base[:, None], permutation_columns(Yb, Z, use_b, seed, j0, j1), 0.0)
            width = nj * T if T <= step else step
            for c0 in range(0, nj * T, width):
                c1 = min(c0 + width, nj * T)
                st = stats_fn(np.ascontiguousarray(Yp[:, c0:c1]), Z, use_b)
                _, _, tp, Fp = solve(f, st.ry, st.yty, K)
                with np.errstate(invalid="ignore"):
                    mt = np.fmax.reduce(np.abs(tp).reshape(-1, c1 - c0), axis=0, initial=-np.inf)      # NaN cells are skipped
                    mF = np.fmax.reduce(Fp, axis=0, initial=-np.inf)
                cols = np.arange(c0, c1)
                pmt[cols % T, j0 + cols // T] = np.where(np.isneginf(mt), np.nan, mt)
                pmF[cols % T, j0 + cols // T] = np.where(np.isneginf(mF), np.nan, mF)
        perm = [pmt, pmF, adjusted_p(np.abs(tt), pmt), adjusted_p(F, pmF)]
    return AdmixMap(beta, se, tt, p, F, f.df1.astype(np.int32), f.df2.astype(np.int32), pj, f.n.astype(np.int32), f.hs.astype(np.int32), f.kept, f.status,
                    *perm)


def admixture_mapping(ctx, labels, A, Y, Z=None, use=None, min_hap=1, n_perm=0, seed=0, check=True, chunk_bytes=None):
    """Admixture mapping of T quantitative traits Y (N / 2, T) (a 1-D y: T = 1) on the labels (N, W) int32 alone: a numpy array, or a CUDA
    tensor that never leaves HBM.  It needs no model and no genotypes: `labels` may come straight from postprocess.read_msp.  The module
    docstring states the model, the tests and the status codes -> AdmixMap.
    n_perm > 0: Freedman-Lane max-T permutations (permutation_columns).  Permutation j is a function of (seed, j, the number of base
    participants) alone: runs on different chromosomes with the same samples and the same seed draw the same permutations, and their
    perm_max_t / perm_max_F combine with numpy.maximum into the genome-wide maxima.  The permuted columns go through the same device
    entry as ordinary traits, in column chunks whose blocks and results stay below chunk_bytes (default assoc.STATS_CHUNK_BYTES); only
    the two maxima per (trait, permutation) are kept and no p-value is computed for a permuted column.
    LIMIT: where df1 / df2 differ between windows, perm_max_F compares F values of different distributions (max-T on |t| has the same
    property for df, usually harmless; per-window p-values would cure it and are not computed).
    check=False: labels outside [0, A) do not raise (such an individual takes no part at that window)."""
    from . import ancestry_ops as ops
    N, W = labels.shape
    ops.check_even(N)
    Y = np.asarray(Y, np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    if Y.ndim != 2 or Y.shape[0] != N // 2:
        raise ValueError(f"Y must be (N / 2 = {N // 2}, T >= 1), got {Y.shape}")
    return run(lambda Yc, Zc, uc: ops.admixmap_stats(ctx, labels, A, Yc, Zc, uc, 0, W, check), W, int(A), Y, Z, use, min_hap, n_perm, seed, chunk_bytes)
