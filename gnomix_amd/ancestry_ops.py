"""The ancestry-specific ops (csrc/summary/: allele counts, dosage, scores, pair counts, LD counts, and the linear, many-trait and
logistic association blocks) driven from Python, each written ONCE over a `Front`: what the three forms of an op (host arrays, CUDA
tensors, the parsed query) differ in.  AncestryOps is the half of DeviceModel that offers them; the module-level functions of
postprocess.py and assoc.py are thin calls into the ops here.  DESIGN.md (section "one copy of each shared helper") has the table of
verdict rules."""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from . import _lib, assoc
from .asmds import PairCounts
from .ld import LDCounts
from .postprocess import AlleleCounts, AncestryScores, AncestrySummary, _summary_weights, score_chunks, score_tables

Front = collections.namedtuple("Front", "ctx suffix head N C M W A alloc ptr put host keep")
Front.__doc__ = """one form of the inputs of an op: suffix of the C entry point ("", "_dev", "_gt2"); head of its argument list ((ctx.h, rows,
row_kind, ld_rows, labels, ld_labels, N, C, M, W, A), or (model.h, G, V, ldg, N, src, labels) for the parsed query); the geometry;
alloc(shape, dtype, zero=True) -> an output where the rows live (numpy array / CUDA tensor); ptr(a) -> its address (None stays None);
put(a) -> a host array where the rows live; host(a) -> an output as a numpy array; keep: what must outlive the call"""


# ---- one copy of each check -----------------------------------------------------------------------------------------------------------
def check_labels(labels, N, W=None):
    """labels as an op takes them: (N, W) int32, a numpy array made C-contiguous or a CUDA tensor as it is; W None: any W, the labels' own"""
    lab = labels if hasattr(labels, "is_cuda") else np.ascontiguousarray(labels, dtype=np.int32)
    if len(lab.shape) != 2 or lab.shape[0] != N or (W is not None and lab.shape[1] != W):
        raise ValueError(f"labels must be (N={N}, W{'' if W is None else '=%d' % W}), got {tuple(lab.shape)}")
    return lab


def check_even(N):
    """the ops that work per individual refuse an odd number of haplotype rows"""
    if N % 2:
        raise ValueError("N must be even (an individual has two haplotype rows)")


def snp_bounds(c0, c1, C):
    """[c0, c1) as ints; c1 None: to the last SNP"""
    return int(c0), int(C) if c1 is None else int(c1)


def verdict(ctx, rc, n_bad, check=True, handed=None):
    """raise the library's error for rc, unless the caller waived it (check=False) for labels out of range (n_bad of them) and rc is a
    code that still hands the outputs over (`handed`; None: every code does)"""
    if check or not n_bad or (handed is not None and rc not in handed):
        ctx.check(rc)


# ---- the three fronts ------------------------------------------------------------------------------------------------------------------
def _address(a):
    return None if a is None else a.ctypes.data


def _same(a):
    return a


def host_rows(X, packed=False, C=None, strided=False):
    """-> (rows, row_kind, C).  int8 rows keep their bytes (anything but 0 / 1 is a missing call), other dtypes are re-coded to 0 / 1 / 2
    first; the rows are made C-contiguous unless `strided` and they are int8 with contiguous rows already (any row stride); packed rows
    (gnx_pack_x layout) need C"""
    if packed:
        rows = np.ascontiguousarray(X, dtype=np.uint8)
        if C is None:
            raise ValueError("packed rows: pass C, the number of SNPs a row holds")
        if rows.ndim != 2 or rows.shape[1] < (int(C) + 3) // 4:
            raise ValueError(f"packed X must be (N, >= ceil(C / 4) = {(int(C) + 3) // 4}) uint8, got {rows.shape}")
        return rows, _lib.GNX_ROWS_PACKED2, int(C)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"X must be (N, C), got {X.shape}")
    if C is not None and int(C) != X.shape[1]:
        raise ValueError(f"X has {X.shape[1]} columns, C = {C}")
    if X.dtype != np.int8:
        X = np.where((X == 0) | (X == 1), X, 2).astype(np.int8)
    if not (strided and X.strides[1] == 1):
        X = np.ascontiguousarray(X)
    return X, _lib.GNX_ROWS_INT8, X.shape[1]


def host_front(ctx, X, labels, M, A, packed=False, C=None, W=None, even=False, strided=False):
    """host arrays: X (N, C) int8 (packed: the 2-bit rows of pack_x and C) and (N, W) labels (W None: the labels' own)"""
    rows, kind, C = host_rows(X, packed, C, strided)
    N = rows.shape[0]
    if even:
        check_even(N)
    lab = check_labels(labels, N, W)
    W = lab.shape[1]
    head = (ctx.h, rows.ctypes.data, kind, rows.strides[0] if N > 1 else rows.shape[1], lab.ctypes.data, W, N, C, int(M), W, int(A))
    return Front(ctx, "", head, N, C, int(M), W, int(A), lambda shape, dtype, zero=True: (np.zeros if zero else np.empty)(shape, dtype),
                 _address, _same, _same, (rows, lab))


def device_front(model, X_t, lab_t, even=False):
    """CUDA tensors: X_t int8 (N, C) or the uint8 tensor pack_device returns, lab_t (N, W) int32, contiguous rows with any row stride;
    binds the library to torch's current stream"""
    import torch
    assert X_t.is_cuda and X_t.dim() == 2 and (X_t.shape[1] == 0 or X_t.stride(1) == 1)
    assert lab_t.is_cuda and lab_t.dtype == torch.int32 and lab_t.dim() == 2 and (lab_t.shape[1] == 0 or lab_t.stride(1) == 1)
    N, C, W = X_t.shape[0], model.C, model.W
    if X_t.dtype == torch.int8:
        kind, need = _lib.GNX_ROWS_INT8, C
        if X_t.shape[1] != C:
            raise ValueError(f"X must be (N, C={C}) int8, got {tuple(X_t.shape)}")
    elif X_t.dtype == torch.uint8:
        kind, need = _lib.GNX_ROWS_PACKED2, (C + 3) // 4
        if X_t.shape[1] < need:
            raise ValueError(f"packed X must be (N, >= {need}) uint8, got {tuple(X_t.shape)}")
    else:
        raise ValueError("X must be an int8 (N, C) tensor or the uint8 tensor pack_device returns")
    if even:
        check_even(N)
    check_labels(lab_t, N, W)
    dev, dtypes = X_t.device, {np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}     # (a dict: the ops' three dtypes)
    head = (model.ctx.h, X_t.data_ptr(), kind, X_t.stride(0) if N > 1 else max(X_t.shape[1], need), lab_t.data_ptr(),
            lab_t.stride(0) if N > 1 else W, N, C, model.M, W, model.A)
    model._bind_torch_stream()
    return Front(model.ctx, "_dev", head, N, C, model.M, W, model.A,
                 lambda shape, dtype, zero=True: (torch.zeros if zero else torch.empty)(shape, dtype=dtypes[dtype], device=dev),
                 lambda a: None if a is None else a.data_ptr(), lambda a: torch.from_numpy(a).to(dev), lambda a: None if a is None else a.cpu().numpy(),
                 (X_t, lab_t))


def gt2_front(model, G, N, src, labels, even=False):
    """the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the rows exist only in HBM"""
    G, N, src = model._gt2_args(G, N, src)
    if even:
        check_even(N)
    lab = check_labels(labels, N, model.W)
    head = (model.h, G.ctypes.data, G.shape[0], G.shape[1], N, src.ctypes.data, lab.ctypes.data)
    return Front(model.ctx, "_gt2", head, N, model.C, model.M, model.W, model.A, lambda shape, dtype, zero=True: np.zeros(shape, dtype),
                 _address, _same, _same, (G, src, lab))


# ---- each op once over a front ---------------------------------------------------------------------------------------------------------
def _call(f, name, *tail, row_kind=True):
    """gnx_ancestry_<name><suffix>(head, tail); row_kind=False: the entry point's host form takes int8 rows only and no row_kind"""
    head = f.head if row_kind or f.suffix else f.head[:2] + f.head[3:]
    return getattr(f.ctx.lib, "gnx_ancestry_" + name + f.suffix)(*head, *tail)


def _debug(f, *values):
    """the debug arguments exist on the host and _dev forms only"""
    return () if f.suffix == "_gt2" else tuple(map(int, values))


def allele_counts(f, debug_rows_per_chunk=0, debug_flush_every=0):
    obs, alt, miss = (f.alloc((f.A, f.C), np.int32) for _ in range(3))
    f.ctx.check(_call(f, "allele_counts", f.ptr(obs), f.ptr(alt), f.ptr(miss), *_debug(f, debug_rows_per_chunk, debug_flush_every)))
    return AlleleCounts(obs, alt, miss)


def dosage(f, ancestry):
    dos, hap = (f.alloc((f.N // 2, f.C), np.uint8) for _ in range(2))
    f.ctx.check(_call(f, "dosage", int(ancestry), f.ptr(dos), f.C, f.ptr(hap), f.C))
    return dos, hap


def scores(f, w, eff, debug_windows_per_block=0, debug_rows_per_pass=0):
    """w (C, A, S) float64 and eff (C,) uint8 where the rows live (score_tables); tables wider than GNX_SCORE_MAX_S go chunk by chunk"""
    S, n = w.shape[2], f.N // 2
    score = f.alloc((n, f.A, S), np.float64)
    counts = [f.alloc((n, f.A), np.int32) for _ in range(3)]
    for s0, s1 in score_chunks(S):
        whole = (s0, s1) == (0, S)
        wc = w if whole else w[:, :, s0:s1].contiguous() if f.suffix == "_dev" else np.ascontiguousarray(w[:, :, s0:s1])
        out = score if whole else f.alloc((n, f.A, s1 - s0), np.float64)
        n_bad = ctypes.c_int64(0)
        f.ctx.check(_call(f, "score", f.ptr(wc), s1 - s0, f.ptr(eff), f.ptr(out), *(f.ptr(v) if s0 == 0 else None for v in counts),
                          *_debug(f, debug_windows_per_block, debug_rows_per_pass), ctypes.byref(n_bad)))
        if not whole:
            score[:, :, s0:s1] = out
    return AncestryScores(score, *counts)


def pair_counts(f, ancestry, snps=None, debug_snps_per_block=0, check=True):
    c0, c1 = snp_bounds(*((0, None) if snps is None else snps), f.C)
    n = f.N // 2
    DD, DO, OO = (f.alloc((n, n), np.int32) for _ in range(3))
    n_bad = ctypes.c_int64(0)
    rc = _call(f, "pair_counts", int(ancestry), c0, c1, f.ptr(DD), f.ptr(DO), f.ptr(OO), n, *_debug(f, debug_snps_per_block), ctypes.byref(n_bad))
    verdict(f.ctx, rc, n_bad.value, check)
    return PairCounts(DD, DO, OO)


def ld_counts(f, ancestry, c0=0, c1=None, band=256, debug_haps_per_block=0, check=True):
    (c0, c1), band = snp_bounds(c0, c1, f.C), int(band)
    tabs = [f.alloc((max(c1 - c0, 0), max(band, 0)), np.int32) for _ in range(4)]     # zeroed: the bands past C have no owner
    n_bad = ctypes.c_int64(0)
    rc = _call(f, "ld_counts", int(ancestry), c0, c1, band, *(f.ptr(t) for t in tabs), band, *_debug(f, debug_haps_per_block), ctypes.byref(n_bad))
    verdict(f.ctx, rc, n_bad.value, check)
    return LDCounts(*tabs, c0, band)


def _blocks(f, zero):
    """the allocator of an association op's blocks (assoc.*_buffers); zero=False: uninitialised on tensors, where the kernel writes all"""
    return lambda shape, dtype: f.alloc(shape, dtype, zero or f.suffix != "_dev")


def assoc_stats(f, y, Z, use, c0, c1, min_ac=1, check=True):
    y, Z, use = assoc.covariates(f.N // 2, y, Z, use)
    K = Z.shape[1]
    bufs = assoc.stats_buffers(f.A, K, c0, c1, f.M, f.W, empty=_blocks(f, False))
    y, Z, use = (f.put(v) for v in (y, Z, use))
    n_bad = ctypes.c_int64(0)
    rc = _call(f, "assoc_stats", f.ptr(y), f.ptr(Z), K, f.ptr(use), int(min_ac), c0, c1, *(f.ptr(b) for b in bufs), ctypes.byref(n_bad),
               row_kind=False)
    verdict(f.ctx, rc, n_bad.value, check)
    return assoc.split_blocks(*(f.host(b) for b in bufs), f.A, K, c0, c1, f.M, f.W, n_bad.value)


def assoc_traits(f, Y, Z, use, c0, c1, min_ac=1, check=True):
    Y, Z, use, _ = assoc.trait_covariates(f.N // 2, Y, Z, use)
    K, T = Z.shape[1], Y.shape[1]
    bufs = assoc.trait_buffers(f.A, K, T, c0, c1, f.M, f.W, empty=_blocks(f, False))
    Y, Z, use = (f.put(v) for v in (Y, Z, use))
    n_bad = ctypes.c_int64(0)
    rc = _call(f, "assoc_traits", f.ptr(Y), T, T, f.ptr(Z), K, f.ptr(use), int(min_ac), c0, c1, *(f.ptr(b) for b in bufs), ctypes.byref(n_bad),
               row_kind=False)
    verdict(f.ctx, rc, n_bad.value, check)
    return assoc.split_traits(*(f.host(b) for b in bufs), T, c0, c1, f.M, f.W, n_bad.value)


def assoc_logit(f, y, Z, use, c0, c1, min_ac=1, tol=None, max_iter=None, check=True, want_theta=True):
    tol = assoc.LOGIT_TOL if tol is None else float(tol)
    max_iter = assoc.LOGIT_MAX_ITER if max_iter is None else int(max_iter)
    y, Z, use = assoc.covariates(f.N // 2, y, Z, use)
    K = Z.shape[1]
    bufs = assoc.logit_buffers(f.A, K, c0, c1, f.M, f.W, want_theta, empty=_blocks(f, True))     # theta is None when it is not wanted
    y, Z, use = (f.put(v) for v in (y, Z, use))
    n_bad = ctypes.c_int64(0)
    rc = _call(f, "assoc_logit", f.ptr(y), f.ptr(Z), K, f.ptr(use), int(min_ac), c0, c1, tol, max_iter, *(f.ptr(b) for b in bufs),
               ctypes.byref(n_bad), row_kind=False)
    verdict(f.ctx, rc, n_bad.value, check, handed=(_lib.GNX_EINVAL,))     # (a phenotype that is not 0 / 1 is GNX_EINVAL too: n_bad tells)
    return assoc.split_logit(*(f.host(b) for b in bufs), f.A, K, c0, c1, f.M, f.W, n_bad.value)


# ---- admixture mapping: the labels alone, no rows and no model ------------------------------------------------------------------------
def admixmap_stats(ctx, labels, A, Y, Z, use, w0=0, w1=None, check=True):
    """gnx_ancestry_admixmap[_dev] for the windows [w0, w1) -> admixmap.AdmixStats of numpy arrays.  labels (N, W) int32: a numpy array
    (contiguous rows, any row stride) or a CUDA tensor (the same), which never leaves HBM: Y, Z and use then go to its device and the
    blocks are allocated there.  Y (N / 2, T) float64 may have any row stride too."""
    from . import admixmap
    dev = hasattr(labels, "is_cuda")
    if dev:
        import torch
        if labels.dim() != 2:
            raise ValueError(f"labels must be (N, W), got {tuple(labels.shape)}")
        lab = labels if labels.dtype == torch.int32 and (labels.shape[1] == 0 or labels.stride(1) == 1) else labels.to(torch.int32).contiguous()
        N, W = lab.shape
        ldl = lab.stride(0) if N > 1 else W
    else:
        lab = np.asarray(labels)
        if lab.ndim != 2 or lab.dtype != np.int32 or (lab.shape[1] and lab.strides[1] != 4) or lab.strides[0] % 4 or lab.strides[0] < 4 * lab.shape[1]:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim != 2:
            raise ValueError(f"labels must be (N, W), got {lab.shape}")
        N, W = lab.shape
        ldl = lab.strides[0] // 4 if N > 1 else W
    check_even(N)
    w0, w1 = int(w0), int(W) if w1 is None else int(w1)
    Ya = np.asarray(Y)
    strided = Ya.ndim == 2 and Ya.dtype == np.float64 and Ya.shape[1] and Ya.strides[1] == 8 and Ya.strides[0] % 8 == 0 and Ya.strides[0] >= 8 * Ya.shape[1]
    Yc, Z, use, _ = assoc.trait_covariates(N // 2, Y, Z, use)
    if strided and not dev:
        Yc = Ya                                    # the caller's row stride goes to the library as it is
    K, T = Z.shape[1], Yc.shape[1]
    ldy = Yc.strides[0] // 8 if N // 2 > 1 else T
    n_bad = ctypes.c_int64(0)
    if dev:
        import torch
        dtypes = {np.int32: torch.int32, np.float64: torch.float64}
        bufs = admixmap.stats_buffers(int(A), K, T, w0, w1, empty=lambda shape, dtype: torch.empty(shape, dtype=dtypes[dtype], device=lab.device))
        Yd, Zd, ud = (torch.from_numpy(np.ascontiguousarray(v)).to(lab.device) for v in (Yc, Z, use))
        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
        rc = ctx.lib.gnx_ancestry_admixmap_dev(ctx.h, lab.data_ptr(), ldl, N, W, int(A), Yd.data_ptr(), T, T, Zd.data_ptr(), K, ud.data_ptr(), w0, w1,
                                               *(b.data_ptr() for b in bufs), ctypes.byref(n_bad))
        verdict(ctx, rc, n_bad.value, check, handed=(_lib.GNX_EINVAL,))
        bufs = [b.cpu().numpy() for b in bufs]
    else:
        bufs = admixmap.stats_buffers(int(A), K, T, w0, w1)
        rc = ctx.lib.gnx_ancestry_admixmap(ctx.h, lab.ctypes.data, ldl, N, W, int(A), Yc.ctypes.data, ldy, T, Z.ctypes.data, K, use.ctypes.data, w0, w1,
                                           *(b.ctypes.data for b in bufs), ctypes.byref(n_bad))
        verdict(ctx, rc, n_bad.value, check, handed=(_lib.GNX_EINVAL,))
    return admixmap.split_blocks(*bufs, int(A), K, T, n_bad.value)


# ---- DeviceModel's half ----------------------------------------------------------------------------------------------------------------
class AncestryOps:
    """the ancestry-specific methods of DeviceModel (which supplies ctx, lib, h, C, M, W, A, _x, _gt2_args, _bind_torch_stream).  The
    numpy forms take X (N, C) int8 (packed=True: the 2-bit rows pack_x returns) and labels (N, W); the _device forms X_t int8 (N, C) or the
    uint8 tensor pack_device returns and lab_t (N, W) int32, contiguous rows with any row stride; the _gt2 forms the parsed query (G, N,
    src as infer_gt2 takes them) and host labels.  Labels must be exactly (N, self.W)."""

    def _host(self, X, labels, packed=False, even=False):
        return host_front(self.ctx, X, labels, self.M, self.A, packed, self.C, self.W, even)

    def _rows(self, X, labels):
        """the front of an op that takes numpy arrays or CUDA tensors under one name (the association ops: int8 rows only on the host)"""
        if hasattr(X, "is_cuda"):
            return device_front(self, X, labels)
        return host_front(self.ctx, self._x(X), labels, self.M, self.A, False, self.C, self.W, strided=True)

    def ancestry_summary(self, lab, weights=None, proba=None):
        """global ancestry and tract statistics of (N, W) labels (and (N, W, A) probabilities) on the device (gnx_ancestry_summary;
        gnomix_amd.postprocess.ancestry_summary) -> AncestrySummary of numpy arrays"""
        from .postprocess import ancestry_summary
        return ancestry_summary(self.ctx, lab, self.A, weights, proba)

    def ancestry_summary_device(self, lab_t, weights=None, proba_t=None):
        """the same on an (N, W) int32 CUDA tensor with contiguous rows (any row stride) and, optionally, a contiguous (N, W, A)
        float32 / float64 CUDA tensor (gnx_ancestry_summary_dev) -> AncestrySummary of CUDA tensors; the weights are a host array"""
        import torch
        assert lab_t.is_cuda and lab_t.dtype == torch.int32 and lab_t.dim() == 2 and (lab_t.shape[1] == 0 or lab_t.stride(1) == 1)
        N, W = lab_t.shape
        if proba_t is not None:
            assert proba_t.is_cuda and proba_t.dtype in (torch.float32, torch.float64) and proba_t.is_contiguous()
            if tuple(proba_t.shape) != (N, W, self.A):
                raise ValueError(f"proba must be (N={N}, W={W}, A={self.A}), got {tuple(proba_t.shape)}")
        w = _summary_weights(weights, W)
        self._bind_torch_stream()
        new = lambda dt: torch.zeros((N, self.A), dtype=dt, device=lab_t.device)
        hard, total, longest, count = new(torch.float64), new(torch.float64), new(torch.float64), new(torch.int32)
        soft = new(torch.float64) if proba_t is not None else None
        self.ctx.check(self.lib.gnx_ancestry_summary_dev(
            self.ctx.h, lab_t.data_ptr(), lab_t.stride(0) if N > 1 else W, proba_t.data_ptr() if proba_t is not None else None,
            int(proba_t is not None and proba_t.dtype == torch.float64), w.ctypes.data, N, W, self.A, hard.data_ptr(),
            soft.data_ptr() if soft is not None else None, count.data_ptr(), total.data_ptr(), longest.data_ptr()))
        return AncestrySummary(hard, soft, count, total, longest, w)

    # ---- admixture mapping (the labels alone)
    def admixture_map_stats(self, labels, Y, Z=None, use=None, w0=0, w1=None, check=True):
        """the blocks of admixture mapping for the windows [w0, w1) of (N, W) host labels (gnx_ancestry_admixmap, the float64 matrix
        cores; include/gnomix_hip.h states them) -> gnomix_amd.admixmap.AdmixStats"""
        return admixmap_stats(self.ctx, check_labels(labels, np.asarray(labels).shape[0], self.W), self.A, Y, Z, use, w0, w1, check)

    def admixture_map_stats_device(self, lab_t, Y, Z=None, use=None, w0=0, w1=None, check=True):
        """the same on an (N, W) int32 CUDA tensor with contiguous rows (any row stride): the labels stay in HBM
        (gnx_ancestry_admixmap_dev) -> admixmap.AdmixStats of numpy arrays"""
        return admixmap_stats(self.ctx, check_labels(lab_t, lab_t.shape[0], self.W), self.A, Y, Z, use, w0, w1, check)

    def admixture_map(self, labels, Y, Z=None, use=None, min_hap=1, n_perm=0, seed=0, check=True):
        """admixture mapping of the traits Y on (N, W) labels, a numpy array or a CUDA tensor (gnomix_amd.admixmap.admixture_mapping states
        the model, the permutations and the result) -> admixmap.AdmixMap"""
        from . import admixmap
        return admixmap.admixture_mapping(self.ctx, check_labels(labels, labels.shape[0], self.W), self.A, Y, Z, use, min_hap, n_perm, seed, check)

    # ---- allele counts and dosage
    def ancestry_allele_counts(self, X, labels, packed=False):
        """ancestry-specific allele counts of X (N, C) int8 (packed=True: the 2-bit rows pack_x returns) under (N, W) labels, on the
        device (gnx_ancestry_allele_counts; gnomix_amd.postprocess.allele_counts) -> AlleleCounts of (A, C) int32 arrays"""
        return allele_counts(self._host(X, labels, packed))

    def ancestry_allele_counts_device(self, X_t, lab_t):
        """the same on CUDA tensors: X_t int8 (N, C) or the uint8 tensor pack_device returns, lab_t (N, W) int32 with any row stride
        (gnx_ancestry_allele_counts_dev) -> AlleleCounts of (A, C) int32 CUDA tensors"""
        return allele_counts(device_front(self, X_t, lab_t))

    def allele_counts_gt2(self, G, N, src, labels):
        """ancestry-specific allele counts of the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the
        packed rows are built and counted in HBM, batch by batch (gnx_ancestry_allele_counts_gt2) -> AlleleCounts"""
        return allele_counts(gt2_front(self, G, N, src, labels))

    def ancestry_dosage(self, X, labels, ancestry, packed=False):
        """(dosage, hapcount) of one ancestry, (N / 2, C) uint8 each (gnx_ancestry_dosage; gnomix_amd.postprocess.ancestry_dosage)"""
        return dosage(self._host(X, labels, packed), ancestry)

    def ancestry_dosage_device(self, X_t, lab_t, ancestry):
        """(dosage, hapcount) uint8 (N / 2, C) CUDA tensors of one ancestry (gnx_ancestry_dosage_dev)"""
        return dosage(device_front(self, X_t, lab_t), ancestry)

    # ---- scores
    def ancestry_scores(self, X, labels, weights, effect=None, packed=False):
        """ancestry-partitioned polygenic scores of X (N, C) int8 (packed=True: the 2-bit rows pack_x returns) under (N, W) labels, on the
        device (gnx_ancestry_score; gnomix_amd.postprocess.ancestry_scores) -> AncestryScores of numpy arrays.  weights (C,), (C, A) or
        (C, A, S) float64; effect None (ALT everywhere) or (C,) of 1 (ALT), 0 (REF), 255 (not scored)"""
        return scores(self._host(X, labels, packed, even=True), *score_tables(weights, effect, self.C, self.A))

    def ancestry_scores_device(self, X_t, lab_t, weights, effect=None):
        """the same on CUDA tensors: X_t int8 (N, C) or the uint8 tensor pack_device returns, lab_t (N, W) int32 with any row stride;
        weights and effect as numpy arrays or CUDA tensors (gnx_ancestry_score_dev) -> AncestryScores of CUDA tensors"""
        import torch
        f = device_front(self, X_t, lab_t, even=True)
        dev = X_t.device
        if hasattr(weights, "is_cuda") and (effect is None or hasattr(effect, "is_cuda")):     # tables that are tensors stay tensors
            w_t = weights.to(device=dev, dtype=torch.float64)
            w_t = w_t[:, None].expand(-1, self.A)[:, :, None] if w_t.dim() == 1 else w_t[:, :, None] if w_t.dim() == 2 else w_t
            if w_t.dim() != 3 or tuple(w_t.shape[:2]) != (self.C, self.A) or w_t.shape[2] < 1:
                raise ValueError(f"weights must be (C={self.C},), (C, A={self.A}) or (C, A, S >= 1), got {tuple(weights.shape)}")
            w_t = w_t.contiguous()
            e_t = torch.ones(self.C, dtype=torch.uint8, device=dev) if effect is None else effect.to(device=dev, dtype=torch.uint8).contiguous()
            if tuple(e_t.shape) != (self.C,):
                raise ValueError(f"effect must be (C={self.C},), got {tuple(e_t.shape)}")
        else:
            to_host = lambda v: v.cpu().numpy() if hasattr(v, "is_cuda") else v
            w_t, e_t = (f.put(v) for v in score_tables(to_host(weights), None if effect is None else to_host(effect), self.C, self.A))
        return scores(f, w_t, e_t)

    def ancestry_scores_gt2(self, G, N, src, labels, weights, effect=None):
        """ancestry_scores of the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the packed rows are built and
        scored in HBM, batch of individuals by batch (gnx_ancestry_score_gt2) -> AncestryScores of numpy arrays"""
        return scores(gt2_front(self, G, N, src, labels, even=True), *score_tables(weights, effect, self.C, self.A))

    # ---- pair counts and LD counts (check: the host forms only; the others always raise on a label out of range)
    def ancestry_pair_counts(self, X, labels, ancestry, snp_range=None, packed=False):
        """the pairwise count tables DD, DO, OO of one ancestry over the SNPs snp_range = (c0, c1) (None: all), X (N, C) int8
        (packed=True: the 2-bit rows pack_x returns) under (N, W) labels, on the int8 matrix cores (gnx_ancestry_pair_counts;
        gnomix_amd.postprocess.pair_counts) -> asmds.PairCounts of (N / 2, N / 2) int32 arrays"""
        return pair_counts(self._host(X, labels, packed, even=True), ancestry, snp_range)

    def ancestry_pair_counts_device(self, X_t, lab_t, ancestry, snp_range=None, debug_snps_per_block=0):
        """the same on CUDA tensors: X_t int8 (N, C) or the uint8 tensor pack_device returns, lab_t (N, W) int32 with any row stride
        (gnx_ancestry_pair_counts_dev) -> asmds.PairCounts of (N / 2, N / 2) int32 CUDA tensors"""
        return pair_counts(device_front(self, X_t, lab_t, even=True), ancestry, snp_range, debug_snps_per_block)

    def ancestry_pair_counts_gt2(self, G, N, src, labels, ancestry, snp_range=None):
        """ancestry_pair_counts of the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the whole packed matrix is
        built in HBM and the kernel runs once (gnx_ancestry_pair_counts_gt2) -> asmds.PairCounts of numpy arrays"""
        return pair_counts(gt2_front(self, G, N, src, labels, even=True), ancestry, snp_range)

    def ancestry_ld_counts(self, X, labels, ancestry, c0=0, c1=None, band=256, packed=False):
        """the banded LD count tables n11, n1o, no1, noo of one ancestry for the SNPs [c0, c1) and the offsets 0 .. band - 1, X (N, C) int8
        (packed=True: the 2-bit rows pack_x returns) under (N, W) labels, on the int8 matrix cores (gnx_ancestry_ld_counts;
        gnomix_amd.postprocess.ld_counts) -> ld.LDCounts of (c1 - c0, band) int32 arrays"""
        return ld_counts(self._host(X, labels, packed), ancestry, c0, c1, band)

    def ancestry_ld_counts_device(self, X_t, lab_t, ancestry, c0=0, c1=None, band=256, debug_haps_per_block=0):
        """the same on CUDA tensors: X_t int8 (N, C) or the uint8 tensor pack_device returns, lab_t (N, W) int32 with any row stride
        (gnx_ancestry_ld_counts_dev) -> ld.LDCounts of (c1 - c0, band) int32 CUDA tensors"""
        return ld_counts(device_front(self, X_t, lab_t), ancestry, c0, c1, band, debug_haps_per_block)

    def ancestry_ld_counts_gt2(self, G, N, src, labels, ancestry, c0=0, c1=None, band=256):
        """ancestry_ld_counts of the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the whole packed matrix is
        built in HBM and the kernel runs once (gnx_ancestry_ld_counts_gt2) -> ld.LDCounts of numpy arrays"""
        return ld_counts(gt2_front(self, G, N, src, labels), ancestry, c0, c1, band)

    # ---- linear association
    def ancestry_assoc_stats(self, X, labels, y, Z=None, use=None, c0=0, c1=None, min_ac=1, check=True):
        """the sufficient statistics of the ancestry-specific association model for the SNPs [c0, c1) (gnx_ancestry_assoc_stats[_dev];
        include/gnomix_hip.h states the blocks) -> gnomix_amd.assoc.AssocStats of numpy arrays.  X (N, C) int8 and labels (N, W) int32 as
        numpy arrays, or as CUDA tensors (X int8 or the uint8 tensor pack_device returns, labels with any row stride): those never leave
        HBM.  check=False: labels out of range do not raise, their count is AssocStats.n_bad."""
        return assoc_stats(self._rows(X, labels), y, Z, use, *snp_bounds(c0, c1, self.C), min_ac, check)

    def ancestry_assoc_stats_gt2(self, G, N, src, labels, y, Z=None, use=None, c0=0, c1=None, min_ac=1, check=True):
        """ancestry_assoc_stats of the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the packed rows are
        built and reduced in HBM, batch of individuals by batch (gnx_ancestry_assoc_stats_gt2) -> assoc.AssocStats of [c0, c1)"""
        return assoc_stats(gt2_front(self, G, N, src, labels), y, Z, use, *snp_bounds(c0, c1, self.C), min_ac, check)

    def ancestry_assoc(self, X, labels, y, Z=None, use=None, min_ac=1):
        """ancestry-specific association (the Tractor model: y = Z g + sum_{a < A-1} alpha_a hapcount_a + sum_a beta_a dosage_a, OLS per
        SNP over the individuals that take part) -> gnomix_amd.assoc.AncestryAssoc.  y (N / 2,), Z (N / 2, K) float64 with the intercept
        column (None = the intercept only), use (N / 2,) (0 = takes no part).  The device reduces X and the labels to per-SNP blocks, chunk
        of SNPs by chunk (gnx_ancestry_assoc_stats); the host factors them (gnomix_amd/assoc.py).  X and labels: numpy arrays or CUDA
        tensors, as ancestry_assoc_stats takes them."""
        return self._assoc(X.shape[0] // 2, y, Z, use, min_ac, lambda y, Z, use, c0, c1: self.ancestry_assoc_stats(X, labels, y, Z, use, c0, c1, min_ac))

    def ancestry_assoc_gt2(self, G, N, src, labels, y, Z=None, use=None, min_ac=1):
        """ancestry_assoc of the parsed query under host labels (the command line's path) -> assoc.AncestryAssoc"""
        return self._assoc(int(N) // 2, y, Z, use, min_ac,
                           lambda y, Z, use, c0, c1: self.ancestry_assoc_stats_gt2(G, N, src, labels, y, Z, use, c0, c1, min_ac))

    def _assoc(self, n_ind, y, Z, use, min_ac, stats):
        if min_ac < 1:
            raise ValueError("min_ac must be >= 1")
        y, Z, use = assoc.covariates(n_ind, y, Z, use)
        return assoc.assoc_from_stats(lambda c0, c1: stats(y, Z, use, c0, c1), self.C, self.A, Z.shape[1], min_ac)

    # ---- many traits at once
    def ancestry_assoc_traits_stats(self, X, labels, Y, Z=None, use=None, c0=0, c1=None, min_ac=1, check=True):
        """the trait-dependent blocks of T quantitative traits for the SNPs [c0, c1) (gnx_ancestry_assoc_traits[_dev], the float64 matrix
        cores; include/gnomix_hip.h states them) -> gnomix_amd.assoc.TraitStats of numpy arrays.  Y (N / 2, T); X and labels as
        ancestry_assoc_stats takes them (numpy arrays, or CUDA tensors that never leave HBM).  check=False: labels out of range do not
        raise, their count is TraitStats.n_bad."""
        return assoc_traits(self._rows(X, labels), Y, Z, use, *snp_bounds(c0, c1, self.C), min_ac, check)

    def ancestry_assoc_traits_stats_gt2(self, G, N, src, labels, Y, Z=None, use=None, c0=0, c1=None, min_ac=1, check=True):
        """ancestry_assoc_traits_stats of the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the packed rows
        are built and reduced in HBM, batch of whole groups of 4 individuals by batch (gnx_ancestry_assoc_traits_gt2) -> assoc.TraitStats"""
        return assoc_traits(gt2_front(self, G, N, src, labels), Y, Z, use, *snp_bounds(c0, c1, self.C), min_ac, check)

    def _traits_chunks(self, n_ind, Y, Z, use, min_ac, p_max, chunk_bytes, stats, traits):
        """per chunk of SNPs the trait-independent blocks come from the linear op with a zero phenotype under use2 (complete cases across
        the traits), the trait-dependent ones from the traits op under use (which applies the same rule itself)"""
        if min_ac < 1:
            raise ValueError("min_ac must be >= 1")
        Y, Z, use, use2 = assoc.trait_covariates(n_ind, Y, Z, use)
        y0 = np.zeros(n_ind)
        return assoc.traits_chunks(lambda c0, c1: (stats(y0, Z, use2, c0, c1), traits(Y, Z, use, c0, c1)), self.C, self.A, Z.shape[1], Y.shape[1],
                                   min_ac, p_max, chunk_bytes)

    def ancestry_assoc_traits_chunks(self, X, labels, Y, Z=None, use=None, min_ac=1, p_max=None, chunk_bytes=None, check=True):
        """ancestry-specific association (the Tractor model, as ancestry_assoc states it) of T quantitative traits Y (N / 2, T) at once: a
        generator of (c0, c1, gnomix_amd.assoc.AncestryAssocTraits) per chunk of SNPs, beta, se, t, p shaped (c1 - c0, A, T).  An
        individual takes part when use says so, Z[i, :] is finite and EVERY trait of Y[i, :] is finite (complete cases across the batch;
        group traits by missingness pattern and call once per group).  Per chunk the device computes D^T Y on the float64 matrix cores
        (gnx_ancestry_assoc_traits) and the trait-independent blocks once (gnx_ancestry_assoc_stats with a zero phenotype); the host
        factors each SNP's normal matrix once and solves all T traits.  The chunks are sized so that the device blocks and the results
        of one chunk stay below chunk_bytes (default assoc.STATS_CHUNK_BYTES): the full result is never materialised here.  p_max: the
        float results of every (SNP, ancestry, trait) whose p is not <= p_max are NaN.  X and labels: numpy arrays or CUDA tensors.
        check=False: labels out of range do not raise (such an individual takes no part at that window)."""
        return self._traits_chunks(X.shape[0] // 2, Y, Z, use, min_ac, p_max, chunk_bytes,
                                   lambda y, Z, use, c0, c1: self.ancestry_assoc_stats(X, labels, y, Z, use, c0, c1, min_ac, check),
                                   lambda Y, Z, use, c0, c1: self.ancestry_assoc_traits_stats(X, labels, Y, Z, use, c0, c1, min_ac, check))

    def ancestry_assoc_traits_gt2_chunks(self, G, N, src, labels, Y, Z=None, use=None, min_ac=1, p_max=None, chunk_bytes=None):
        """ancestry_assoc_traits_chunks of the parsed query under host labels (the command line's path)"""
        return self._traits_chunks(int(N) // 2, Y, Z, use, min_ac, p_max, chunk_bytes,
                                   lambda y, Z, use, c0, c1: self.ancestry_assoc_stats_gt2(G, N, src, labels, y, Z, use, c0, c1, min_ac),
                                   lambda Y, Z, use, c0, c1: self.ancestry_assoc_traits_stats_gt2(G, N, src, labels, Y, Z, use, c0, c1, min_ac))

    def ancestry_assoc_traits(self, X, labels, Y, Z=None, use=None, min_ac=1, p_max=None, max_bytes=2 << 30, check=True):
        """the chunks of ancestry_assoc_traits_chunks concatenated -> assoc.AncestryAssocTraits of all C SNPs.  ValueError naming the byte
        count, before any work, when the result would exceed max_bytes (chr22 x 7 ancestries x 1024 traits is 18 GB per field)."""
        T = np.asarray(Y).shape[1] if np.asarray(Y).ndim == 2 else 0
        return assoc.traits_concat(self.ancestry_assoc_traits_chunks(X, labels, Y, Z, use, min_ac, p_max, check=check), self.C, self.A, T, max_bytes)

    def ancestry_assoc_traits_gt2(self, G, N, src, labels, Y, Z=None, use=None, min_ac=1, p_max=None, max_bytes=2 << 30):
        """ancestry_assoc_traits of the parsed query under host labels -> assoc.AncestryAssocTraits; ValueError above max_bytes"""
        T = np.asarray(Y).shape[1] if np.asarray(Y).ndim == 2 else 0
        return assoc.traits_concat(self.ancestry_assoc_traits_gt2_chunks(G, N, src, labels, Y, Z, use, min_ac, p_max), self.C, self.A, T, max_bytes)

    # ---- logistic association
    def ancestry_assoc_logit_fit(self, X, labels, y, Z=None, use=None, c0=0, c1=None, min_ac=1, tol=None, max_iter=None, check=True):
        """the logistic fits of the SNPs [c0, c1) (gnx_ancestry_assoc_logit[_dev]; include/gnomix_hip.h states the model and the iteration)
        -> gnomix_amd.assoc.LogitFit of numpy arrays.  X and labels as ancestry_assoc_stats takes them (numpy arrays, or CUDA tensors
        that never leave HBM).  check=False: labels out of range do not raise, their count is LogitFit.n_bad."""
        return assoc_logit(self._rows(X, labels), y, Z, use, *snp_bounds(c0, c1, self.C), min_ac, tol, max_iter, check)

    def ancestry_assoc_logit_fit_gt2(self, G, N, src, labels, y, Z=None, use=None, c0=0, c1=None, min_ac=1, tol=None, max_iter=None, check=True):
        """ancestry_assoc_logit_fit of the parsed query (G, N, src as infer_gt2 takes them) under host labels (N, W): the packed rows of
        all individuals are built in HBM and fitted there (gnx_ancestry_assoc_logit_gt2) -> assoc.LogitFit of [c0, c1)"""
        return assoc_logit(gt2_front(self, G, N, src, labels), y, Z, use, *snp_bounds(c0, c1, self.C), min_ac, tol, max_iter, check)

    def _logit(self, n_ind, y, Z, use, min_ac, fit):
        if min_ac < 1:
            raise ValueError("min_ac must be >= 1")
        y, Z, use = assoc.covariates(n_ind, y, Z, use)
        assoc.check_binary(y, use)
        return assoc.logit_from_fits(lambda c0, c1: fit(y, Z, use, c0, c1), self.C, self.A, Z.shape[1])

    def ancestry_assoc_logit(self, X, labels, y, Z=None, use=None, min_ac=1, tol=None, max_iter=None):
        """ancestry-specific association of a case / control trait (the Tractor model with a logit link: logit P(y = 1) = Z g +
        sum_{a < A-1} alpha_a hapcount_a + sum_a beta_a dosage_a, maximum likelihood per SNP over the individuals that take part, fitted
        on the device: k_ancestry_assoc_logit_snp) -> gnomix_amd.assoc.AncestryAssocLogit.  y (N / 2,) coded 0 / 1, Z, use as
        ancestry_assoc takes them; X and labels numpy arrays or CUDA tensors.  The SNPs are walked in chunks whose outputs stay below
        assoc.STATS_CHUNK_BYTES."""
        return self._logit(X.shape[0] // 2, y, Z, use, min_ac,
                           lambda y, Z, use, c0, c1: self.ancestry_assoc_logit_fit(X, labels, y, Z, use, c0, c1, min_ac, tol, max_iter))

    def ancestry_assoc_logit_gt2(self, G, N, src, labels, y, Z=None, use=None, min_ac=1, tol=None, max_iter=None):
        """ancestry_assoc_logit of the parsed query under host labels (the command line's path) -> assoc.AncestryAssocLogit"""
        return self._logit(int(N) // 2, y, Z, use, min_ac,
                           lambda y, Z, use, c0, c1: self.ancestry_assoc_logit_fit_gt2(G, N, src, labels, y, Z, use, c0, c1, min_ac, tol, max_iter))
