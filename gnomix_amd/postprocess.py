"""Writers on the output side of the hot path: window metadata, .msp, .fb (+ .lai, .bed).

Mirrors the reference's src/postprocess.py:25-210 byte for byte (pinned by tests/golden/G6_writers, produced by
running the reference's own get_meta_data / write_msp / write_fb).  The two big tables (.msp labels, .fb probabilities) are
formatted and written by the library (include/gnomix_io.h: gnx_write_msp / gnx_write_fb, all host cores); the window
metadata (W rows) is plain numpy.  No pandas needed."""
from __future__ import annotations

import collections
import os

import numpy as np

from . import _lib


def _fmt(v):
    """str() of a numpy scalar the way `np.array([...mixed...]).astype(str)` / pandas print it: shortest repr"""
    if isinstance(v, (np.floating, float)):
        return str(np.float64(v)) if not isinstance(v, np.float32) else str(v)
    return str(v)


def get_meta_data(chm, model_pos, query_pos, n_wind, wind_size, gen_map_pos, gen_map_cm):
    """Window table of the .msp/.fb files (postprocess.py:25-67): columns chm, spos, epos, sgpos, egpos, "n snps".
    Returns a dict of equal-length lists/arrays (a stand-in for the reference's DataFrame)."""
    model_pos = np.asarray(model_pos)
    query_pos = np.asarray(query_pos)
    C = len(model_pos)
    idx = np.arange(0, C, wind_size)
    spos_idx = idx[:-1]
    epos_idx = np.concatenate([idx[1:-1], np.array([C])]) - 1
    spos, epos = model_pos[spos_idx], model_pos[epos_idx]
    gpos = np.asarray(gen_map_pos, dtype=float)
    gcm = np.asarray(gen_map_cm, dtype=float)

    def interp(x):  # linear interpolation, ends clamped to the first/last cM (interp1d(fill_value=end_pts))
        x = np.asarray(x, dtype=float)
        k = np.clip(np.searchsorted(gpos, x, side="left"), 1, len(gpos) - 1)  # interp1d: x_new in (x[k-1], x[k]]
        lo, hi = k - 1, k
        slope = (gcm[hi] - gcm[lo]) / (gpos[hi] - gpos[lo])
        y = slope * (x - gpos[lo]) + gcm[lo]
        y = np.where(x < gpos[0], gcm[0], y)
        y = np.where(x > gpos[-1], gcm[-1], y)
        return y

    sgpos = np.round(interp(spos), 5)
    egpos = np.round(interp(epos), 5)
    n_snps = np.zeros_like(epos)
    if len(query_pos) < 2 or bool(np.all(query_pos[1:] >= query_pos[:-1])):
        # the reference's running pointer (postprocess.py:56-62) on sorted positions = counts between successive window ends
        # (the pointer never moves backwards: a window end below its predecessor adds nothing)
        cut = np.maximum.accumulate(np.searchsorted(query_pos, epos[:n_wind - 1], side="right")) if n_wind > 1 else np.zeros(0, int)
        n_snps[:n_wind - 1] = np.diff(np.concatenate([[0], cut]))
        q = int(cut[-1]) if n_wind > 1 else 0
    else:
        q = 0
        for w in range(n_wind - 1):
            while q < len(query_pos) and query_pos[q] <= epos[w]:
                n_snps[w] += 1
                q += 1
    n_snps[n_wind - 1] = len(query_pos) - q
    return {"chm": [chm] * n_wind, "spos": spos, "epos": epos, "sgpos": sgpos, "egpos": egpos, "n snps": n_snps}


META_COLUMNS = ["chm", "spos", "epos", "sgpos", "egpos", "n snps"]


def _meta_strings(meta):
    n = len(meta["spos"])
    return [[_fmt(meta[c][i]) for c in META_COLUMNS] for i in range(n)]


def _blob(rows):
    enc = [r.encode() for r in rows]
    off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        np.cumsum([len(e) for e in enc], out=off[1:])
    return b"".join(enc), off


def write_msp(msp_prefix, meta_data, pred_labels, populations, query_samples, n_threads=0):
    """<prefix>.msp (postprocess.py:84-98): pred_labels (N, W) ints, haplotype columns sample.0 / sample.1.  The header and
    the W metadata prefixes are built here; the N x W label text is produced by the library on all host cores."""
    rows = ["\t".join(r) for r in _meta_strings(meta_data)]
    lab = np.ascontiguousarray(pred_labels, dtype=np.int32)
    head = "#Subpopulation order/codes: " + "\t".join([str(pop) + "=" + str(i) for i, pop in enumerate(populations)]) + "\n"
    head += "#" + "\t".join(META_COLUMNS) + "\t"
    head += "\t".join([str(s) for q in query_samples for s in (str(q) + ".0", str(q) + ".1")]) + "\n"
    head = head.encode()
    pb, po = _blob(rows)
    if lab.ndim != 2 or lab.shape[1] != len(rows):
        raise ValueError(f"pred_labels must be (N, W={len(rows)}), got {lab.shape}")
    _lib.io_check(_lib.load().gnx_write_msp((msp_prefix + ".msp").encode(), head, len(head), pb, po.ctypes.data, lab.ctypes.data,
                                            lab.shape[0], lab.shape[1], lab.shape[1], int(n_threads)))


Msp = collections.namedtuple("Msp", "labels populations samples meta")
Msp.__doc__ = """what read_msp returns: labels (N, W) int32 (rows 2 i and 2 i + 1 are samples[i]); the populations in code order; the samples; meta:
the window table as write_msp takes it (chm: strings; spos, epos, n snps: int64; sgpos, egpos: float64)"""


def read_msp(path):
    """the inverse of write_msp, in plain Python / numpy: <prefix>.msp -> Msp.  With it admixmap.admixture_mapping runs from an .msp alone:
    no model, no VCF."""
    with open(path) as f:
        first = f.readline().rstrip("\n")
        second = f.readline().rstrip("\n")
        body = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    if ":" not in first or not first.startswith("#") or not second.startswith("#"):
        raise ValueError(f"{path}: not an .msp file (two header lines starting with '#')")
    pops = {}
    for cell in first.split(":", 1)[1].strip().split("\t"):
        name, _, code = cell.rpartition("=")
        pops[int(code)] = name
    if sorted(pops) != list(range(len(pops))):
        raise ValueError(f"{path}: the population codes are not 0 .. {len(pops) - 1}")
    cols = second[1:].split("\t")
    nm = len(META_COLUMNS)
    if cols[:nm] != META_COLUMNS or (len(cols) - nm) % 2:
        raise ValueError(f"{path}: the second header line must hold {META_COLUMNS} and two columns per sample")
    haps = cols[nm:]
    samples = [h[:-2] for h in haps[0::2]]
    if any(a != s + ".0" or b != s + ".1" for s, a, b in zip(samples, haps[0::2], haps[1::2])):
        raise ValueError(f"{path}: the haplotype columns must come as <sample>.0, <sample>.1")
    if any(len(r) != len(cols) for r in body):
        raise ValueError(f"{path}: a line does not have {len(cols)} cells")
    W = len(body)
    labels = np.array([r[nm:] for r in body], dtype=np.int32).reshape(W, len(haps)).T
    meta = {"chm": [r[0] for r in body]}
    for j, (name, dt) in enumerate(zip(META_COLUMNS[1:], (np.int64, np.int64, np.float64, np.float64, np.int64)), 1):
        meta[name] = np.array([r[j] for r in body], dtype=np.float64).astype(dt) if W else np.zeros(0, dt)
    return Msp(np.ascontiguousarray(labels), [pops[i] for i in range(len(pops))], samples, meta)


def write_admixmap(prefix, meta_data, result, populations, trait_names=None):
    """<prefix>.admixmap.tsv from an admixmap.AdmixMap, or <prefix>.admixmap.<trait>.tsv per trait when trait_names is given: one header
    line, then one line per window: the .msp's window columns (chm, spos, epos, sgpos, egpos, n snps), the joint fields n, status, df1,
    df2, F, p_joint [, p_adj_F], then per population <pop>.n_hap, .beta, .se, .t, .p [, .p_adj] (the p_adj columns only for a result with
    permutations; floats with six significant digits, nan where the statistic is), tab-separated -> the paths written"""
    W, A, T = np.asarray(result.beta).shape
    if A != len(populations) or W != len(meta_data["spos"]):
        raise ValueError(f"the result holds {W} windows x {A} populations, the table {len(meta_data['spos'])} x {len(populations)}")
    if trait_names is None and T != 1:
        raise ValueError(f"a result of {T} traits needs trait_names")
    if trait_names is not None and len(trait_names) != T:
        raise ValueError(f"{len(trait_names)} trait names for {T} traits")
    perm = result.perm_max_t is not None
    num = lambda v: format(float(v), ".6g") if np.isfinite(v) else "nan"
    rows = _meta_strings(meta_data)
    head = ["#" + META_COLUMNS[0]] + META_COLUMNS[1:] + ["n", "status", "df1", "df2", "F", "p_joint"] + (["p_adj_F"] if perm else [])
    for p in populations:
        head += [str(p) + s for s in (".n_hap", ".beta", ".se", ".t", ".p") + ((".p_adj",) if perm else ())]
    paths = []
    for t in range(T):
        path = prefix + (".admixmap.tsv" if trait_names is None else ".admixmap.%s.tsv" % trait_names[t])
        with open(path, "w") as f:
            f.write("\t".join(head) + "\n")
            for k in range(W):
                cells = rows[k] + [str(int(result.n[k])), str(int(result.status[k])), str(int(result.df1[k])), str(int(result.df2[k])),
                                   num(result.F[k, t]), num(result.p_joint[k, t])] + ([num(result.p_adj_F[k, t])] if perm else [])
                for a in range(A):
                    cells += [str(int(result.n_hap[k, a])), num(result.beta[k, a, t]), num(result.se[k, a, t]), num(result.t[k, a, t]),
                              num(result.p[k, a, t])] + ([num(result.p_adj_t[k, a, t])] if perm else [])
                f.write("\t".join(cells) + "\n")
        paths.append(path)
    return paths


def write_fb(fb_prefix, meta_data, proba, ancestry, query_samples, n_threads=0, ctx=None):
    """<prefix>.fb (postprocess.py:100-126): proba (N, W, A); every value is printed as pandas' to_csv prints a float column
    (numpy's shortest round-trip text of the array's dtype) — by the library, W rows in parallel on the host's cores, or, when a
    context is given and the probabilities are float32, as text produced on the GPU (gnx_write_fb_dev: same bytes, one write())."""
    proba = np.asarray(proba)
    if proba.dtype not in (np.float32, np.float64):
        proba = proba.astype(np.float64)
    proba = np.ascontiguousarray(proba)
    n_rows = len(meta_data["spos"])
    if proba.ndim != 3 or proba.shape[1] != n_rows:
        raise ValueError(f"proba must be (N, W={n_rows}, A), got {proba.shape}")
    se = np.stack([np.asarray(meta_data["spos"]).astype(int), np.asarray(meta_data["epos"]).astype(int)], axis=1)
    pp = np.round(np.mean(se, axis=1)).astype(int)
    gp = np.mean(np.stack([np.asarray(meta_data["sgpos"], dtype=float), np.asarray(meta_data["egpos"], dtype=float)], 1), axis=1)
    header = ["chromosome", "physical position", "genetic_position", "genetic_marker_index"]
    header += [":::".join([str(q), h, str(a)]) for q in query_samples for h in ["hap1", "hap2"] for a in ancestry]
    head = ("#reference_panel_population:\t" + "\t".join([str(a) for a in ancestry]) + "\n" + "\t".join(header) + "\n").encode()
    rows = ["\t".join([str(meta_data["chm"][r]), str(pp[r]), _fmt(np.float64(gp[r])), "."]) for r in range(n_rows)]
    pb, po = _blob(rows)
    # (measured, chr22 x 10 000 haplotypes into tmpfs: 0.078-0.082 s either way — one thread putting 305 MB into a FRESH file costs
    #  0.052-0.056 s in the kernel's page cache whoever produced the text: scripts/dev/tmpfs_write_probe.py.  The GPU route is what a
    #  caller asks for with ctx=; the command line keeps the host writer unless GNX_FB_DEV=1)
    if ctx is not None and proba.dtype == np.float32 and proba.size > 0:
        ctx.check(ctx.lib.gnx_write_fb_dev(ctx.h, (fb_prefix + ".fb").encode(), head, len(head), pb, po.ctypes.data, proba.ctypes.data,
                                           proba.shape[0], n_rows, proba.shape[2]))
        return
    _lib.io_check(_lib.load().gnx_write_fb((fb_prefix + ".fb").encode(), head, len(head), pb, po.ctypes.data, proba.ctypes.data,
                                           int(proba.dtype == np.float64), proba.shape[0], n_rows, proba.shape[2], int(n_threads)))


def mode_filter(ctx, labels, A, size):
    """Smoother.predict's mode_filter (src/Smooth/utils.py:31-46) on (N, W) labels in [0, A), on the device (gnx_mode_filter):
    -> a new int32 array.  size 0 / None / False: the labels as they came, nothing launched."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 2:
        raise ValueError(f"labels must be (N, W), got {lab.shape}")
    if not size:
        return lab
    out = np.empty_like(lab)
    ctx.check(ctx.lib.gnx_mode_filter(ctx.h, lab.ctypes.data, out.ctypes.data, lab.shape[0], lab.shape[1], int(A), int(size)))
    return out


def label_runs(ctx, labels):
    """run-length encoding of every row of (N, W) labels on the device (gnx_label_runs): -> (counts (N,) int64, offsets (N + 1,)
    int64, triples (total, 3) int32 of (first_window, last_window, label)); row n owns triples offsets[n] .. offsets[n + 1] - 1"""
    import ctypes as C
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 2:
        raise ValueError(f"labels must be (N, W), got {lab.shape}")
    N, W = lab.shape
    counts, offsets, total = np.zeros(N, np.int64), np.zeros(N + 1, np.int64), C.c_int64(0)
    triples = np.empty((N * min(W, 8), 3), np.int32)   # room for 8 runs a row; the entry says how many there are when that is too few
    for _ in range(2):
        rc = ctx.lib.gnx_label_runs(ctx.h, lab.ctypes.data, W, N, W, counts.ctypes.data, offsets.ctypes.data, triples.ctypes.data,
                                    triples.shape[0], C.byref(total))
        if rc == _lib.GNX_EINVAL and total.value > triples.shape[0]:
            triples = np.empty((total.value, 3), np.int32)
            continue
        ctx.check(rc)
        break
    return counts, offsets, triples[:total.value]


WEIGHT_KINDS = ("cM", "bp", "snps")


def window_weights(meta, kind="cM"):
    """(W,) float64 weights of the windows from the table write_msp prints (get_meta_data): "cM" = egpos - sgpos, "bp" = epos - spos,
    "snps" = n snps"""
    if kind == "cM":
        return np.asarray(meta["egpos"], dtype=np.float64) - np.asarray(meta["sgpos"], dtype=np.float64)
    if kind == "bp":
        return (np.asarray(meta["epos"]).astype(np.int64) - np.asarray(meta["spos"]).astype(np.int64)).astype(np.float64)
    if kind == "snps":
        return np.asarray(meta["n snps"]).astype(np.float64)
    raise ValueError(f"window_weights: kind must be one of {WEIGHT_KINDS}, got {kind!r}")


class AncestrySummary:
    """what ancestry_summary returns: (N, A) arrays hard, soft (None without probabilities), tract_total, tract_longest (float64)
    and tract_count (int32), numpy arrays or CUDA tensors as the labels were; `weights` the (W,) float64 weights used"""
    __slots__ = ("hard", "soft", "tract_count", "tract_total", "tract_longest", "weights")

    def __init__(self, hard, soft, tract_count, tract_total, tract_longest, weights):
        self.hard, self.soft, self.tract_count = hard, soft, tract_count
        self.tract_total, self.tract_longest, self.weights = tract_total, tract_longest, weights


def _summary_weights(weights, W):
    if weights is None:
        return np.ones(W, np.float64)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (W,):
        raise ValueError(f"weights must be (W={W},), got {w.shape}")
    return w


def ancestry_summary(ctx, labels, A, weights=None, proba=None):
    """global ancestry proportions and tract statistics of (N, W) labels in [0, A) on the device (gnx_ancestry_summary):
    hard[n, a] = share of the weights of row n's windows labelled a; soft[n, a] = the weighted mean of proba[n, :, a] (proba (N, W, A)
    float32 / float64, optional); per ancestry the number of tracts, their total weight and the longest one -> AncestrySummary"""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 2:
        raise ValueError(f"labels must be (N, W), got {lab.shape}")
    N, W = lab.shape
    w = _summary_weights(weights, W)
    p = None
    if proba is not None:
        p = np.asarray(proba)
        if p.dtype not in (np.float32, np.float64):
            p = p.astype(np.float64)
        p = np.ascontiguousarray(p)
        if p.shape != (N, W, int(A)):
            raise ValueError(f"proba must be (N={N}, W={W}, A={A}), got {p.shape}")
    hard, total, longest = (np.zeros((N, int(A)), np.float64) for _ in range(3))
    soft = np.zeros((N, int(A)), np.float64) if p is not None else None
    count = np.zeros((N, int(A)), np.int32)
    ctx.check(ctx.lib.gnx_ancestry_summary(ctx.h, lab.ctypes.data, W, p.ctypes.data if p is not None else None,
                                           int(p is not None and p.dtype == np.float64), w.ctypes.data, N, W, int(A), hard.ctypes.data,
                                           soft.ctypes.data if soft is not None else None, count.ctypes.data, total.ctypes.data,
                                           longest.ctypes.data))
    return AncestrySummary(hard, soft, count, total, longest, w)


def _individuals(rows):
    """(N, A) haplotype rows -> (N / 2, A): the mean of each individual's two rows"""
    return (rows[0::2] + rows[1::2]) / 2


def write_q(prefix, proportions, populations, samples, kind="hard calls", weights="cM"):
    """<prefix>.Q: global ancestry per individual.  proportions (2 * len(samples), A) haplotype rows (AncestrySummary.hard or
    .soft); an individual's value is the mean of its two rows, printed with five decimals"""
    q = np.asarray(proportions, dtype=np.float64)
    if q.ndim != 2 or q.shape != (2 * len(samples), len(populations)):
        raise ValueError(f"proportions must be (2 * {len(samples)} haplotypes, {len(populations)} populations), got {q.shape}")
    q = _individuals(q)
    with open(prefix + ".Q", "w") as f:
        f.write("#global ancestry, %s, weights: %s\n" % (kind, weights))
        f.write("#sample\t" + "\t".join(str(p) for p in populations) + "\n")
        for s, row in zip(samples, q):
            f.write(str(s) + "\t" + "\t".join("%.5f" % v for v in row) + "\n")


def write_tracts(prefix, summary, populations, samples):
    """<prefix>.tracts.tsv: one line per haplotype (0, then 1) and ancestry (population order): number of tracts, their total
    weight, the longest and the mean one (0 without tracts), lengths with five decimals"""
    cnt, tot, lng = np.asarray(summary.tract_count), np.asarray(summary.tract_total), np.asarray(summary.tract_longest)
    if cnt.shape != (2 * len(samples), len(populations)):
        raise ValueError(f"the summary must hold (2 * {len(samples)} haplotypes, {len(populations)} populations), got {cnt.shape}")
    with open(prefix + ".tracts.tsv", "w") as f:
        f.write("sample\thaplotype\tancestry\tn_tracts\ttotal_cM\tlongest_cM\tmean_cM\n")
        for i, s in enumerate(samples):
            for h in (0, 1):
                for a, pop in enumerate(populations):
                    n, t = int(cnt[2 * i + h, a]), float(tot[2 * i + h, a])
                    f.write("%s\t%d\t%s\t%d\t%.5f\t%.5f\t%.5f\n" % (s, h, pop, n, t, float(lng[2 * i + h, a]), t / n if n else 0.0))


class AlleleCounts(collections.namedtuple("AlleleCounts", "n_obs n_alt n_miss")):
    """what allele_counts returns: three (A, C) int32 tables (numpy arrays or CUDA tensors as the rows were).  Per ancestry a and
    SNP c, over the haplotypes whose label at c's window is a: n_obs = called (0 or 1), n_alt = ALT (1), n_miss = missing"""
    __slots__ = ()

    def freq(self):
        """n_alt / n_obs as float64 (A, C) numpy array, NaN where n_obs == 0"""
        obs = np.asarray(_to_host(self.n_obs), dtype=np.float64)
        alt = np.asarray(_to_host(self.n_alt), dtype=np.float64)
        out = np.full(obs.shape, np.nan, dtype=np.float64)
        np.divide(alt, obs, out=out, where=obs > 0)
        return out


def _to_host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


def _front(ctx, X_or_packed, labels, M, A, packed, C, even=False):
    """the host front of the ops below (ancestry_ops.host_front: the rows re-coded and made contiguous, W taken from the labels)"""
    from .ancestry_ops import host_front
    return host_front(ctx, X_or_packed, labels, M, A, packed, C, even=even)


def allele_counts(ctx, X_or_packed, labels, M, A, packed=False, C=None, debug_rows_per_chunk=0, debug_flush_every=0):
    """ancestry-specific allele counts on the device (gnx_ancestry_allele_counts): X (N, C) int8 in the model's coding (0 REF, 1 ALT,
    anything else missing), or with packed=True the 2-bit rows of DeviceModel.pack_x and C; labels (N, W) in [0, A); the window of SNP c
    is min(c // M, W - 1) -> AlleleCounts of (A, C) int32 arrays"""
    from . import ancestry_ops
    return ancestry_ops.allele_counts(_front(ctx, X_or_packed, labels, M, A, packed, C), debug_rows_per_chunk, debug_flush_every)


def ancestry_dosage(ctx, X, labels, M, A, ancestry, packed=False, C=None):
    """per-individual dosage of one ancestry on the device (gnx_ancestry_dosage): for individual i = rows 2 i, 2 i + 1 and SNP c,
    hapcount = how many of the two haplotypes carry label `ancestry` at c's window, dosage = how many of those are ALT (a missing call
    counts in hapcount only) -> (dosage, hapcount), (N / 2, C) uint8 arrays"""
    from . import ancestry_ops
    return ancestry_ops.dosage(_front(ctx, X, labels, M, A, packed, C), ancestry)


class AncestryScores(collections.namedtuple("AncestryScores", "score n_effect n_scored n_miss")):
    """what ancestry_scores returns (numpy arrays or CUDA tensors as the rows were).  Individual i is haplotype rows 2 i, 2 i + 1.
    score (N / 2, A, S) float64: per ancestry a and score s, the sum of weights[c, a, s] over the scored SNPs c and the individual's
    haplotypes labelled a at c's window that carry the effect allele; n_effect, n_scored, n_miss (N / 2, A) int32: the number of such
    (haplotype, SNP) pairs, of the pairs with a called genotype (0 or 1) and of those with a missing call"""
    __slots__ = ()

    def avg(self):
        """score / n_scored as a float64 (N / 2, A, S) numpy array, NaN where nothing was scored"""
        score = np.asarray(_to_host(self.score), dtype=np.float64)
        den = np.asarray(_to_host(self.n_scored), dtype=np.float64)[:, :, None]
        out = np.full(score.shape, np.nan, dtype=np.float64)
        np.divide(score, den, out=out, where=np.broadcast_to(den > 0, score.shape))
        return out


def score_tables(weights, effect, C, A):
    """the weights and effect alleles of ancestry_scores as the device takes them -> (weights (C, A, S) float64 C-contiguous, effect (C,)
    uint8).  weights: (C,) (one score, the same weight for every ancestry), (C, A) (one score) or (C, A, S); effect: None (ALT
    everywhere) or (C,) of 1 (ALT), 0 (REF), 255 (not scored)"""
    w = np.asarray(weights, dtype=np.float64)
    C, A = int(C), int(A)
    if w.ndim == 1 and w.shape == (C,):
        w = np.repeat(w[:, None], A, axis=1)[:, :, None]
    elif w.ndim == 2 and w.shape == (C, A):
        w = w[:, :, None]
    elif not (w.ndim == 3 and w.shape[:2] == (C, A) and w.shape[2] >= 1):
        raise ValueError(f"weights must be (C={C},), (C, A={A}) or (C, A, S >= 1), got {w.shape}")
    if effect is None:
        eff = np.ones(C, np.uint8)
    else:
        e = np.asarray(effect)
        if e.shape != (C,) or not np.all((e == 0) | (e == 1) | (e == 255)):
            raise ValueError(f"effect must be (C={C},) of 1 (ALT), 0 (REF) or 255 (not scored)")
        eff = e.astype(np.uint8)
    return np.ascontiguousarray(w), eff


def score_chunks(S):
    """the column ranges [s0, s1) in which a table of S scores is served: at most GNX_SCORE_MAX_S per call of the library"""
    step = _lib.GNX_SCORE_MAX_S
    return [(s0, min(s0 + step, S)) for s0 in range(0, S, step)]


def ancestry_scores(ctx, X_or_packed, labels, M, A, weights, effect=None, packed=False, C=None, debug_windows_per_block=0,
                    debug_rows_per_pass=0):
    """ancestry-partitioned polygenic scores on the device (gnx_ancestry_score; include/gnomix_hip.h states the contract and the
    summation order): X (N, C) int8 in the model's coding, or with packed=True the 2-bit rows of DeviceModel.pack_x and C; labels (N, W)
    in [0, A); weights and effect as score_tables takes them -> AncestryScores of numpy arrays.  More than GNX_SCORE_MAX_S scores are
    served in chunks; every score's bits are those of a call with that score alone."""
    from . import ancestry_ops
    f = _front(ctx, X_or_packed, labels, M, A, packed, C, even=True)
    return ancestry_ops.scores(f, *score_tables(weights, effect, f.C, A), debug_windows_per_block, debug_rows_per_pass)


def write_sscore(prefix, scores, names, populations, samples):
    """<prefix>.sscore.tsv from an AncestryScores: one header line, then one line per individual: sample, then per population
    <pop>.n_scored, <pop>.n_effect, <pop>.n_miss, then per score <name>.<pop> for every population and <name>.total (their sum in
    population order), tab-separated.  Floats are written with repr, the shortest text that reads back to the same float64."""
    score = np.asarray(_to_host(scores.score), dtype=np.float64)
    ne, ns, nm = (np.asarray(_to_host(v)) for v in (scores.n_effect, scores.n_scored, scores.n_miss))
    n_ind, A, S = len(samples), len(populations), len(names)
    if score.shape != (n_ind, A, S) or ne.shape != (n_ind, A):
        raise ValueError(f"scores must be ({n_ind} individuals, {A} populations, {S} scores), got {score.shape}")
    num = lambda v: repr(float(v))
    with open(prefix + ".sscore.tsv", "w") as f:
        f.write("sample\t" + "\t".join("%s.n_scored\t%s.n_effect\t%s.n_miss" % (p, p, p) for p in populations) + "\t" +
                "\t".join("\t".join(["%s.%s" % (n, p) for p in populations] + ["%s.total" % n]) for n in names) + "\n")
        for i in range(n_ind):
            cells = [str(samples[i])]
            for a in range(A):
                cells += [str(int(ns[i, a])), str(int(ne[i, a])), str(int(nm[i, a]))]
            for s in range(S):
                total = 0.0
                for a in range(A):
                    total += float(score[i, a, s])
                    cells.append(num(score[i, a, s]))
                cells.append(num(total))
            f.write("\t".join(cells) + "\n")


def pair_counts(ctx, X_or_packed, labels, M, A, ancestry, snp_range=None, packed=False, C=None, debug_snps_per_block=0, check=True):
    """ancestry-specific pairwise counts on the device (gnx_ancestry_pair_counts; include/gnomix_hip.h states the tables): X (N, C) int8
    in the model's coding, or with packed=True the 2-bit rows of DeviceModel.pack_x and C; labels (N, W); snp_range (c0, c1), None = every
    SNP -> asmds.PairCounts of (N / 2, N / 2) int32 arrays.  check=False: labels outside [0, A) do not raise (they count for no ancestry)"""
    from . import ancestry_ops
    return ancestry_ops.pair_counts(_front(ctx, X_or_packed, labels, M, A, packed, C, even=True), ancestry, snp_range, debug_snps_per_block, check)


def ld_counts(ctx, X_or_packed, labels, M, A, ancestry, c0=0, c1=None, band=256, packed=False, C=None, debug_haps_per_block=0, check=True):
    """ancestry-specific LD counts on the device (gnx_ancestry_ld_counts; include/gnomix_hip.h states the tables): X (N, C) int8 in the
    model's coding, or with packed=True the 2-bit rows of DeviceModel.pack_x and C; labels (N, W); the SNPs [c0, c1) (c1 None: to the
    last) and the offsets 0 .. band - 1 -> ld.LDCounts of (c1 - c0, band) int32 arrays.  check=False: labels outside [0, A) do not raise
    (they count for no ancestry)"""
    from . import ancestry_ops
    return ancestry_ops.ld_counts(_front(ctx, X_or_packed, labels, M, A, packed, C), ancestry, c0, c1, band, debug_haps_per_block, check)


def write_clumps(prefix, chm, snp_pos, index_of, p, populations):
    """<prefix>.clumped.tsv from the clumps of every ancestry: index_of (C, A) int64 as ld.clump returns it per column, p (C, A) the
    p-values it was made from.  One header line `chm  pos  population  p  n_members  members`, then one line per index SNP, population
    by population in population order and within one in SNP order: members = the positions of the SNPs clumped with it (itself not
    among them), ascending and comma-separated, `.` when there are none.  p is written with repr, the shortest text that reads back to
    the same float64."""
    pos = np.asarray(snp_pos)
    idx = np.asarray(index_of)
    pv = np.asarray(p, dtype=np.float64)
    if idx.shape != (len(pos), len(populations)) or pv.shape != idx.shape:
        raise ValueError(f"index_of and p must be ({len(pos)} SNPs, {len(populations)} populations), got {idx.shape} and {pv.shape}")
    with open(prefix + ".clumped.tsv", "w") as f:
        f.write("chm\tpos\tpopulation\tp\tn_members\tmembers\n")
        for a, pop in enumerate(populations):
            col = idx[:, a]
            order = np.argsort(col, kind="stable")
            col_s = col[order]
            for c in np.nonzero(col == np.arange(len(pos)))[0]:
                mem = order[np.searchsorted(col_s, c, side="left"):np.searchsorted(col_s, c, side="right")]
                mem = mem[mem != c]
                f.write("%s\t%d\t%s\t%s\t%d\t%s\n" % (chm, int(pos[c]), pop, repr(float(pv[c, a])), mem.size,
                                                      ",".join(str(int(pos[m])) for m in mem) if mem.size else "."))


def write_asmds(prefix, results, population_order, samples):
    """<prefix>.asmds.tsv from the ancestry-specific MDS of every ancestry: results[a] is an asmds.AncestryMDS over the len(samples)
    individuals (kept = the indices embedded, n_sites = their OO[i, i]) or None (fewer than k + 1 individuals kept: the ancestry gets
    its header line and no rows).  One block per ancestry in population order: a header line `sample  population  n_sites  kept  PC1..PCk`,
    then one line per individual; a dropped individual has kept = 0, n_sites NA and NA coordinates.  Floats are written with repr, the
    shortest text that reads back to the same float64."""
    if len(results) != len(population_order):
        raise ValueError(f"one result per population: {len(results)} results, {len(population_order)} populations")
    ks = {np.asarray(r.coords).shape[1] for r in results if r is not None}
    if len(ks) > 1:
        raise ValueError(f"the embeddings have different numbers of components: {sorted(ks)}")
    k = ks.pop() if ks else 0
    head = "sample\tpopulation\tn_sites\tkept" + "".join("\tPC%d" % (q + 1) for q in range(k)) + "\n"
    with open(prefix + ".asmds.tsv", "w") as f:
        for pop, r in zip(population_order, results):
            f.write(head)
            if r is None:
                continue
            coords = np.asarray(r.coords, dtype=np.float64)
            kept = np.arange(len(samples)) if r.kept is None else np.asarray(r.kept)
            if coords.shape[0] != kept.shape[0] or (kept.size and kept.max() >= len(samples)):
                raise ValueError(f"{pop}: {coords.shape[0]} embedded rows, {kept.shape[0]} kept indices, {len(samples)} samples")
            row_of = {int(i): q for q, i in enumerate(kept)}
            for i, smp in enumerate(samples):
                q = row_of.get(i)
                if q is None:
                    f.write("%s\t%s\tNA\t0%s\n" % (smp, pop, "\tNA" * k))
                else:
                    sites = "NA" if r.n_sites is None else str(int(r.n_sites[q]))
                    f.write("%s\t%s\t%s\t1\t%s\n" % (smp, pop, sites, "\t".join(repr(float(v)) for v in coords[q])))


def write_afreq(prefix, chm, snp_pos, M, W, counts, populations):
    """<prefix>.afreq.tsv: one header line, then one line per model SNP in model order: chm, pos, window (min(c // M, W - 1)), then per
    population <pop>.n_obs, <pop>.n_alt, <pop>.freq (n_alt / n_obs with six decimals, nan when n_obs == 0), tab-separated"""
    obs, alt = np.asarray(_to_host(counts.n_obs)), np.asarray(_to_host(counts.n_alt))
    pos = np.asarray(snp_pos)
    if obs.ndim != 2 or obs.shape != alt.shape or obs.shape != (len(populations), len(pos)):
        raise ValueError(f"counts must be ({len(populations)} populations, {len(pos)} SNPs), got {obs.shape}")
    freq = counts.freq()
    with open(prefix + ".afreq.tsv", "w") as f:
        f.write("chm\tpos\twindow\t" + "\t".join("%s.n_obs\t%s.n_alt\t%s.freq" % (p, p, p) for p in populations) + "\n")
        for c in range(len(pos)):
            cells = [str(chm), str(int(pos[c])), str(min(c // int(M), int(W) - 1))]
            for a in range(len(populations)):
                cells += [str(int(obs[a, c])), str(int(alt[a, c])), format(float(freq[a, c]), ".6f") if obs[a, c] > 0 else "nan"]
            f.write("\t".join(cells) + "\n")


def write_assoc(prefix, chm, snp_pos, M, W, result, populations, c0=None, name=None):
    """<prefix>.assoc.tsv from an assoc.AncestryAssoc: one header line, then one line per model SNP in model order: chm, pos, window,
    n, df, status, n_miss, then per population <pop>.n_hap, .n_alt, .beta, .se, .t, .p (floats with six significant digits, nan for a
    dropped term or a SNP that was not fitted), tab-separated.  name: the file is <prefix>.assoc.<name>.tsv (one trait of several).
    c0 (None: `result` holds all C SNPs): `result` holds the SNPs c0 .. c0 + len(result.beta) - 1 only, a result that arrives chunk of
    SNPs by chunk: the chunk at c0 = 0 starts the file, a later one goes behind the lines the file has."""
    pos = np.asarray(snp_pos)
    A, C = len(populations), len(pos)
    nc = C if c0 is None else len(result.beta)
    append = c0 is not None and int(c0) > 0
    c0 = 0 if c0 is None else int(c0)
    if np.asarray(result.beta).shape != (nc, A) or c0 < 0 or c0 + nc > C:
        raise ValueError(f"result must be ({nc} SNPs, {A} populations), got {np.asarray(result.beta).shape}")
    num = lambda v: format(float(v), ".6g") if np.isfinite(v) else "nan"
    with open(prefix + (".assoc.tsv" if name is None else ".assoc.%s.tsv" % name), "a" if append else "w") as f:
        if not append:
            f.write("chm\tpos\twindow\tn\tdf\tstatus\tn_miss\t" +
                    "\t".join("\t".join(p + s for s in (".n_hap", ".n_alt", ".beta", ".se", ".t", ".p")) for p in populations) + "\n")
        for i in range(nc):
            c = c0 + i
            cells = [str(chm), str(int(pos[c])), str(min(c // int(M), int(W) - 1)), str(int(result.n[i])), str(int(result.df[i])),
                     str(int(result.status[i])), str(int(result.n_miss[i]))]
            for a in range(A):
                cells += [str(int(result.n_hap[i, a])), str(int(result.n_alt[i, a])), num(result.beta[i, a]), num(result.se[i, a]),
                          num(result.t[i, a]), num(result.p[i, a])]
            f.write("\t".join(cells) + "\n")


def write_assoc_logit(prefix, chm, snp_pos, M, W, result, populations):
    """<prefix>.assoc.logistic.tsv from an assoc.AncestryAssocLogit: one header line, then one line per model SNP in model order: chm,
    pos, window, n, n_case, df, status, iters, n_miss, lrt, lrt_df, lrt_p, then per population <pop>.n_hap, .n_alt, .n_alt_case, .beta,
    .se, .z, .p (floats with six significant digits, nan for a dropped term or a SNP that was not fitted), tab-separated"""
    pos = np.asarray(snp_pos)
    A, C = len(populations), len(pos)
    if np.asarray(result.beta).shape != (C, A):
        raise ValueError(f"result must be ({C} SNPs, {A} populations), got {np.asarray(result.beta).shape}")
    num = lambda v: format(float(v), ".6g") if np.isfinite(v) else "nan"
    with open(prefix + ".assoc.logistic.tsv", "w") as f:
        f.write("chm\tpos\twindow\tn\tn_case\tdf\tstatus\titers\tn_miss\tlrt\tlrt_df\tlrt_p\t" +
                "\t".join("\t".join(p + s for s in (".n_hap", ".n_alt", ".n_alt_case", ".beta", ".se", ".z", ".p")) for p in populations) + "\n")
        for c in range(C):
            cells = [str(chm), str(int(pos[c])), str(min(c // int(M), int(W) - 1)), str(int(result.n[c])), str(int(result.n_case[c])),
                     str(int(result.df[c])), str(int(result.status[c])), str(int(result.iters[c])), str(int(result.n_miss[c])), num(result.lrt[c]),
                     str(int(result.lrt_df[c])), num(result.lrt_p[c])]
            for a in range(A):
                cells += [str(int(result.n_hap[c, a])), str(int(result.n_alt[c, a])), str(int(result.n_alt_case[c, a])), num(result.beta[c, a]),
                          num(result.se[c, a]), num(result.z[c, a]), num(result.p[c, a])]
            f.write("\t".join(cells) + "\n")


def write_lai(prefix, meta, labels, positions, samples, populations=None, n_threads=0, first_line=None):
    """<prefix>.lai — the bytes msp_to_lai writes from <prefix>.msp, from the labels themselves (gnx_write_lai): the .msp's first
    header line (built from `populations`, or given as `first_line`), "position" and the haplotype columns, then one line per query
    SNP: its position and the N labels of its window (meta["n snps"] positions per window)."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    n_snps = np.ascontiguousarray(meta["n snps"], dtype=np.int64)
    if lab.ndim != 2 or lab.shape[1] != len(n_snps):
        raise ValueError(f"labels must be (N, W={len(n_snps)}), got {lab.shape}")
    pos = np.ascontiguousarray(positions, dtype=np.int64)
    if first_line is None:
        first_line = "#Subpopulation order/codes: " + "\t".join([str(pop) + "=" + str(i) for i, pop in enumerate(populations)]) + "\n"
    head = first_line + "position\t" + "\t".join([str(s) for q in samples for s in (str(q) + ".0", str(q) + ".1")]) + "\n"
    head = head.encode()
    _lib.io_check(_lib.load().gnx_write_lai((prefix + ".lai").encode(), head, len(head), pos.ctypes.data, len(pos), n_snps.ctypes.data,
                                            lab.ctypes.data, lab.shape[0], lab.shape[1], lab.shape[1], int(n_threads)))


def write_bed_runs(root, meta, offsets, triples, samples, pop_order=None, n_threads=0):
    """one .bed per haplotype column from a run list (label_runs): the files msp_to_bed writes (gnx_write_bed)"""
    os.makedirs(root, exist_ok=True)
    cols = [s for r in _meta_strings(meta) for s in r[:5]]
    cb, co = _blob(cols)
    names = [(str(q) + h).replace(".", "_") + ".bed" for q in samples for h in (".0", ".1")]
    fb, fo = _blob(names)
    ab, ao = _blob([str(p) for p in pop_order] if pop_order is not None else [])
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    triples = np.ascontiguousarray(triples, dtype=np.int32)
    if len(offsets) != len(names) + 1:
        raise ValueError(f"{len(names)} haplotype columns but {len(offsets) - 1} rows of runs")
    head = b"chm\tspos\tepos\tancestry\tsgpos\tegpos\n"
    _lib.io_check(_lib.load().gnx_write_bed(root.encode(), fb, fo.ctypes.data, head, len(head), cb, co.ctypes.data, ab, ao.ctypes.data,
                                            0 if pop_order is None else len(pop_order), offsets.ctypes.data, triples.ctypes.data,
                                            len(names), len(meta["spos"]), int(n_threads)))


def write_bed(root, meta, labels, samples, pop_order=None, ctx=None, n_threads=0):
    """<root>/<sample>_<0|1>.bed for every haplotype row of labels (N, W): the runs come from the device (k_label_runs), the text
    and the files from the library's host threads"""
    if ctx is None:
        ctx = _lib.default_context(0)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 2 or lab.shape[1] != len(meta["spos"]):
        raise ValueError(f"labels must be (N, W={len(meta['spos'])}), got {lab.shape}")
    _, offsets, triples = label_runs(ctx, lab)
    write_bed_runs(root, meta, offsets, triples, samples, pop_order, n_threads)


def msp_to_lai(msp_file, positions, lai_file=None):
    """SNP-level labels (postprocess.py:128-160): every window row repeated `n snps` times."""
    with open(msp_file) as f:
        first, second = f.readline(), f.readline()
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    samples = second[:-1].split("\t")[6:]
    n_reps = np.array([int(r[5]) for r in rows])
    assert n_reps.sum() == len(positions)
    data = np.array([[int(v) for v in r[6:]] for r in rows])
    snp = np.repeat(data, n_reps, axis=0)
    if lai_file is not None:
        with open(lai_file, "w") as f:
            f.write(first)
            f.write("position\t" + "\t".join(samples) + "\n")
            for p, r in zip(positions, snp):
                f.write(str(p) + "\t" + "\t".join(str(v) for v in r) + "\n")
    return samples, snp


def msp_to_bed(msp_file, root, pop_order=None):
    """one run-length encoded .bed per haplotype column (postprocess.py:162-210)"""
    with open(msp_file) as f:
        f.readline()
        header = f.readline().rstrip("\n").split("\t")
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    os.makedirs(root, exist_ok=True)
    lab = (lambda a: a) if pop_order is None else (lambda a: pop_order[int(a)])
    for ci, sample in enumerate(header[6:]):
        out = []
        start = 0
        for i in range(1, len(rows) + 1):
            if i == len(rows) or rows[i][6 + ci] != rows[start][6 + ci]:
                out.append((rows[start][0], rows[start][1], rows[i - 1][2], lab(rows[start][6 + ci]), rows[start][3], rows[i - 1][4]))
                start = i
        with open(os.path.join(root, sample.replace(".", "_") + ".bed"), "w") as f:
            f.write("chm\tspos\tepos\tancestry\tsgpos\tegpos\n")
            for r in out:
                f.write("\t".join(str(v) for v in r) + "\n")
