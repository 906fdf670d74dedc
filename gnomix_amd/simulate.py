"""Training data for a new model: the reference's admixture simulator (src/laidataset.py, driven by gnomix.py:245-306) and its
per-window labels (src/preprocess.py:37-82), with the random draws on the host and the matrix written by the GPU.

The host restates the reference's draws call for call on numpy's legacy global generator, so the same seed gives the same
splits and the same simulated individuals; what the draws produce is a short segment table per haplotype.  gnx_simulate_admix
(csrc/sim/k_sim_admix.hip) expands the tables into X (mat_vcf_2d), the per-SNP ancestry (mat_map) and the window labels in one
pass.  `expand_numpy` is the same expansion on the CPU (the check of the kernel, and what the host tests run).

    plan = simulate.plan_splits(panel, gmap, smap, config)   # host-side draws
    data = plan.materialise(ctx)                             # ((X_t1, y_t1), (X_t2, y_t2), (X_v, y_v)) for HipGnomix.train

Deviations from the reference, on purpose:
  * a founder genotype other than 0 / 1 (missing, allele >= 2) is an error that names the sample and the variant; the reference
    casts allel's -1 to uint8 255 and keeps alleles >= 2 as they are.
  * include_all (laidataset.py:312-331) calls DataFrame.append, which pandas >= 2 removed (and DataFrame.sample refuses its float
    count): here it draws what it intends, np.random.choice(len(founders of the population), n_copies, replace=False) on the global
    generator, and appends those founders to train2.  That branch is NOT pinned to the reference (no environment here runs it).
  * sample weights are uniform (the weights file cannot be given on the command line).
"""
from __future__ import annotations

import os
import pickle
from dataclasses import dataclass, field

import numpy as np

from . import _lib

SPLITS = ("train1", "train2", "val")
MIN_SPLIT = {"train1": 800, "train2": 150, "val": 50}   # gnomix.py:288
NOT_A_FOUNDER = 255                                      # anc_of_src code of a panel haplotype no segment may use

# the reference's config.yaml, as plain values
DEFAULT_CONFIG = {
    "verbose": True,
    "seed": 94305,
    "simulation": {"run": True, "path": None, "splits": {"ratios": {"train1": 0.8, "train2": 0.15, "val": 0.05}},
                   "gens": [0, 2, 4, 6, 8, 12, 16, 24], "r_admixed": 1, "rm_data": False},
    "model": {"name": "model", "inference": None, "window_size_cM": 0.2, "smooth_size": 75, "context_ratio": 0.5,
              "retrain_base": True, "calibrate": False, "n_cores": None},
    "inference": {"bed_file_output": False, "snp_level_inference": False, "visualize_inference": False},
}


def merge_config(user):
    """the reference's defaults under the user's values (dicts merged key by key, everything else replaced)"""
    def merge(d, u):
        out = {k: (merge(v, {}) if isinstance(v, dict) else (list(v) if isinstance(v, list) else v)) for k, v in d.items()}
        for k, v in (u or {}).items():
            out[k] = merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
        return out
    return merge(DEFAULT_CONFIG, user)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def read_genetic_map(path, chm=None, header=None):
    """read_genetic_map (src/utils.py:161-182): tab-separated chm / pos / pos_cm, '#' comments, no header; when the values do not
    parse, once more with the first row as a header; the rows of `chm`, or of "chr" + chm when there are none"""
    import pandas as pd
    df = pd.read_csv(path, delimiter="\t", header=header, comment="#", dtype=str)
    if df.shape[1] != 3:
        raise ValueError("genetic map %s: expected 3 tab-separated columns (chm, pos, pos_cm), found %d" % (path, df.shape[1]))
    df.columns = ["chm", "pos", "pos_cm"]
    try:
        df = df.astype({"chm": str, "pos": int, "pos_cm": float})
    except ValueError:
        if header is None:
            print("WARNING: Something wrong with genetic map format. Trying with header...")
            return read_genetic_map(path, chm=chm, header=0)
        raise ValueError("Genetic map format not understood.")
    if chm is not None:
        chm = str(chm)
        df = df[df.chm == chm] if (df.chm == chm).any() else df[df.chm == "chr" + chm]
    return df


def chm_info(gmap, snp_pos):
    """get_chm_info (laidataset.py:9-42): chromosome length in Morgans and the probability of a breakpoint before each SNP 1..C-1
    (scipy's interpolation itself: the probabilities feed RandomState.choice, so they must be the reference's bit for bit)"""
    import scipy.interpolate
    morgans = max(gmap["pos_cm"]) / 100.0
    cm = scipy.interpolate.interp1d(x=gmap["pos"].to_numpy(), y=gmap["pos_cm"].to_numpy(), fill_value="extrapolate")(snp_pos)
    lengths = cm[1:] - cm[0:-1]
    return morgans, lengths / lengths.sum()


def read_sample_map(path):
    """get_sample_map_data (laidataset.py:44-68) without a weights file -> (samples, populations, pop_to_num); codes follow the order of
    first appearance"""
    import pandas as pd
    df = pd.read_csv(path, delimiter="\t", header=None, comment="#", dtype="object")
    if df.shape[1] != 2:
        raise ValueError("sample map %s: expected 2 tab-separated columns (sample, population), found %d" % (path, df.shape[1]))
    samples, pops = [str(s) for s in df[0]], [str(p) for p in df[1]]
    pop_to_num = {}
    for p in pops:
        pop_to_num.setdefault(p, len(pop_to_num))
    return samples, pops, pop_to_num


# ---- splits and segment tables --------------------------------------------------------------------------------------
def split_founders(pops, ratios):
    """create_splits (laidataset.py:333-353) with split_sample_map (:277-310) and include_all (:312-331), on the global generator.
    -> {split: sample-map rows of its founders, in the order the reference's table holds them}"""
    names, prop = zip(*ratios.items())
    prop = np.array(prop) / np.sum(prop)
    pops = np.array(pops, dtype=object)
    split_of = {}
    for p in np.unique(pops):
        ids = list(np.flatnonzero(pops == p))
        n_pop = len(ids)
        n_sets = [int(round(r * n_pop)) for r in prop]
        while sum(n_sets) > n_pop:
            n_sets[0] -= 1
        while sum(n_sets) < n_pop:
            n_sets[-1] += 1
        for s, name in enumerate(names):
            pick = np.random.choice(len(ids), n_sets[s], replace=False)
            for i in sorted(pick, reverse=True):
                split_of[ids.pop(i)] = name
    rows = {name: [r for r in range(len(pops)) if split_of.get(r) == name] for name in names}
    # include_all(from_split="train1", in_split="train2")
    frm, into = rows.get("train1", []), rows.get("train2", [])
    from_pop = np.unique(pops[frm]) if frm else np.array([], dtype=object)
    if len(from_pop) and "train2" in rows:
        ave = np.round(len(frm) / len(from_pop))
        missing = [p for p in from_pop if p not in set(pops[into])]
        if missing:
            print("WARNING: Small sample size from populations: {}".format(np.array(missing)))
            print("... Proceeding by including duplicates in both base- and smoother data...")
        for p in missing:
            cand = [r for r in frm if pops[r] == p]
            n = int(min(ave, len(cand)))
            rows["train2"] += [cand[i] for i in np.random.choice(len(cand), n, replace=False)]
    return rows


def _admix(n_founders, weights, hap_of, gen, bp, C, morgans):
    """admix (laidataset.py:119-176): the same draws in the same order -> (begins, sources)"""
    k = int(sum(np.random.poisson(morgans, size=gen)))
    if k == 0:
        f = np.random.choice(n_founders, p=weights)
        return [0], [hap_of[f] + (0 if np.random.rand() >= 0.5 else 1)]
    cuts = np.sort(np.random.choice(np.arange(1, C), size=k, replace=False, p=bp))
    srcs = []
    for _ in range(k + 1):
        f = np.random.choice(n_founders, p=weights)
        srcs.append(hap_of[f] + (0 if np.random.rand() >= 0.5 else 1))
    return [0] + [int(c) for c in cuts], srcs


@dataclass
class SimPlan:
    """Everything drawn on the host.  Haplotypes are numbered in the order of the reference's files: split, then generation, then
    individual (maternal 2i, paternal 2i + 1).  Segment sources are panel haplotypes (2 * VCF sample + {0 maternal, 1 paternal})."""
    C: int
    morgans: float
    bp: np.ndarray
    chm: str
    pop_order: list                 # population of code a
    samples: list                   # sample map rows
    pops: list
    vcf_index: np.ndarray           # sample-map row -> VCF sample
    split_rows: dict                # split -> founder rows (sample map)
    gens: dict                      # split -> generations, in simulation order
    num_outs: dict                  # split -> individuals per generation (gen 0: the split's founders)
    seg_off: np.ndarray             # (N + 1,) int64
    seg_begin: np.ndarray           # int32
    seg_src: np.ndarray             # int32
    parts: list                     # [(split, gen, first haplotype, haplotype count)]
    anc_of_src: np.ndarray          # (2 * VCF samples,) uint8, NOT_A_FOUNDER outside the sample map
    panel: object = None            # the parsed reference VCF (vcfio.VcfData)
    meta: dict = field(default_factory=dict)

    @property
    def N(self):
        return len(self.seg_off) - 1

    @property
    def A(self):
        return len(self.pop_order)

    def window_size(self, window_size_cM):
        """get_data (gnomix.py:121-125): window size in SNPs"""
        M = int(round(window_size_cM * (self.C / (100 * self.morgans))))
        return M + 1 if self.C % M == 0 else M

    def split_slices(self):
        """split -> (first haplotype, last + 1) over all its generations"""
        out = {}
        for split, _, h0, n in self.parts:
            lo, hi = out.get(split, (h0, h0))
            out[split] = (min(lo, h0), max(hi, h0 + n))
        return out

    def founders_host(self):
        """(2 * VCF samples, C) int8: the panel's haplotypes, row 2s + {0, 1} = the two alleles of VCF sample s"""
        gt = np.asarray(self.panel["calldata/GT"])
        return np.ascontiguousarray(gt.reshape(gt.shape[0], -1).T)

    def _check(self, ctx, rc):
        if rc != _lib.GNX_OK:
            msg = ctx.lib.gnx_last_error(ctx.h).decode()
            raise _lib.GnxError(rc, self._name_founder(msg))

    def _name_founder(self, msg):
        import re
        m = re.search(r"founder haplotype (\d+) \(sample \d+\) holds (-?\d+) at SNP (\d+)", msg)
        if not m:
            return msg
        h, v, c = int(m.group(1)), int(m.group(2)), int(m.group(3))
        name = str(self.panel["samples"][h // 2])
        pos = int(np.asarray(self.panel["variants/POS"])[c])
        return "%s (sample %s, %s allele, variant %d at position %d: value %s)" % (msg, name, "first" if h % 2 == 0 else "second", c, pos,
                                                                                  "missing or allele >= 2" if v == 2 else v)

    def simulate_host(self, ctx, M, want_anc=True):
        """gnx_simulate_admix on host arrays -> X (N, C) int8, Y (N, W) int32, anc (N, C) uint8 or None"""
        F = self.founders_host()
        N, W = self.N, self.C // M
        X = np.empty((N, self.C), np.int8)
        Y = np.empty((N, W), np.int32)
        anc = np.empty((N, self.C), np.uint8) if want_anc else None
        self._check(ctx, ctx.lib.gnx_simulate_admix(ctx.h, F.ctypes.data, F.shape[0], F.shape[1], self.C, int(M), self.seg_off.ctypes.data,
                                                    self.seg_begin.ctypes.data, self.seg_src.ctypes.data, self.anc_of_src.ctypes.data,
                                                    self.A, N, X.ctypes.data, self.C, Y.ctypes.data, anc.ctypes.data if want_anc else None))
        return X, Y, anc

    def founders_device(self, ctx, device):
        """the panel's haplotypes built in HBM from its 2-bit rows (gnx_gt2_to_x_dev, identity column map): (2 * VCF samples, ld) int8
        tensor, ld a multiple of 16"""
        import torch
        G = torch.from_numpy(np.require(self.panel.gt2, requirements=["C", "W"])).to(device)
        n_haps = 2 * len(self.panel["samples"])
        ld = (self.C + 15) // 16 * 16
        src = torch.arange(self.C, dtype=torch.int32, device=device)
        F = torch.empty((n_haps, ld), dtype=torch.int8, device=device)
        ctx.set_stream(torch.cuda.current_stream(device).cuda_stream)
        ctx.check(ctx.lib.gnx_gt2_to_x_dev(ctx.h, G.data_ptr(), self.C, G.stride(0), 0, n_haps, src.data_ptr(), self.C, F.data_ptr(), ld))
        return F

    def simulate_device(self, ctx, M, want_anc=True, F=None):
        """gnx_simulate_admix_dev on torch tensors (asynchronous on torch's current stream, apart from the validation read-back)
        -> X (N, ld) int8, Y (N, W) int32, anc (N, C) uint8 or None, all CUDA tensors; X[:, :C] is the matrix"""
        import torch
        device = torch.device("cuda", ctx.device)
        if F is None:
            F = self.founders_device(ctx, device)
        t = {k: torch.from_numpy(getattr(self, k)).to(device) for k in ("seg_off", "seg_begin", "seg_src", "anc_of_src")}
        N, W, ld = self.N, self.C // M, F.shape[1]
        X = torch.empty((N, ld), dtype=torch.int8, device=device)
        Y = torch.empty((N, W), dtype=torch.int32, device=device)
        anc = torch.empty((N, self.C), dtype=torch.uint8, device=device) if want_anc else None
        ctx.set_stream(torch.cuda.current_stream(device).cuda_stream)
        self._check(ctx, ctx.lib.gnx_simulate_admix_dev(ctx.h, F.data_ptr(), F.shape[0], F.stride(0), self.C, int(M), t["seg_off"].data_ptr(),
                                                        t["seg_begin"].data_ptr(), t["seg_src"].data_ptr(), t["anc_of_src"].data_ptr(), self.A,
                                                        N, X.data_ptr(), X.stride(0), Y.data_ptr(), anc.data_ptr() if want_anc else None))
        return X, Y, anc

    def as_splits(self, X, Y):
        """the rows of each split -> ((X_t1, y_t1), (X_t2, y_t2), (X_v, y_v)), (None, None) for a split that was not simulated"""
        sl = self.split_slices()
        return tuple((X[sl[s][0]:sl[s][1]], Y[sl[s][0]:sl[s][1]]) if s in sl else (None, None) for s in SPLITS)

    def materialise(self, ctx, window_size_cM=None, M=None, want_anc=False):
        """the simulated splits as HipGnomix.train takes them (host arrays; the host entry point stages through the device).
        want_anc: also return the per-SNP ancestry (N, C) -> (data, anc)"""
        M = M if M is not None else self.window_size(window_size_cM if window_size_cM is not None else DEFAULT_CONFIG["model"]["window_size_cM"])
        X, Y, anc = self.simulate_host(ctx, M, want_anc=want_anc)
        data = self.as_splits(X, Y)
        return (data, anc) if want_anc else data

    def materialise_dev(self, ctx, window_size_cM=None, M=None, want_anc=False):
        """the same with the founders built in HBM and every array a CUDA tensor (X as (N, C) views of 16-byte aligned rows)"""
        M = M if M is not None else self.window_size(window_size_cM if window_size_cM is not None else DEFAULT_CONFIG["model"]["window_size_cM"])
        X, Y, anc = self.simulate_device(ctx, M, want_anc=want_anc)
        data = self.as_splits(X[:, :self.C], Y)
        return (data, anc) if want_anc else data


def plan_splits(panel, gmap, smap, config, chm=None, verbose=False):
    """simulate_splits (gnomix.py:245-306) up to the matrices: reads the inputs, seeds numpy's global generator with config["seed"] as
    LAIDataset.__init__ does, splits the founders and draws every simulated haplotype's segments.  `panel`: a path or a parsed
    vcfio.VcfData; `gmap`: a path or read_genetic_map's frame; `smap`: a path or (samples, populations)."""
    from . import vcfio
    config = merge_config(config)
    sim = config["simulation"]
    if isinstance(panel, (str, os.PathLike)):
        panel = vcfio.read_vcf(str(panel), chm=chm)
        if panel is None:
            raise ValueError("no variants in the reference file")
    pos = np.asarray(panel["variants/POS"])
    C = len(pos)
    if C < 2:
        raise ValueError("the reference panel needs at least two SNPs")
    if isinstance(gmap, (str, os.PathLike)):
        gmap = read_genetic_map(str(gmap), chm)
    if len(gmap) == 0:
        raise ValueError("the genetic map holds no rows of chromosome %s" % chm)
    np.random.seed(config["seed"])
    morgans, bp = chm_info(gmap, pos)
    if isinstance(smap, (str, os.PathLike)):
        samples, pops, pop_to_num = read_sample_map(str(smap))
    else:
        samples, pops = [str(s) for s in smap[0]], [str(p) for p in smap[1]]
        pop_to_num = {}
        for p in pops:
            pop_to_num.setdefault(p, len(pop_to_num))
    vcf_samples = [str(s) for s in panel["samples"]]
    where = {s: i for i, s in enumerate(vcf_samples)}
    absent = [s for s in samples if s not in where]
    if absent:
        raise ValueError("sample %r of the sample map is not in the reference file%s" % (absent[0], " (and %d more)" % (len(absent) - 1) if len(absent) > 1 else ""))
    if len(set(samples)) != len(samples):
        raise ValueError("the sample map names a sample twice")
    vcf_index = np.array([where[s] for s in samples], np.int64)
    if len(pop_to_num) > 255:   # ancestry codes are bytes (GNX_SIM_MAX_A)
        raise ValueError("more than 255 populations")

    ratios = {k: v for k, v in dict(sim["splits"]["ratios"]).items() if not (k == "val" and v == 0)}   # gnomix.py:378-379
    if len(samples) <= 25 and ratios.get("val"):                                                   # gnomix.py:270-273
        print("WARNING: Too few samples to run validation.")
        del ratios["val"]
    gens = split_generations(sim)
    rows = split_founders(pops, ratios)

    # gnomix.py:285-292 and LAIDataset.simulate (laidataset.py:362-428), split by split, generation by generation
    w_all = np.array([1.0 / len(samples)] * len(samples))
    codes = np.array([pop_to_num[p] for p in pops], np.uint8)
    num_outs, off, begins, srcs, parts = {}, [0], [], [], []
    for split in ratios:
        total = max(len(rows[split]) * sim["r_admixed"], MIN_SPLIT[split])
        num_outs[split] = int(total / len(gens[split]))
        founders = rows[split]
        if not founders:
            raise ValueError("Split does not exist!!!")
        hap_of = [2 * int(vcf_index[r]) for r in founders]
        w = w_all[founders]
        w = list(w / w.sum())
        for gen in gens[split]:
            h0 = len(off) - 1
            if gen == 0:
                for h in hap_of:
                    for side in (0, 1):
                        begins.append(0); srcs.append(h + side); off.append(len(begins))
            else:
                for _ in range(num_outs[split]):
                    for _side in (0, 1):
                        b, s = _admix(len(founders), w, hap_of, gen, bp, C, morgans)
                        begins += b; srcs += s; off.append(len(begins))
                    np.random.rand()   # the individual's name (laidataset.py:412)
            parts.append((split, gen, h0, len(off) - 1 - h0))
            if verbose:
                print("simulated %s gen %s: %d haplotypes" % (split, gen, len(off) - 1 - h0))
    anc_of_src = np.full(2 * len(vcf_samples), NOT_A_FOUNDER, np.uint8)
    anc_of_src[2 * vcf_index] = codes
    anc_of_src[2 * vcf_index + 1] = codes
    alt = np.asarray(panel["variants/ALT"])
    meta = {"chm": chm, "morgans": morgans, "num_snps": C, "pos_snps": pos.copy(), "ref_snps": np.asarray(panel["variants/REF"]).astype(str),
            "alt_snps": (alt[:, 0] if alt.ndim == 2 else alt).astype(str), "pop_to_num": dict(pop_to_num),
            "num_to_pop": {v: k for k, v in pop_to_num.items()}}
    return SimPlan(C=C, morgans=morgans, bp=bp, chm=chm, pop_order=list(pop_to_num), samples=samples, pops=pops, vcf_index=vcf_index,
                   split_rows=rows, gens={s: gens[s] for s in ratios}, num_outs=num_outs, seg_off=np.array(off, np.int64),
                   seg_begin=np.array(begins, np.int32), seg_src=np.array(srcs, np.int32), parts=parts, anc_of_src=anc_of_src,
                   panel=panel, meta=meta)


def split_generations(sim):
    """gnomix.py:381-389: the generations of each split (train1 gets 0 added, in Python's set order, as the reference builds it)"""
    g = sim["splits"].get("gens")
    if g:
        return {k: list(v) for k, v in g.items()}
    generations = list(sim["gens"])
    return {"train1": list(set(generations + [0])), "train2": generations, "val": [x for x in generations if x != 0]}


# ---- CPU expansion: the check of the kernel -----------------------------------------------------------------------------
def expand_numpy(F, seg_off, seg_begin, seg_src, anc_of_src, C):
    """the segment tables over founder rows F (n, >= C) -> X (N, C) int8, anc (N, C) uint8; F values other than 0 / 1 in a used row
    raise ValueError"""
    N = len(seg_off) - 1
    X = np.empty((N, C), np.int8)
    anc = np.empty((N, C), np.uint8)
    for n in range(N):
        s0, s1 = int(seg_off[n]), int(seg_off[n + 1])
        for s in range(s0, s1):
            b, e = int(seg_begin[s]), (int(seg_begin[s + 1]) if s + 1 < s1 else C)
            X[n, b:e] = F[seg_src[s], b:e]
            anc[n, b:e] = anc_of_src[seg_src[s]]
    used = np.unique(seg_src)
    bad = (F[used, :C] != 0) & (F[used, :C] != 1)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise ValueError("founder haplotype %d holds %d at SNP %d: founders must be 0 or 1" % (used[r], F[used[r], c], c))
    return X, anc


def window_labels(anc, M):
    """window_reshape (src/preprocess.py:37-59): W = C // M windows, the last one M + C % M SNPs long; label = most frequent code,
    ties to the smallest (scipy.stats.mode) -> (N, W) int16, as data_process returns it"""
    anc = np.asarray(anc)
    N, C = anc.shape
    W = C // M
    A = int(anc.max()) + 1 if anc.size else 1
    y = np.empty((N, W), np.int16)
    for w in range(W):
        seg = anc[:, w * M:(C if w == W - 1 else (w + 1) * M)]
        counts = np.stack([(seg == a).sum(1) for a in range(A)], axis=1)
        y[:, w] = np.argmax(counts, axis=1)
    return y


def simulate_numpy(plan, M):
    """the plan expanded on the CPU -> X (N, C) int8, Y (N, W) int16, anc (N, C) uint8"""
    X, anc = expand_numpy(plan.founders_host(), plan.seg_off, plan.seg_begin, plan.seg_src, plan.anc_of_src, plan.C)
    return X, window_labels(anc, M), anc


# ---- the reference's on-disk layout -------------------------------------------------------------------------------------
def write_generated_data(plan, data_path, X, anc, gen_map=None):
    """what simulate_splits writes under <out>/generated_data: sample_maps/<split>.map, metadata.pkl, gen_map_df.pkl and, per split
    and generation, mat_vcf_2d.npy / mat_map.npy as uint8 (write_output, laidataset.py:180-201)"""
    os.makedirs(os.path.join(data_path, "sample_maps"), exist_ok=True)
    for split in plan.gens:
        with open(os.path.join(data_path, "sample_maps", split + ".map"), "w") as f:
            for r in plan.split_rows[split]:
                f.write("%s\t%s\n" % (plan.samples[r], plan.pops[r]))
    with open(os.path.join(data_path, "metadata.pkl"), "wb") as f:
        pickle.dump(plan.meta, f, protocol=pickle.HIGHEST_PROTOCOL)
    if gen_map is not None:
        with open(os.path.join(data_path, "gen_map_df.pkl"), "wb") as f:
            pickle.dump(gen_map, f, protocol=pickle.HIGHEST_PROTOCOL)
    for split, gen, h0, n in plan.parts:
        d = os.path.join(data_path, split, "gen_" + str(gen))
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "mat_vcf_2d.npy"), np.ascontiguousarray(X[h0:h0 + n, :plan.C]).view(np.uint8))
        np.save(os.path.join(d, "mat_map.npy"), np.ascontiguousarray(anc[h0:h0 + n]))


def read_generated_data(data_path, generations, window_size_cM):
    """get_data (gnomix.py:102-156) on a generated_data directory (this project's or the reference's): metadata.pkl through the
    restricted unpickler (numpy arrays and builtins only), the .npy files, window labels on the host -> (data, meta)"""
    from .refpickle import load_reference_pickle
    md = load_reference_pickle(os.path.join(data_path, "metadata.pkl"), use_sklearn=False)
    pop_order = [str(md["num_to_pop"][i]) for i in range(len(md["num_to_pop"]))]
    C = len(md["pos_snps"])
    M = int(round(window_size_cM * (C / (100 * md["morgans"]))))
    if C % M == 0:
        M += 1
    meta = {"A": len(pop_order), "C": C, "M": M, "snp_pos": np.asarray(md["pos_snps"]), "snp_ref": np.asarray(md["ref_snps"]),
            "snp_alt": np.asarray(md["alt_snps"]), "pop_order": pop_order, "morgans": md["morgans"]}

    def read(split):
        paths = [os.path.join(data_path, split, "gen_" + str(g)) for g in generations[split]]
        X = np.concatenate([np.load(os.path.join(p, "mat_vcf_2d.npy")).astype(np.int8) for p in paths])
        anc = np.concatenate([np.load(os.path.join(p, "mat_map.npy")) for p in paths])
        return X, window_labels(anc, M)

    data = (read("train1"), read("train2"), read("val") if generations.get("val") is not None else (None, None))
    return data, meta
