#!/usr/bin/env python3
"""Generate tests/golden/G21_sim/ by RUNNING the reference's simulator (src/laidataset.py) and label reduction
(src/preprocess.py) on a tiny panel; the reference is imported read-only from /root/reference (GNOMIX_REFERENCE), nothing of it is
copied here.  scikit-allel is absent: an empty stub stands in for it and the panel arrays are set on a LAIDataset made with
__new__, exactly as LAIDataset.__init__ sets them (np.random.seed(seed) first).

Inputs written:  panel.vcf.gz (60 samples, 3 populations, 500 SNPs, fully called and phased), gmap.tsv, smap.tsv, config.yaml.
Output:          expected.npz — split membership, chm_info, and for every split and generation X bit-packed, the per-SNP ancestry
                 run-length encoded, the window labels of data_process, the sha256 of each .npy the reference wrote.

The panel never triggers include_all's DataFrame.append (removed in pandas >= 2): that branch stays unpinned.
"""
import gzip
import hashlib
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("GNOMIX_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "G21_sim")
SEED = 94305
N_SAMPLES, N_POP, C = 60, 3, 500
WINDOW_CM, SMOOTH = 1.0, 15


def write_inputs(rng):
    os.makedirs(OUT, exist_ok=True)
    pos = np.sort(rng.choice(np.arange(10_000, 5_000_000), C, replace=False))
    # population allele frequencies far apart (the end-to-end GPU test trains on this panel)
    levels = np.array([0.05, 0.5, 0.95])
    freq = np.stack([rng.permutation(levels) for _ in range(C)], axis=1)     # (N_POP, C)
    pop_of = np.array([i % N_POP for i in range(N_SAMPLES)])
    names = ["S%03d" % i for i in range(N_SAMPLES)]
    gt = (rng.uniform(size=(C, N_SAMPLES, 2)) < freq[pop_of].T[:, :, None]).astype(np.int8)   # (C, samples, 2), sample-map order
    # vcf with the samples in another order than the sample map
    order = rng.permutation(N_SAMPLES)
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=22>",
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names[i] for i in order)]
    bases = np.array(list("ACGT"))
    ref = bases[rng.randint(0, 4, C)]
    alt = np.array([bases[(list("ACGT").index(r) + 1 + rng.randint(0, 3)) % 4] for r in ref])
    for v in range(C):
        g = "\t".join("%d|%d" % (gt[v, i, 0], gt[v, i, 1]) for i in order)
        lines.append("22\t%d\trs%d\t%s\t%s\t.\tPASS\t.\tGT\t%s" % (pos[v], v, ref[v], alt[v], g))
    with gzip.open(os.path.join(OUT, "panel.vcf.gz"), "wt", compresslevel=9) as f:
        f.write("\n".join(lines) + "\n")
    # genetic map: starts after the first SNP and ends before the last (interp1d extrapolates at both ends), uneven rates
    mpos = np.linspace(pos[3], pos[-5], 40).astype(np.int64)
    mcm = np.concatenate([[0.0], np.cumsum(rng.gamma(2.0, 0.7, len(mpos) - 1))])
    with open(os.path.join(OUT, "gmap.tsv"), "w") as f:
        f.write("# chm\tpos\tpos_cm\n")
        for p, c in zip(mpos, mcm):
            f.write("chr22\t%d\t%.6f\n" % (p, c))
    with open(os.path.join(OUT, "smap.tsv"), "w") as f:
        for i in range(N_SAMPLES):
            f.write("%s\tPOP%s\n" % (names[i], "BCA"[pop_of[i]]))   # first appearance: B, C, A -> codes 0, 1, 2
    with open(os.path.join(OUT, "config.yaml"), "w") as f:
        f.write("verbose: False\nseed: %d\nsimulation:\n  run: True\n  path:\n  splits:\n    ratios:\n      train1: 0.8\n      train2: 0.15\n"
                "      val: 0.05\n  gens: [0, 2, 4, 6, 8, 12, 16, 24]\n  r_admixed: 1\n  rm_data: False\nmodel:\n  name: model\n  inference:\n"
                "  window_size_cM: %s\n  smooth_size: %d\n  context_ratio: 0.5\n  retrain_base: True\n  calibrate: False\n  n_cores:\n"
                "inference:\n  bed_file_output: False\n  snp_level_inference: False\n  visualize_inference: False\n" % (SEED, WINDOW_CM, SMOOTH))
    return names, order, gt, pos, ref, alt


def rle(row):
    cut = np.flatnonzero(np.diff(row.astype(np.int16))) + 1
    starts = np.concatenate([[0], cut])
    return starts.astype(np.int32), row[starts].astype(np.uint8)


def main():
    if not os.path.isdir(os.path.join(REF, "src")):
        print("reference not found at %s: skipped" % REF)
        return
    sys.modules.setdefault("allel", types.ModuleType("allel"))
    sys.path.insert(0, REF)
    from src import laidataset as L
    from src import preprocess as P
    rng = np.random.RandomState(2024)
    names, order, gt, pos, ref, alt = write_inputs(rng)

    ds = L.LAIDataset.__new__(L.LAIDataset)
    np.random.seed(SEED)
    ds.chm = "22"
    ds.pos_snps = pos.astype(np.int32)
    ds.num_snps = C
    ds.ref_snps = ref.astype(str)
    ds.alt_snps = alt.astype(str)
    ds.call_data = gt[:, order, :]
    ds.vcf_samples = np.array([names[i] for i in order], dtype=object)
    ds.morgans, ds.breakpoint_prob = L.get_chm_info(os.path.join(OUT, "gmap.tsv"), ds.pos_snps, ds.chm)
    ds.buildDataset(os.path.join(OUT, "smap.tsv"))
    ratios = {"train1": 0.8, "train2": 0.15, "val": 0.05}
    gens = [0, 2, 4, 6, 8, 12, 16, 24]
    split_gens = {"train1": list(set(gens + [0])), "train2": gens, "val": [g for g in gens if g != 0]}
    out = {"morgans": np.float64(ds.morgans), "bp": ds.breakpoint_prob}
    M = int(round(WINDOW_CM * (C / (100 * ds.morgans))))
    M = M + 1 if C % M == 0 else M
    out["M"] = M
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, "sample_maps"))
        ds.create_splits(ratios, os.path.join(td, "sample_maps"))
        for split in ratios:
            out["split_" + split] = np.array(list(ds.return_split(split)["sample"]), dtype="U")
            with open(os.path.join(td, "sample_maps", split + ".map"), "rb") as f:
                out["sha_map_" + split] = np.array(hashlib.sha256(f.read()).hexdigest())
            total = max(len(ds.return_split(split)) * 1, {"train1": 800, "train2": 150, "val": 50}[split])
            n_out = int(total / len(split_gens[split]))
            out["gens_" + split] = np.array(split_gens[split])
            for g in split_gens[split]:
                d = os.path.join(td, split, "gen_%d" % g)
                ds.simulate(n_out, split=split, gen=g, outdir=d, return_out=False)
                key = "%s_gen%d" % (split, g)
                for fn in ("mat_vcf_2d.npy", "mat_map.npy"):
                    with open(os.path.join(d, fn), "rb") as f:
                        out["sha_%s_%s" % (key, fn[:-4])] = np.array(hashlib.sha256(f.read()).hexdigest())
                X = np.load(os.path.join(d, "mat_vcf_2d.npy"))
                anc = np.load(os.path.join(d, "mat_map.npy"))
                assert X.dtype == np.uint8 and anc.dtype == np.uint8 and X.max() <= 1
                out["X_" + key] = np.packbits(X, axis=1)
                out["shape_" + key] = np.array(X.shape)
                st, val, off = [], [], [0]
                for row in anc:
                    s, v = rle(row)
                    st.append(s); val.append(v); off.append(off[-1] + len(s))
                out["anc_start_" + key] = np.concatenate(st)
                out["anc_val_" + key] = np.concatenate(val)
                out["anc_off_" + key] = np.array(off, np.int64)
                _, y = P.data_process(P.load_np_data([os.path.join(d, "mat_vcf_2d.npy")]), P.load_np_data([os.path.join(d, "mat_map.npy")]), M)
                out["y_" + key] = y.astype(np.int8)
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **out)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("wrote %s (%d bytes in all)" % (OUT, total))


if __name__ == "__main__":
    main()
