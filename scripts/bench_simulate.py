#!/usr/bin/env python3
"""Training mode's data at a size a user runs: a 1000-Genomes-like panel (2 000 founders, 7 populations) at the chr22 geometry of
BASELINE config 2 (C = 370 500), default generations, r_admixed = 1, synthetic genotypes from a seed.  One JSON line:

  plan_s            host draws (gnomix_amd.simulate.plan_splits: splits + every haplotype's segments)
  founders_ms       the panel's haplotypes built in HBM from its 2-bit rows (gnx_gt2_to_x_dev), device events
  simulate_ms       gnx_simulate_admix_dev (validation + k_sim_admix), device events; best of --reps
  bytes / frac_8TBps  the bytes the expansion must move (founder bytes read + X written + window labels + ancestry rows if asked)
                    over simulate_ms, and that rate over 8 TB/s
  train_s           HipGnomix.train on the simulated splits (--train; host round trip included)

The kernel's own time comes from `rocprofv3 --kernel-trace --stats` in a separate run of this script.
--reference-cpu F: instead, time the reference's own LAIDataset.simulate loop on the CPU for a fraction F of train1's individuals
of one generation (needs the reference checkout, GNOMIX_REFERENCE; scikit-allel is stubbed); no GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class SyntheticPanel(dict):
    """the parts of a parsed VCF that plan_splits and the device founders read"""

    def __init__(self, n_samples, C, seed):
        rng = np.random.default_rng(seed)
        pos = np.sort(rng.choice(np.arange(16_050_000, 51_240_000), C, replace=False)).astype(np.int64)
        super().__init__({"variants/POS": pos, "variants/REF": np.array(["A"] * C), "variants/ALT": np.array([["C", "", ""]] * C),
                          "samples": np.array(["HG%05d" % i for i in range(n_samples)])})
        ldg = (2 * n_samples + 3) // 4
        self.gt2 = rng.integers(0, 256, size=(C, ldg), dtype=np.uint8) & np.uint8(0x55)   # 2-bit fields holding 0 / 1 only


def genetic_map(pos, seed):
    import pandas as pd
    rng = np.random.default_rng(seed + 1)
    mpos = np.linspace(pos[0], pos[-1], 4000).astype(np.int64)
    cm = np.concatenate([[0.0], np.cumsum(rng.gamma(2.0, 72.0 / 2.0 / 3999, 3999))])
    return pd.DataFrame({"chm": "22", "pos": mpos, "pos_cm": cm})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--founders", type=int, default=2000)
    ap.add_argument("--pops", type=int, default=7)
    ap.add_argument("--C", type=int, default=370_500)
    ap.add_argument("--seed", type=int, default=94305)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--anc", action="store_true", help="also write the per-SNP ancestry rows (mat_map)")
    ap.add_argument("--train", action="store_true", help="also time HipGnomix.train on the simulated data")
    ap.add_argument("--reference-cpu", type=float, default=None)
    a = ap.parse_args()
    from gnomix_amd import simulate as S
    panel = SyntheticPanel(a.founders, a.C, a.seed)
    gmap = genetic_map(panel["variants/POS"], a.seed)
    smap = (list(panel["samples"]), ["POP%d" % (i % a.pops) for i in range(a.founders)])
    if a.reference_cpu:
        return reference_cpu(a, panel, gmap, smap)
    t0 = time.perf_counter()
    plan = S.plan_splits(panel, gmap, smap, {"seed": a.seed}, chm="22")
    plan_s = time.perf_counter() - t0
    M = plan.window_size(0.2)
    import torch
    from gnomix_amd import _lib
    ctx = _lib.default_context(0)
    dev = torch.device("cuda", 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    F = plan.founders_device(ctx, dev)
    ev[1].record()
    torch.cuda.synchronize()
    founders_ms = ev[0].elapsed_time(ev[1])
    plan.simulate_device(ctx, M, want_anc=a.anc, F=F)   # warm-up
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(a.reps):
        ev[0].record()
        X, Y, anc = plan.simulate_device(ctx, M, want_anc=a.anc, F=F)
        ev[1].record()
        torch.cuda.synchronize()
        best = min(best, ev[0].elapsed_time(ev[1]))
    N, C, W = plan.N, plan.C, plan.C // M
    nbytes = N * C + N * C + 4 * N * W + (N * C if a.anc else 0)   # founder byte read + X byte written per SNP, labels, ancestry
    out = {"metric": "simulate_admix", "founders": a.founders, "pops": a.pops, "C": C, "M": M, "N_haplotypes": N, "segments": int(plan.seg_off[-1]),
           "plan_s": round(plan_s, 3), "founders_ms": round(founders_ms, 3), "simulate_ms": round(best, 3), "bytes": nbytes,
           "GBps": round(nbytes / best / 1e6, 1), "frac_8TBps": round(nbytes / best / 1e6 / 8000, 3), "anc": bool(a.anc)}
    # the device result against the host expansion on a sample of rows
    Xh = X[:64, :C].cpu().numpy()
    Fh = F.cpu().numpy()
    Xn, _ = S.expand_numpy(Fh, plan.seg_off[:65], plan.seg_begin[:plan.seg_off[64]], plan.seg_src[:plan.seg_off[64]], plan.anc_of_src, C)
    out["rows_checked_equal"] = bool(np.array_equal(Xh, Xn))
    del Fh, Xh, Xn
    if a.train:
        from gnomix_amd.cli import _initial_model
        from gnomix_amd.gnomix import HipGnomix
        t0 = time.perf_counter()
        data = plan.as_splits(X[:, :C].cpu().numpy(), Y.cpu().numpy())
        d = _initial_model(C, M, plan.A, 75, int(M * 0.5), "default", a.seed,
                           {"snp_pos": plan.meta["pos_snps"], "snp_ref": plan.meta["ref_snps"], "snp_alt": plan.meta["alt_snps"], "pop_order": plan.pop_order})
        del X, Y, anc, F
        torch.cuda.empty_cache()
        g = HipGnomix(d, ctx=ctx)
        g.train(data)
        out["train_s"] = round(time.perf_counter() - t0, 2)
        out["simulate_plus_train_s"] = round(plan_s + founders_ms / 1e3 + best / 1e3 + out["train_s"], 2)
        out["val_smooth_acc"] = g.accuracies.get("smooth_val_acc")
    print(json.dumps(out))


def reference_cpu(a, panel, gmap, smap):
    """the reference's LAIDataset.simulate on the same panel, for a fraction of train1's individuals of generation 8"""
    import tempfile
    import types
    ref = os.environ.get("GNOMIX_REFERENCE", "/root/reference")
    sys.modules.setdefault("allel", types.ModuleType("allel"))
    sys.path.insert(0, ref)
    from src import laidataset as L
    from gnomix_amd import simulate as S
    C, n = a.C, a.founders
    codes = ((panel.gt2[:, :, None] >> (2 * np.arange(4))) & 3).reshape(C, -1)[:, :2 * n].astype(np.int8)
    ds = L.LAIDataset.__new__(L.LAIDataset)
    np.random.seed(a.seed)
    ds.chm, ds.pos_snps, ds.num_snps = "22", panel["variants/POS"], C
    ds.ref_snps, ds.alt_snps = panel["variants/REF"], panel["variants/ALT"][:, 0]
    ds.call_data, ds.vcf_samples = codes.reshape(C, n, 2), panel["samples"]
    ds.morgans, ds.breakpoint_prob = S.chm_info(gmap, ds.pos_snps)
    with tempfile.TemporaryDirectory() as td:
        sm = os.path.join(td, "smap.tsv")
        with open(sm, "w") as f:
            f.writelines("%s\t%s\n" % sp for sp in zip(*smap))
        t0 = time.perf_counter()
        ds.buildDataset(sm)
        ds.create_splits({"train1": 0.8, "train2": 0.15, "val": 0.05})
        t_build = time.perf_counter() - t0
        k = max(1, int(a.reference_cpu * int(len(ds.return_split("train1")) / 8)))
        t0 = time.perf_counter()
        ds.simulate(k, split="train1", gen=8, return_out=False, outdir=os.path.join(td, "g8"))
        t = time.perf_counter() - t0
    print(json.dumps({"metric": "reference_simulate_cpu", "C": C, "founders": n, "individuals": k, "generation": 8, "seconds": round(t, 3),
                      "seconds_per_individual": round(t / k, 4), "build_founders_s": round(t_build, 2)}))


if __name__ == "__main__":
    main()
