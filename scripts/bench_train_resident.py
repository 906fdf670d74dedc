#!/usr/bin/env python3
"""Training from host arrays against training from device-resident splits, end to end, in one process: the panel, geometry and
sizes of scripts/bench_simulate.py (2 000 founders of 7 populations, chr22's C = 370 500 SNPs, the default generations, windows of
0.2 cM, S = 75, context ratio 0.5, mode "default").  Each route runs --reps times, alternating, from the same plan and the same
numpy seed:

  host      plan.materialise      (X, y copied to numpy arrays)  + HipGnomix.train on numpy arrays
  resident  plan.materialise_dev  (X, y stay CUDA tensors)       + HipGnomix.train on those tensors

One JSON line per run (route, simulate_s, train_s, total_s, pcie_bytes) and a last line with the medians, the spread (min .. max),
and whether both routes trained the same model.  pcie_bytes is computed from the shapes of what each step moves between host and
device (the library keeps no transfer counters): see pcie_bytes() below.  Run it on an otherwise idle GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def pcie_bytes(route, plan, M, A, n1, n2, nv, calibrate):
    """bytes crossing the host link in materialise + train, from shapes.  X rows are C int8, labels W int32, base probabilities
    W * A float64, smoother labels W int32.
    host: the simulator stages the founders in and X, y out; every train / predict call stages its inputs in and its outputs out:
      base fit (X_t1, y_t1 in), B_t2 (X_t2 in, B out), smoother fit (B_t2, y_t2 in), [calibrator: X_t1 in, B out, 5 % of B in, as
      float32 out], scoring train (X_t1 in, B out, B in, labels out, B_t2 in, labels out), scoring val (X_v in, B out, B in, labels
      out), retrain (all X, y in).
    resident: the panel's 2-bit rows and the segment tables in; the calibrator's 5 % sample out.  (Fitted arrays and the A x A
      counts come back on both routes and are left out of both.)"""
    C, W, N = plan.C, plan.C // M, plan.N
    x, y, b, lab = C, 4 * W, 8 * W * A, 4 * W
    tables = plan.seg_off.nbytes + plan.seg_begin.nbytes + plan.seg_src.nbytes + plan.anc_of_src.nbytes
    cal = int(0.05 * n1)
    if route == "resident":
        return int(plan.panel.gt2.nbytes + tables + (cal * (W * A * 4 + y) if calibrate else 0))
    founders = 2 * len(plan.panel["samples"]) * C
    total = founders + tables + N * (x + y)                     # simulate_host
    total += n1 * (x + y) + n2 * (x + b) + n2 * (b + y)         # base fit, B_t2, smoother fit
    if calibrate:
        total += n1 * (x + b) + cal * (b + W * A * 4)
    total += n1 * (x + b + b + lab) + n2 * (b + lab)            # scoring: train
    total += nv * (x + b + b + lab)                             # scoring: val
    total += N * (x + y)                                        # retrain on everything
    return int(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--founders", type=int, default=2000)
    ap.add_argument("--pops", type=int, default=7)
    ap.add_argument("--C", type=int, default=370_500)
    ap.add_argument("--seed", type=int, default=94305)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calibrate", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from bench_simulate import SyntheticPanel, genetic_map
    from gnomix_amd import _lib, simulate as S
    from gnomix_amd.cli import _initial_model
    from gnomix_amd.gnomix import HipGnomix
    panel = SyntheticPanel(a.founders, a.C, a.seed)
    # the host route stages the founders from the parsed VCF's genotype array: the same alleles as the 2-bit rows
    panel["calldata/GT"] = np.ascontiguousarray(((panel.gt2[:, :, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3)
                                                .reshape(a.C, -1)[:, :2 * a.founders].astype(np.int8).reshape(a.C, a.founders, 2))
    gmap = genetic_map(panel["variants/POS"], a.seed)
    smap = (list(panel["samples"]), ["POP%d" % (i % a.pops) for i in range(a.founders)])
    plan = S.plan_splits(panel, gmap, smap, {"seed": a.seed}, chm="22")
    M, C, A = plan.window_size(0.2), plan.C, plan.A
    meta = {"snp_pos": plan.meta["pos_snps"], "snp_ref": plan.meta["ref_snps"], "snp_alt": plan.meta["alt_snps"], "pop_order": plan.pop_order}
    ctx = _lib.default_context(0)
    sl = plan.split_slices()
    n1, n2, nv = (sl[s][1] - sl[s][0] if s in sl else 0 for s in ("train1", "train2", "val"))
    lines, models = [], {}

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def run(route, rep):
        np.random.seed(a.seed)
        g = HipGnomix(_initial_model(C, M, A, 75, int(M * 0.5), "default", a.seed, meta), ctx=ctx, calibrate=a.calibrate)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = plan.materialise_dev(ctx, M=M) if route == "resident" else plan.materialise(ctx, M=M)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        g.train(data)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        emit({"metric": "train_resident", "route": route, "rep": rep, "simulate_s": round(t1 - t0, 3), "train_s": round(t2 - t1, 3),
              "total_s": round(t2 - t0, 3), "pcie_bytes": pcie_bytes(route, plan, M, A, n1, n2, nv, a.calibrate),
              "smooth_val_acc": g.accuracies.get("smooth_val_acc")})
        models[route] = g.dev.data
        del data, g
        torch.cuda.empty_cache()
        return t2 - t0

    run("resident", -1)   # warm-up of both routes (allocator, code objects, workspaces): not counted
    run("host", -1)
    lines.clear()
    T = {"host": [], "resident": []}
    for rep in range(a.reps):
        for route in ("host", "resident"):
            T[route].append(run(route, rep))
    h, r = models["host"], models["resident"]
    same = all(np.array_equal(getattr(h, k), getattr(r, k)) for k in ("lr_coef", "lr_intercept", "tree_off", "left", "right", "feat", "cond"))
    emit({"metric": "train_resident_summary", "C": C, "M": M, "A": A, "N_haplotypes": plan.N, "rows": [n1, n2, nv], "reps": a.reps,
          "calibrate": bool(a.calibrate),
          **{"%s_total_s" % k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in T.items()},
          "speedup_median": round(statistics.median(T["host"]) / statistics.median(T["resident"]), 3),
          "pcie_bytes": {k: pcie_bytes(k, plan, M, A, n1, n2, nv, a.calibrate) for k in T}, "same_model": bool(same)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
