#!/usr/bin/env python3
"""The boosted-tree base trainer (gnx_train_gbt_base: XGBBase's 20 rounds of depth-4 trees per window) on ONE GPU at chr22 geometry:
W = 317 windows of 2 000 SNPs (M = 1 000, context 500; the last window 2 531), A = 7, N = 4 000 admixed haplotypes resident in HBM.
End-to-end seconds (one warm-up, median of `reps` runs), then one more run with the library's phase timer on (a stream
synchronisation per phase: gradients + loss, per-level sums, split search, row partition, leaves + margins).  xgboost is absent and
cannot be timed; beside the GPU figure stands the plain-Python restatement (tests/gbt_base_exact.py) on ONE window and `cpu_rounds`
rounds, extrapolated to all rounds and windows and labelled as such.  Prints one JSON line; `--out FILE` also writes it.

  python scripts/bench_train_forest.py [--reps 3] [--cpu-rounds 1] [--small] [--out profiles/train_forest_chr22.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from gnomix_amd import _lib, synth, train

PHASES = ("gradients_and_loss_ms", "histogram_ms", "split_search_ms", "partition_ms", "leaves_and_margins_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-rounds", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="a twentieth of the windows (a quick look, not the quoted figure)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    M, ctx, A, N, rounds, depth = 1000, 500, 7, 4000, 20, 4
    C = (16 if a.small else 317) * M + 408 + 123
    W = C // M
    X, y, _ = synth.synthetic_admixed_device(N // 2, C, M, A, "cuda:0", seed=7)
    yd = torch.as_tensor(y, device="cuda:0")
    c = _lib.default_context(0)
    fit = lambda: train.train_forest_arrays(X, yd, M, ctx, A, n_rounds=rounds, max_depth=depth, ctx=c)
    c.lib.gnx_train_gbt_base_phases(0, None)
    fit()                                              # warm-up
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fb, loss = fit()
        ts.append(time.perf_counter() - t0)
    ms = (ctypes.c_double * 5)()
    c.lib.gnx_train_gbt_base_phases(1, None)
    t0 = time.perf_counter()
    fit()
    t_prof = time.perf_counter() - t0
    c.lib.gnx_train_gbt_base_phases(0, ctypes.addressof(ms))
    out = {"config": "boosted-tree base trainer chr22 C=%d M=%d ctx=%d A=%d W=%d N=%d rounds=%d depth=%d" % (C, M, ctx, A, W, N, rounds, depth),
           "train_s_median": round(float(np.median(ts)), 3), "train_s_all": [round(t, 3) for t in ts], "reps": a.reps, "warmup": 1,
           "trees": int(len(fb["fb_tree_off"]) - 1), "nodes": int(len(fb["fb_left"])), "loss_first": float(loss[0]), "loss_last": float(loss[-1]),
           "phase_run_s": round(t_prof, 3), "phases": {k: round(float(v), 1) for k, v in zip(PHASES, ms)}}
    if a.cpu_rounds > 0:
        import gbt_base_exact as E
        Xw = X[:, torch.as_tensor(train.window_columns(C, M, ctx, 0), device=X.device)].cpu().numpy()
        t0 = time.perf_counter()
        E.train_window(Xw, y[:, 0], A, n_rounds=a.cpu_rounds, max_depth=depth)
        t = time.perf_counter() - t0
        out.update({"python_restatement_one_window_rounds": a.cpu_rounds, "python_restatement_one_window_s": round(t, 2),
                    "python_restatement_s_extrapolated_to_all_rounds_and_windows_one_core": round(t / a.cpu_rounds * rounds * W, 1)})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
