#!/usr/bin/env python3
"""The random-forest base trainer (gnx_train_rforest: RFBase's 20 depth-4 trees per window, scikit-learn's own trees) on ONE GPU at
chr22 geometry: C = 370 500, M = 1 000 (W = 370 windows; context 500, so 2 000 SNPs per window, the last 2 500), A = 7, N = 4 000
admixed haplotypes resident in HBM.  End-to-end seconds (one warm-up, median of `reps` runs; the numpy bootstrap draw on the host is
inside and also reported alone), then one more run with the library's phase timer on (a stream synchronisation per phase: the count
product, the draw, the row partition).  Beside it scikit-learn's own RandomForestClassifier(n_estimators=20, max_depth=4).fit on
`sk_windows` of the same windows, the windows spread over `threads` host threads with n_jobs = 1 each (tree building releases the
interpreter lock), SCALED to all W windows and labelled as such.  Prints one JSON line; `--out FILE` also writes it.

  python scripts/bench_train_rforest.py [--reps 3] [--sk-windows 32] [--threads 16] [--small] [--out profiles/train_rforest_chr22.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from gnomix_amd import _lib, synth, train

PHASES = ("counts_ms", "draw_ms", "partition_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sk-windows", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--small", action="store_true", help="a twentieth of the windows (a quick look, not the quoted figure)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    M, ctx, A, N, T, depth = 1000, 500, 7, 4000, 20, 4
    C = (18 if a.small else 370) * M + 500
    W = C // M
    X, y, _ = synth.synthetic_admixed_device(N // 2, C, M, A, "cuda:0", seed=7)
    yd = torch.as_tensor(y, device="cuda:0")
    c = _lib.default_context(0)
    seeds = np.random.RandomState(22).randint(2 ** 31 - 1, size=W)
    t0 = time.perf_counter()
    train.rforest_bootstrap(seeds, T, N)
    t_boot = time.perf_counter() - t0
    fit = lambda: train.train_rforest_arrays(X, yd, M, ctx, A, seeds, n_trees=T, max_depth=depth, ctx=c)
    c.lib.gnx_train_rforest_phases(0, None)
    fit()                                              # warm-up
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rf = fit()
        ts.append(time.perf_counter() - t0)
    ms = (ctypes.c_double * 3)()
    c.lib.gnx_train_rforest_phases(1, None)
    t0 = time.perf_counter()
    fit()
    t_prof = time.perf_counter() - t0
    c.lib.gnx_train_rforest_phases(0, ctypes.addressof(ms))
    out = {"config": "random-forest base trainer chr22 C=%d M=%d ctx=%d A=%d W=%d N=%d trees=%d depth=%d" % (C, M, ctx, A, W, N, T, depth),
           "train_s_median": round(float(np.median(ts)), 3), "train_s_all": [round(t, 3) for t in ts], "reps": a.reps, "warmup": 1,
           "host_bootstrap_s": round(t_boot, 3), "trees": int(len(rf["rf_tree_off"]) - 1), "nodes": int(len(rf["rf_left"])),
           "phase_run_s": round(t_prof, 3), "phases": {k: round(float(v), 1) for k, v in zip(PHASES, ms)}}
    k = min(a.sk_windows, W)
    if k > 0:
        from concurrent.futures import ThreadPoolExecutor
        from sklearn.ensemble import RandomForestClassifier
        Xw = [X[:, torch.as_tensor(train.window_columns(C, M, ctx, w), device=X.device)].cpu().numpy() for w in range(k)]
        one = lambda w: RandomForestClassifier(n_estimators=T, max_depth=depth, n_jobs=1, random_state=int(seeds[w])).fit(Xw[w], y[:, w])
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=a.threads) as pool:
            models = list(pool.map(one, range(k)))
        t = time.perf_counter() - t0
        same = all(np.array_equal(e.tree_.threshold, rf["rf_thr"][rf["rf_tree_off"][i]:rf["rf_tree_off"][i + 1]])
                   for i, e in enumerate(models[0].estimators_))
        out.update({"sklearn_windows": k, "sklearn_threads": a.threads, "sklearn_s_measured": round(t, 2),
                    "sklearn_s_scaled_to_all_windows": round(t / k * W, 1), "window0_thresholds_equal_sklearn": bool(same)})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
