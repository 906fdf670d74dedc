#!/usr/bin/env python3
"""The string-kernel SVC trainers (gnx_train_svc_poly: PolynomialStringKernelBase; gnx_train_svc2 with the plain kernel:
StringKernelBase; and CovRSK for comparison) on ONE GPU: one warm-up and `reps` fits per kernel at one geometry, the median of the
device times gnx_svc_train_info reports (gram_ms: k_svc_pack + k_svc_gram / k_svc_gram_poly; smo_ms: k_svc_smo; platt_ms:
k_svc_heldout + k_svc_sigmoid) and of the wall time of the call (host staging, problem layout and assembly included).

  sim     the train1 split of the simulated data tests/test_gpu_train_svc.py::test_best_model_trains_end_to_end fits
          (tests/golden/G21_sim)
  chr22   16 windows of chr22's width (M = 1 168, context 584: 2 336 SNPs per window), A = 3, N = 1 000 synthetic admixed haplotypes:
          one batch of windows

Prints one JSON line per geometry; `--out FILE` appends them.

  python scripts/bench_train_sk.py [sim|chr22|all] [--reps 3] [--out profiles/sk_train_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from gnomix_amd import _lib, train

KERNELS = ("poly_kernel", "string_kernel", "CovRSK")


def sim_geometry(ctx):
    import yaml
    from gnomix_amd import simulate as S
    g = os.path.join(ROOT, "tests", "golden", "G21_sim")
    with open(os.path.join(g, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    plan = S.plan_splits(os.path.join(g, "panel.vcf.gz"), os.path.join(g, "gmap.tsv"), os.path.join(g, "smap.tsv"), cfg, chm="22")
    M = plan.window_size(cfg["model"]["window_size_cM"])
    X, y = plan.materialise(ctx, M=M)[0]
    return np.asarray(X), np.asarray(y), M, int(M * cfg["model"]["context_ratio"]), plan.A


def chr22_geometry(W=16, M=1168, cx=584, A=3, N=1000):
    rng = np.random.RandomState(22)
    C = W * M
    f = rng.uniform(0.05, 0.95, (A, C))
    y = np.empty((N, W), np.int32)
    for i in range(N):
        cut = rng.randint(0, W + 1)
        y[i, :cut], y[i, cut:] = rng.randint(A), rng.randint(A)
    y[:A] = np.arange(A)[:, None]
    anc = np.repeat(y, M, axis=1)
    X = (rng.uniform(size=(N, C)) < f[anc, np.arange(C)[None, :]]).astype(np.int8)
    X[rng.uniform(size=X.shape) < 0.01] = 2
    return X, y, M, cx, A


def measure(name, X, y, M, cx, A, reps, ctx):
    N, C = X.shape
    W = C // M
    seeds = np.random.RandomState(5).randint(train.SVC_SEED_HIGH, size=W).astype(np.uint32)
    out = {"config": "string-kernel SVC trainers, %s: N=%d C=%d M=%d ctx=%d (windows of %d SNPs, the last %d) W=%d A=%d" %
                     (name, N, C, M, cx, M + 2 * cx, M + 2 * cx + C % M, W, A), "reps": reps, "warmup": 1, "statistic": "median"}
    for kernel in KERNELS:
        fit = lambda: train.train_svc_arrays(X, y, M, cx, A, seeds, kernel=kernel, ctx=ctx)
        fit()
        rows = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _, info = fit()
            rows.append(dict(info, wall_ms=(time.perf_counter() - t0) * 1e3))
        out[kernel] = {k: round(float(np.median([r[k] for r in rows])), 3) for k in ("gram_ms", "smo_ms", "platt_ms", "wall_ms")}
        out[kernel].update(smo_iterations=int(rows[0]["smo_iterations"]), n_solves=int(rows[0]["n_solves"]), n_guarded=int(rows[0]["n_guarded"]),
                           gram_ms_all=[round(float(r["gram_ms"]), 3) for r in rows])
    out["poly_gram_over_covrsk_gram"] = round(out["poly_kernel"]["gram_ms"] / max(out["CovRSK"]["gram_ms"], 1e-9), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="?", default="all", choices=("sim", "chr22", "all"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    for name in (("sim", "chr22") if a.which == "all" else (a.which,)):
        X, y, M, cx, A = sim_geometry(ctx) if name == "sim" else chr22_geometry()
        line = json.dumps(measure(name, X, y, M, cx, A, a.reps, ctx))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
