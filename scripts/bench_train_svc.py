#!/usr/bin/env python3
"""Training the CovRSK SVC base (mode "best") at config 3's geometry on ONE GPU (scripts/bench_configs.py:c3: C = 250 400, M = 175,
windows of 349 SNPs, A = 7, W = 1 430, 1 400 training haplotypes = 200 per class in every window), next to sklearn's libsvm on the
same Gram matrices for a sample of windows, extrapolated to all windows over 16 host cores.  Prints one JSON line.

  python scripts/bench_train_svc.py [n_cpu_windows]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from gnomix_amd import train

C, M, A, ctx, PER_CLASS = 250_400, 175, 7, 87, 200
W, N = C // M, A * PER_CLASS
HOST_CORES = 16
n_cpu = int(sys.argv[1]) if len(sys.argv) > 1 else 2

rng = np.random.RandomState(3)
# every window holds 200 rows of each ancestry; a row's SNPs in a window follow that ancestry's allele frequencies
freq = rng.uniform(0.05, 0.95, size=(A, C)).astype(np.float32)
y = np.stack([rng.permutation(np.repeat(np.arange(A), PER_CLASS)) for _ in range(W)], axis=1).astype(np.int32)
X = np.empty((N, C), np.int8)
for w in range(W):
    c0, c1 = w * M, (C if w == W - 1 else (w + 1) * M)
    X[:, c0:c1] = rng.random_sample((N, c1 - c0)).astype(np.float32) < freq[y[:, w]][:, c0:c1]
X[rng.random_sample(X.shape) < 0.01] = 2
widths = [M + 2 * ctx + (C - M * W if w == W - 1 else 0) for w in range(W)]
seeds = train.svc_seed_chain(widths, 12345)

Cw = M * 3 + 1   # warm-up: context, code objects, first allocations (three windows of the same shape)
train.train_svc_arrays(X[:, :Cw], y[:, :3], M, ctx, A, seeds[:3])
t0 = time.perf_counter()
res, info = train.train_svc_arrays(X, y, M, ctx, A, seeds)
t_e2e = time.perf_counter() - t0
compares = sum(N * (N + 1) / 2 * wd for wd in widths)   # symbol compares of the upper triangles

out = {"config": "train CovRSK SVC base, config-3 geometry C=250400 M=175 width 349 (last 499) A=7 W=1430 N=1400 (200 per class)",
       "gram_ms": round(info["gram_ms"], 1), "gram_symbol_compares_per_s": compares / (info["gram_ms"] / 1e3),
       "smo_ms": round(info["smo_ms"], 1), "smo_iterations": info["smo_iterations"],
       "smo_iterations_per_s": info["smo_iterations"] / (info["smo_ms"] / 1e3), "solves": info["n_solves"],
       "platt_assembly_ms": round(info["platt_ms"], 1), "guarded_solves": info["n_guarded"], "end_to_end_s": round(t_e2e, 2),
       "mean_support_vectors_per_window": float(np.mean(res["n_sv"]))}

# CPU: sklearn's libsvm (the reference's solver) on the same Gram matrices, a sample of windows, one core each
try:
    from sklearn.svm import SVC
    from oracle import gnx_oracle as O
    O.build()
    t_fit, same = 0.0, True
    for w in range(n_cpu):
        Xw = X[:, train.window_columns(C, M, ctx, w)]
        K = O.covrsk(Xw, Xw).astype(np.float64)
        rs = np.random.RandomState(0)
        t1 = time.perf_counter()
        sk = SVC(kernel="precomputed", probability=True, random_state=rs).fit(K, y[:, w])
        t_fit += time.perf_counter() - t1
        same &= np.array_equal(sk.support_, res["support"][w, :res["n_sv"][w]])   # the full fit does not depend on the seed
    per_window = t_fit / n_cpu
    out["cpu_libsvm_s_per_window"] = round(per_window, 3)
    out["cpu_libsvm_all_windows_16_cores_s_extrapolated"] = round(per_window * W / HOST_CORES, 1)
    out["cpu_note"] = ("sklearn SVC(precomputed, probability=True) on the oracle's Gram, %d windows timed on one core, extrapolated to "
                       "%d windows over %d cores; the reference's own numpy kernel time comes on top" % (n_cpu, W, HOST_CORES))
    out["cpu_support_identical"] = bool(same)
    out["speedup_vs_cpu_extrapolated"] = round(per_window * W / HOST_CORES / t_e2e, 1)
except ImportError as e:
    out["cpu_libsvm_s_per_window"] = None
    out["cpu_note"] = "not measured: %s" % e
print(json.dumps(out))
