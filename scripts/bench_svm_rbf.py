#!/usr/bin/env python3
"""The RBF SVC base (SVMBase: SVC(C=100, gamma=0.001, probability=True)) on ONE GPU at config 3's geometry (chr1 array: C = 250 400,
M = 175, windows of 349 SNPs, A = 7, W = 1 430, 1 400 support vectors per window, 4 096 query haplotypes) and at chr22 / M = 1 000:
inference ms per pass and the int8 MFMA rate of the distance tiles against the matrix-core peak, the trainer's gram / smo / platt
times on a slice of windows, and sklearn's predict_proba / fit on a sample of windows extrapolated to all windows over 16 host
cores (stated as such).  Prints one JSON line per geometry.

  python scripts/bench_svm_rbf.py [c3|chr22|all] [n_cpu_windows] [n_train_windows]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from gnomix_amd import DeviceModel, train

I8_MFMA_PEAK_TOPS = 3944.0   # bench.py: int8 MFMA 16x16x64 measured ceiling
HOST_CORES = 16
which = sys.argv[1] if len(sys.argv) > 1 else "all"
n_cpu = int(sys.argv[2]) if len(sys.argv) > 2 else 2
n_train = int(sys.argv[3]) if len(sys.argv) > 3 else 32
GEOS = {"c3": dict(C=250_400, M=175, ctx=87, A=7, per_class=200, Nq=4096),
        "chr22": dict(C=317_408 + 123, M=1000, ctx=500, A=7, per_class=200, Nq=4096)}


def run(name, C, M, ctx, A, per_class, Nq):
    rng = np.random.RandomState(3)
    W, N, P = C // M, A * per_class, A * (A - 1) // 2
    freq = rng.uniform(0.05, 0.95, size=(A, C)).astype(np.float32)
    d = train.untrained_model(C, M, A, 75, ctx, "default", base="svm")
    # every support vector of a window follows its class's allele frequencies; coefficients in libsvm's range for C = 100
    for w in range(W):
        cols = train.window_columns(C, M, ctx, w)
        cls = np.repeat(np.arange(A), per_class)
        xf = (rng.random_sample((N, len(cols))).astype(np.float32) < freq[cls][:, cols]).astype(np.int8)
        d.svc[w] = dict(xfit=xf, support=np.arange(N, dtype=np.int32), dual_coef=rng.uniform(-100, 100, (A - 1, N)),
                        intercept=rng.normal(size=P), prob_a=-rng.uniform(0.5, 3, P), prob_b=rng.normal(0, 0.3, P),
                        n_support=np.full(A, per_class, np.int32), kernel=np.array("rbf"), gamma=np.float64(0.001))
    yq = rng.randint(0, A, Nq)
    Xq = (rng.random_sample((Nq, C)).astype(np.float32) < freq[yq]).astype(np.int8)
    Xq[rng.random_sample(Xq.shape) < 0.01] = 2
    dev = DeviceModel(d)
    import torch
    Xd = torch.from_numpy(Xq).cuda()
    for _ in range(2):
        dev.base_predict_device(Xd, f64=True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        dev.base_predict_device(Xd, f64=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(ts))
    widths = [d.window_width(w) for w in range(W)]
    ops = sum(2.0 * Nq * N * ((wd + 63) // 64 * 64) for wd in widths)
    out = {"config": "RBF SVC base %s C=%d M=%d ctx=%d A=%d W=%d n_sv=%d N=%d" % (name, C, M, ctx, A, W, N, Nq),
           "inference_ms_median_of_5": round(ms, 2), "inference_ms_all": [round(t, 2) for t in ts], "haplotypes_per_s": Nq / (ms / 1e3),
           "int8_mfma_tops": ops / (ms / 1e3) / 1e12, "int8_mfma_frac_of_peak": ops / (ms / 1e3) / 1e12 / I8_MFMA_PEAK_TOPS}
    # sklearn predict_proba of the same windows (fitted objects are not needed: the restated model is the same arithmetic) is
    # measured on live fits below, together with the fit
    Wt = min(n_train, W)
    Ct = Wt * M + (C - W * M)
    yt = np.stack([rng.permutation(np.repeat(np.arange(A), per_class)) for _ in range(Wt)], axis=1).astype(np.int32)
    Xt = np.empty((N, Ct), np.int8)
    for w in range(Wt):
        c0, c1 = w * M, (Ct if w == Wt - 1 else (w + 1) * M)
        Xt[:, c0:c1] = rng.random_sample((N, c1 - c0)).astype(np.float32) < freq[yt[:, w]][:, c0:c1]
    seeds = np.arange(Wt, dtype=np.uint32) + 7
    train.train_svc_arrays(Xt[:, :2 * M + Ct - Wt * M], yt[:, :2], M, ctx, A, seeds[:2], kernel="rbf")   # warm-up
    t0 = time.perf_counter()
    res, info = train.train_svc_arrays(Xt, yt, M, ctx, A, seeds, kernel="rbf")
    out.update({"train_windows": Wt, "train_end_to_end_s": round(time.perf_counter() - t0, 2), "gram_ms": round(info["gram_ms"], 2),
                "smo_ms": round(info["smo_ms"], 1), "platt_ms": round(info["platt_ms"], 1), "smo_iterations": info["smo_iterations"],
                "guarded_solves": info["n_guarded"], "mean_support_vectors": float(np.mean(res["n_sv"])),
                "train_s_extrapolated_to_all_windows": (info["gram_ms"] + info["smo_ms"] + info["platt_ms"]) / 1e3 * W / Wt})
    try:
        from sklearn.svm import SVC
        t_fit = t_pred = 0.0
        for w in range(min(n_cpu, Wt)):
            cols = train.window_columns(Ct, M, ctx, w)
            t1 = time.perf_counter()
            sk = SVC(C=100., gamma=0.001, probability=True, random_state=np.random.RandomState(0)).fit(Xt[:, cols], yt[:, w])
            t_fit += time.perf_counter() - t1
            t1 = time.perf_counter()
            sk.predict_proba(Xq[:, cols])
            t_pred += time.perf_counter() - t1
        k = min(n_cpu, Wt)
        if k > 0:
            out.update({"sklearn_windows_sampled": k, "sklearn_fit_s_per_window_one_core": t_fit / k,
                        "sklearn_fit_s_all_windows_16_cores_extrapolated": t_fit / k * W / HOST_CORES,
                        "sklearn_predict_proba_s_per_window_one_core": t_pred / k,
                        "sklearn_predict_proba_s_all_windows_16_cores_extrapolated": t_pred / k * W / HOST_CORES})
    except ImportError:
        out["sklearn"] = "not importable"
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    for k, g in GEOS.items():
        if which in ("all", k):
            run(k, **g)
