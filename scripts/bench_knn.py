#!/usr/bin/env python3
"""The 1-nearest-neighbour base (KNNBase: KNeighborsClassifier(n_neighbors=1) per window) on ONE GPU at config 3's geometry (chr1
array: C = 250 400, M = 175, windows of 349 SNPs, A = 7, W = 1 430) and at chr22 / M = 1 000, with 1 400 fit rows per window and
4 096 query haplotypes — the geometry of scripts/bench_svm_rbf.py, whose k_rbf_dec<64> is the same distance arithmetic plus a
float64 epilogue (profiles/r08_svm_rbf_bench.jsonl holds its time).  One warm-up, then the median of three passes; the int8 MFMA
rate of the distance tiles against the matrix-core peak; beside it sklearn's predict_proba of ONE window on one host core, and
that time multiplied out to all windows over 16 cores — an EXTRAPOLATION, labelled as such.  Prints one JSON line per geometry.

  python scripts/bench_knn.py [c3|chr22|all] [n_cpu_windows]"""
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
n_cpu = int(sys.argv[2]) if len(sys.argv) > 2 else 1
GEOS = {"c3": dict(C=250_400, M=175, ctx=87, A=7, per_class=200, Nq=4096),
        "chr22": dict(C=317_408 + 123, M=1000, ctx=500, A=7, per_class=200, Nq=4096)}
RBF_MS = {}   # the yardstick: k_rbf_dec at the same geometry, as recorded
try:
    for ln in open(os.path.join(ROOT, "profiles", "r08_svm_rbf_bench.jsonl")):
        r = json.loads(ln)
        RBF_MS[r["config"].split()[3]] = r["inference_ms_median_of_5"]
except (OSError, ValueError, KeyError, IndexError):
    pass


def run(name, C, M, ctx, A, per_class, Nq):
    rng = np.random.RandomState(3)
    W, N = C // M, A * per_class
    freq = rng.uniform(0.05, 0.95, size=(A, C)).astype(np.float32)
    # the shared form: the same N haplotypes are every window's fit rows, each window with its own labels; a row follows the
    # allele frequencies of its label in that window
    y = np.stack([rng.permutation(np.repeat(np.arange(A), per_class)) for _ in range(W)], axis=1).astype(np.int32)
    anc = np.repeat(y, M, axis=1)
    anc = np.concatenate([anc, np.repeat(anc[:, -1:], C - W * M, axis=1)], axis=1)
    X = (rng.random_sample((N, C)).astype(np.float32) < freq[anc, np.arange(C)[None, :]]).astype(np.int8)
    del anc
    d = train.untrained_model(C, M, A, 75, ctx, "default", base="knn")
    train.train_knn_base(d, X, y)
    yq = rng.randint(0, A, Nq)
    Xq = (rng.random_sample((Nq, C)).astype(np.float32) < freq[yq]).astype(np.int8)
    Xq[rng.random_sample(Xq.shape) < 0.01] = 2
    t0 = time.perf_counter()
    dev = DeviceModel(d)
    load_s = time.perf_counter() - t0
    import torch
    Xd = torch.from_numpy(Xq).cuda()
    dev.base_predict_device(Xd, f64=True)   # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        B = dev.base_predict_device(Xd, f64=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(ts))
    acc = float((B.argmax(-1).cpu().numpy() == yq[:, None]).mean())
    widths = [d.window_width(w) for w in range(W)]
    n_pad = (N + 127) // 128 * 128
    ops = sum(2.0 * Nq * N * ((wd + 63) // 64 * 64) for wd in widths)            # useful: real fit rows, padded row pitch (as bench_svm_rbf.py)
    ops_issued = sum(2.0 * ((Nq + 63) // 64 * 64) * n_pad * ((wd + 63) // 64 * 64) for wd in widths)
    out = {"config": "KNN base %s C=%d M=%d ctx=%d A=%d W=%d n_fit=%d N=%d" % (name, C, M, ctx, A, W, N, Nq),
           "inference_ms_median_of_3": round(ms, 3), "inference_ms_all": [round(t, 3) for t in ts], "haplotypes_per_s": Nq / (ms / 1e3),
           "int8_mfma_tops": ops / (ms / 1e3) / 1e12, "int8_mfma_frac_of_peak": ops / (ms / 1e3) / 1e12 / I8_MFMA_PEAK_TOPS,
           "int8_mfma_tops_issued": ops_issued / (ms / 1e3) / 1e12, "fit_row_bytes": int(sum(n_pad * ((wd + 63) // 64 * 64) for wd in widths)),
           "model_load_s": round(load_s, 2), "window_label_accuracy_of_the_queries": acc}
    if name in RBF_MS:
        out.update({"k_rbf_dec_ms_same_geometry_recorded": RBF_MS[name], "rbf_over_knn_time_ratio": RBF_MS[name] / ms})
    try:
        from sklearn.neighbors import KNeighborsClassifier
        t_pred, k = 0.0, min(n_cpu, W)
        for w in range(k):
            cols = train.window_columns(C, M, ctx, w)
            sk = KNeighborsClassifier(n_neighbors=1, n_jobs=1).fit(X[:, cols], y[:, w])
            xq = Xq[:, cols]
            t1 = time.perf_counter()
            sk.predict_proba(xq)
            t_pred += time.perf_counter() - t1
        if k > 0:
            out.update({"sklearn_windows_sampled": k, "sklearn_predict_proba_s_per_window_one_core": t_pred / k,
                        "sklearn_predict_proba_s_all_windows_16_cores_EXTRAPOLATED": t_pred / k * W / HOST_CORES})
    except ImportError:
        out["sklearn"] = "not importable"
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    for k, g in GEOS.items():
        if which in ("all", k):
            run(k, **g)
