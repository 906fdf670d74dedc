#!/usr/bin/env python3
"""The Naive-Bayes bases (per-window GaussianNB / BernoulliNB / MultinomialNB as likelihood tables) on ONE GPU at config 3's geometry
(chr1 array: C = 250 400, M = 175, windows of 349 SNPs, A = 7, W = 1 430) and at chr22 / M = 1 000, with 1 400 fit rows and 4 096
query haplotypes — the geometry of scripts/bench_knn.py.  The fit (counts on the device, closed forms on the host) is timed as a
whole and its counting call alone, against the bytes of X the counting kernel reads; the table pass: one warm-up, then the median of
three; float64 MFMAs per second (N / 16 * sum of widths per pass) against the matrix-core rate F64_MFMA_PEAK_TF / 2048 flops per
instruction; resident table bytes; beside it scikit-learn's predict_proba of ONE window on one host core, and that time multiplied
out to all windows over 16 cores — an EXTRAPOLATION, labelled as such.  Prints one JSON line per geometry.

  python scripts/bench_nb.py [c3|chr22|all] [n_cpu_windows] [kind]
  python scripts/bench_nb.py lr_c3|lr_chr22      the same geometry through the float64-MFMA logistic pass (k_base_logistic,
                                                 GNX_BASE_LR_IMPL=f64, set here): random weights, the table pass's yardstick"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

if len(sys.argv) > 1 and sys.argv[1].startswith("lr_"):
    os.environ["GNX_BASE_LR_IMPL"] = "f64"   # read when the context is made

from gnomix_amd import DeviceModel, train

F64_MFMA_PEAK_TF = 78.6      # MI355X float64 matrix peak (vendor figure); one v_mfma_f64_16x16x4_f64 is 2 * 16 * 16 * 4 = 2048 flops
HOST_CORES = 16
which = sys.argv[1] if len(sys.argv) > 1 else "all"
n_cpu = int(sys.argv[2]) if len(sys.argv) > 2 else 1
kind = sys.argv[3] if len(sys.argv) > 3 else "gaussian"
GEOS = {"c3": dict(C=250_400, M=175, ctx=87, A=7, per_class=200, Nq=4096),
        "chr22": dict(C=317_408 + 123, M=1000, ctx=500, A=7, per_class=200, Nq=4096)}


def run(name, C, M, ctx, A, per_class, Nq):
    rng = np.random.RandomState(3)
    W, N = C // M, A * per_class
    freq = rng.uniform(0.05, 0.95, size=(A, C)).astype(np.float32)
    y = np.stack([rng.permutation(np.repeat(np.arange(A), per_class)) for _ in range(W)], axis=1).astype(np.int32)
    anc = np.repeat(y, M, axis=1)
    anc = np.concatenate([anc, np.repeat(anc[:, -1:], C - W * M, axis=1)], axis=1)
    X = (rng.random_sample((N, C)).astype(np.float32) < freq[anc, np.arange(C)[None, :]]).astype(np.int8)
    del anc
    d = train.untrained_model(C, M, A, 75, ctx, "default", base="nb_" + kind)
    train.nb_counts(X[:8], y[:8], M, ctx, A)        # warm-up: context, workspaces
    t0 = time.perf_counter()
    train.nb_counts(X, y, M, ctx, A)
    count_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    train.train_nb_base(d, X, y, kind)
    fit_s = time.perf_counter() - t0
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
    mfmas = (Nq / 16.0) * sum(widths)
    peak = F64_MFMA_PEAK_TF * 1e12 / 2048.0
    out = {"config": "NB base %s %s C=%d M=%d ctx=%d A=%d W=%d n_fit=%d N=%d" % (kind, name, C, M, ctx, A, W, N, Nq),
           "inference_ms_median_of_3": round(ms, 3), "inference_ms_all": [round(t, 3) for t in ts], "haplotypes_per_s": Nq / (ms / 1e3),
           "f64_mfma_per_pass": mfmas, "f64_mfma_per_s": mfmas / (ms / 1e3), "f64_mfma_frac_of_matrix_peak": mfmas / (ms / 1e3) / peak,
           "ms_at_matrix_peak": mfmas / peak * 1e3, "resident_table_bytes": int(sum(widths)) * 512,
           "fit_s_counts_and_closed_forms": round(fit_s, 3), "fit_counts_call_s_with_staging": round(count_s, 3),
           "fit_x_bytes_read_by_the_counting_kernel": int(N) * int(sum(widths)), "model_load_s": round(load_s, 2),
           "window_label_accuracy_of_the_queries": acc}
    try:
        from sklearn.naive_bayes import BernoulliNB, GaussianNB, MultinomialNB
        mk = {"gaussian": GaussianNB, "bernoulli": lambda: BernoulliNB(alpha=1e-10), "multinomial": lambda: MultinomialNB(alpha=1e-10)}[kind]
        t_pred, k = 0.0, min(n_cpu, W)
        for w in range(k):
            cols = train.window_columns(C, M, ctx, w)
            sk = mk().fit(X[:, cols], y[:, w])
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


def run_lr(name, C, M, ctx, A, per_class, Nq):
    import torch
    rng = np.random.RandomState(3)
    d = train.untrained_model(C, M, A, 75, ctx, "default")
    d.lr_coef, d.lr_intercept = rng.normal(size=d.lr_coef.shape) * 0.05, rng.normal(size=d.lr_intercept.shape)
    dev = DeviceModel(d)
    Xd = torch.from_numpy(rng.randint(0, 3, (Nq, C)).astype(np.int8)).cuda()
    dev.base_predict_device(Xd, f64=True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev.base_predict_device(Xd, f64=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"config": "logistic base GNX_BASE_LR_IMPL=f64 %s C=%d M=%d ctx=%d A=%d W=%d N=%d" % (name, C, M, ctx, A, C // M, Nq),
                      "inference_ms_median_of_3": round(float(np.median(ts)), 3), "inference_ms_all": [round(t, 3) for t in ts]}), flush=True)


if __name__ == "__main__":
    if which.startswith("lr_"):
        run_lr(which[3:], **GEOS[which[3:]])
        sys.exit(0)
    for k, g in GEOS.items():
        if which in ("all", k):
            run(k, **g)
