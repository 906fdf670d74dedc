#!/usr/bin/env python3
"""The LDA base (LDABase) on ONE GPU at chr22's geometry with windows of 2 336 SNPs (C = 370 379, M = 1 168, context 584, W = 317,
A = 7): 4 000 fit haplotypes, 10 000 query haplotypes, everything resident in HBM.  Prints one JSON line per mode.

  python scripts/bench_lda.py gram [windows_per_call]   the Gram pass of the fit (gnx_train_lda_gram_dev over all windows, a range at a
                                                        time into one reused output buffer): one warm-up sweep, then the median of
                                                        three; int8 multiply-adds per second counted as N * width^2 per window
  python scripts/bench_lda.py finish [n_windows]        the host finish (train.lda_finish: one eigen-decomposition of size width per
                                                        window) of n_windows windows over the allowed host threads; the figure for
                                                        all W windows is that time multiplied out — an EXTRAPOLATION, labelled so
  python scripts/bench_lda.py infer                     the inference pass (k_lda_softmax), random coefficients: one warm-up, median of five
  python scripts/bench_lda.py lr                        the same geometry through the float64-MFMA logistic pass (k_base_logistic,
                                                        GNX_BASE_LR_IMPL=f64, set here): the same arithmetic volume, the yardstick"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

mode = sys.argv[1] if len(sys.argv) > 1 else "infer"
if mode == "lr":
    os.environ["GNX_BASE_LR_IMPL"] = "f64"   # read when the context is made

from gnomix_amd import DeviceModel, _lib, train

C, M, CTX, A, N_FIT, N_Q = 317 * 1168 + 123, 1168, 584, 7, 4000, 10000
W, LDW = C // M, M + 2 * CTX + C - M * (C // M)
GEO = "C=%d M=%d ctx=%d A=%d W=%d width=%d" % (C, M, CTX, A, W, M + 2 * CTX)


def fit_data(n, rng):
    y = rng.randint(0, A, (n, W)).astype(np.int32)
    y[:A] = np.arange(A)[:, None]
    X = np.empty((n, C), np.int8)
    for r0 in range(0, n, 250):   # (in slices: the float64 draws of the whole matrix would be 12 GB)
        u = rng.random_sample((min(250, n - r0), C))
        X[r0:r0 + 250] = np.where(u < 0.02, 2, u < 0.42)
    return X, y


def median_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def run_gram(per_call):
    import torch
    rng = np.random.RandomState(3)
    X, y = fit_data(N_FIT, rng)
    ctx = _lib.default_context(0)
    dX, dy = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    G = torch.empty((per_call, LDW, LDW), dtype=torch.int32, device="cuda")
    S = torch.empty((per_call, A, LDW), dtype=torch.int32, device="cuda")
    n = torch.empty((per_call, A), dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)

    def sweep():
        for w0 in range(0, W, per_call):
            ctx.check(ctx.lib.gnx_train_lda_gram_dev(ctx.h, dX.data_ptr(), N_FIT, C, dy.data_ptr(), C, M, CTX, A, w0, min(W, w0 + per_call),
                                                     G.data_ptr(), S.data_ptr(), n.data_ptr()))

    ms, all_ms = median_ms(sweep, 3)
    macs = float(N_FIT) * sum(float(M + 2 * CTX + (C - M * W if w == W - 1 else 0)) ** 2 for w in range(W))
    print(json.dumps({"config": "LDA Gram pass " + GEO + " n_fit=%d windows_per_call=%d" % (N_FIT, per_call), "gram_ms_median_of_3": round(ms, 3),
                      "gram_ms_all": all_ms, "int8_macs_counted_full_square": macs, "int8_macs_per_s": macs / (ms / 1e3),
                      "note": "the kernel computes the tiles on or below the diagonal only (about half the counted products); the output "
                              "buffer's memset is inside the time"}), flush=True)


def run_finish(k):
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.RandomState(3)
    X, y = fit_data(N_FIT, rng)
    k = min(k, W)
    t0 = time.perf_counter()
    G, S, n = train.lda_gram(X, y, M, CTX, A, 0, k)
    gram_s = time.perf_counter() - t0
    workers = min(train.host_threads(), k)
    width = M + 2 * CTX
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=workers) as pool:
        ranks = list(pool.map(lambda w: train.lda_finish(G[w, :width, :width], S[w, :, :width], n[w], N_FIT)[2]["rank"], range(k)))
    fin_s = time.perf_counter() - t0
    print(json.dumps({"config": "LDA host finish " + GEO + " n_fit=%d" % N_FIT, "windows_finished": k, "host_threads": workers,
                      "finish_s": round(fin_s, 2), "finish_s_all_windows_EXTRAPOLATED": round(fin_s * W / k, 1),
                      "gram_host_form_s_for_these_windows_with_staging": round(gram_s, 2), "ranks_min_max": [int(min(ranks)), int(max(ranks))]}),
          flush=True)


def run_infer(lr):
    import torch
    rng = np.random.RandomState(3)
    d = train.untrained_model(C, M, A, 75, CTX, "default", base=None if lr else "lda_svd")
    if lr:
        d.lr_coef, d.lr_intercept = rng.normal(size=d.lr_coef.shape) * 0.05, rng.normal(size=d.lr_intercept.shape)
    else:
        d.lda_coef, d.lda_intercept = rng.normal(size=d.lda_coef.shape) * 0.05, rng.normal(size=d.lda_intercept.shape)
        d.lda_coef[:-1, :, M + 2 * CTX:] = 0.0
    dev = DeviceModel(d)
    Xd = torch.from_numpy(rng.randint(0, 3, (N_Q, C), dtype=np.int8)).cuda()
    ms, all_ms = median_ms(lambda: dev.base_predict_device(Xd, f64=True), 5)
    name = "logistic base GNX_BASE_LR_IMPL=f64 (k_base_logistic)" if lr else "LDA base (k_lda_softmax)"
    print(json.dumps({"config": name + " " + GEO + " N=%d" % N_Q, "inference_ms_median_of_5": round(ms, 3), "inference_ms_all": all_ms,
                      "haplotypes_per_s": N_Q / (ms / 1e3)}), flush=True)


if __name__ == "__main__":
    if mode == "gram":
        run_gram(int(sys.argv[2]) if len(sys.argv) > 2 else 16)
    elif mode == "finish":
        run_finish(int(sys.argv[2]) if len(sys.argv) > 2 else 16)
    elif mode in ("infer", "lr"):
        run_infer(mode == "lr")
    else:
        sys.exit(__doc__)
