#!/usr/bin/env python3
"""gnx_ancestry_assoc_logit_dev at the bench's config-2 geometry (N = 10 000 haplotypes, chr22: C = 317 408 SNPs, M = 1 000, W = 317,
A = 7) with K = 5 covariates on ONE GPU, one run: HIP events around the entry point on device-resident inputs (prep, the verdict on
y, the null fits, the SNP fits and the verdict's read-back), median of 11 calls after a warm-up, for int8 and 2-bit rows, with the
histogram of the Newton steps per SNP and the status counts.

Baseline: the numpy restatement's arithmetic (a batched Newton iteration over the explicit designs, numpy on 16 threads) on the first
C_SMALL SNPs, its time SCALED by C / C_SMALL and labelled as scaled.  One JSON line per measurement goes to --out
(profiles/assoc_logit_bench.jsonl).  --snps limits the SNP range (a shorter run; the record says so).

  python scripts/bench_assoc_logit.py [--out FILE] [--snps C1] [--reps 11]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N, C, M, A, K = 10_000, 317_408, 1_000, 7, 5
W = C // M
C_SMALL = 2_000


def numpy_newton(D, y, keep, steps=6):
    """batched Newton steps from theta = 0 on designs D (B, n, Q) with kept columns `keep` (B, Q): the baseline's arithmetic (dense
    float64 products; no stopping rule: a fixed number of steps, about what the device takes)"""
    B, n, Q = D.shape
    D = D * keep[:, None, :]
    theta = np.zeros((B, Q))
    eye = (~keep)[:, :, None] * np.eye(Q)[None]
    for _ in range(steps):
        eta = np.einsum("bnq,bq->bn", D, theta)
        mu = 1.0 / (1.0 + np.exp(-eta))
        g = np.einsum("bnq,bn->bq", D, y[None, :] - mu)
        H = np.einsum("bnq,bn,bnr->bqr", D, mu * (1 - mu), D, optimize=True) + eye
        theta = theta + np.linalg.solve(H + 1e-12 * np.eye(Q)[None], g[:, :, None])[:, :, 0]
    return theta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_logit_bench.jsonl"))
    ap.add_argument("--snps", type=int, default=C)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    import torch
    from gnomix_amd import _lib, assoc, resident
    ctx = _lib.default_context(0)
    c1 = min(a.snps, C)
    rng = np.random.RandomState(1)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 25 + 1)), 25, axis=1)[:, :W]
    lab_t = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    maf = torch.rand((1, C), device="cuda", generator=g) ** 3 * 0.5                     # most SNPs rare, as in real panels
    X = (torch.rand((N, C), device="cuda", generator=g) < maf).to(torch.int8)
    X[torch.rand((N, C), device="cuda", generator=g) < 0.005] = 2
    x = X.to(torch.uint8)
    P = (x[:, 0::4] | (x[:, 1::4] << 2) | (x[:, 2::4] << 4) | (x[:, 3::4] << 6)).contiguous()
    del x
    n_ind = N // 2
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, K - 1))], 1)
    y = (rng.uniform(size=n_ind) < 1.0 / (1.0 + np.exp(0.3 - 0.4 * Z[:, 1]))).astype(np.float64)
    y_t, Z_t = torch.from_numpy(y).cuda(), torch.from_numpy(Z).cuda()
    bufs = assoc.logit_buffers(A, K, 0, c1, M, W, empty=lambda s, dt: torch.zeros(s, dtype=torch.float64 if dt == np.float64 else torch.int32, device="cuda"))
    sf, si, th, wf, wi = bufs
    n_bad = ctypes.c_int64(0)
    recs = []
    first = None
    with resident.torch_stream(ctx):
        for name, rows, kind, ld in (("int8 rows", X, _lib.GNX_ROWS_INT8, C), ("2-bit rows", P, _lib.GNX_ROWS_PACKED2, P.shape[1])):
            ms = []
            for i in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(ctx.lib.gnx_ancestry_assoc_logit_dev(ctx.h, rows.data_ptr(), kind, ld, lab_t.data_ptr(), W, N, C, M, W, A, y_t.data_ptr(),
                                                               Z_t.data_ptr(), K, None, 1, 0, c1, assoc.LOGIT_TOL, assoc.LOGIT_MAX_ITER, sf.data_ptr(),
                                                               si.data_ptr(), th.data_ptr(), wf.data_ptr(), wi.data_ptr(), ctypes.byref(n_bad)))
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            got = [t.cpu().numpy().copy() for t in bufs]
            if first is None:
                first = got
            assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(first, got)), "the two row forms disagree"
            fit = assoc.split_logit(*got, A, K, 0, c1, M, W)
            it, cnt = np.unique(fit.iters, return_counts=True)
            st, scnt = np.unique(fit.status, return_counts=True)
            recs.append(dict(what="gnx_ancestry_assoc_logit_dev, " + name, N=N, C=C, snps=c1, M=M, W=W, A=A, K=K,
                             ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), reps=len(ms),
                             iters_histogram={int(k): int(v) for k, v in zip(it, cnt)}, status_counts={int(k): int(v) for k, v in zip(st, scnt)},
                             status0_counts={int(k): int(v) for k, v in zip(*np.unique(fit.status0, return_counts=True))},
                             note="events around the entry point: prep, the verdict on y, null fits, SNP fits, the verdict's read-back; one run on "
                                  "one box; the ALT frequency is drawn as u^3 / 2 (most SNPs rare), so many dosage terms are dropped by the column rule"))
        # baseline: numpy on the explicit designs of the first C_SMALL SNPs
        Cs = min(C_SMALL, c1)
        Xh = X[:, :Cs].cpu().numpy()
        keep_d = ~np.isnan(first[0][:Cs, :A])
        t0 = time.perf_counter()
        for b0 in range(0, Cs, 50):
            cs = np.arange(b0, min(b0 + 50, Cs))
            lw = lab[:, cs // M]
            la, lb = lw[0::2], lw[1::2]
            xa, xb = Xh[0::2][:, cs] == 1, Xh[1::2][:, cs] == 1
            h = np.stack([(la == k).astype(np.float64) + (lb == k) for k in range(A - 1)], 2)
            d = np.stack([((la == k) & xa).astype(np.float64) + ((lb == k) & xb) for k in range(A)], 2)
            D = np.concatenate([np.broadcast_to(Z[:, None, :], (n_ind, len(cs), K)), h, d], 2).transpose(1, 0, 2)
            keep = np.concatenate([np.ones((len(cs), K + A - 1), bool), keep_d[cs]], 1)
            numpy_newton(np.ascontiguousarray(D), y, keep)
        t_np = time.perf_counter() - t0
        recs.append(dict(what="numpy baseline, SCALED from the first %d SNPs by %.1f: six dense Newton steps per SNP on the explicit designs, "
                              "OMP_NUM_THREADS=%s" % (Cs, c1 / Cs, os.environ.get("OMP_NUM_THREADS")), s_wall_scaled=round(t_np * c1 / Cs, 1),
                         s_wall_measured=round(t_np, 2), measured_on_snps=Cs))
    with open(a.out, "w") as f:      # one run = the whole file
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
