#!/usr/bin/env python3
"""Times gnx_ancestry_admixmap_dev at chr1 geometry -> profiles/admixmap_bench.jsonl (one JSON line per configuration).

W = 1431 windows, 50 000 haplotypes, A in {7, 12}, K = 5, T in {1, 64, 1024}; random labels, Y and Z resident in HBM.  HIP events around
the entry (prep, Gram and main kernels and the read-back of the label counter), one warm-up, the median of 11.  mfma_share: the main
kernel's v_mfma_f64_16x16x4_f64 count per second (W * ceil(n / 4) * ceil((K + A) / 16) * ldt / 16, each 2048 flop) as a share of the
float64 matrix peak F64_MFMA_PEAK_TF.  s_host_finish: admixmap.finish (factor, solve, p-values) of the call's blocks on the host, once.
Then, in the same run, at T = 64 on chr22 geometry (10 000 haplotypes, C = 317 408, M = 1 000, W = 317, A = 7, K = 5): the existing route
to the same window blocks (gnx_ancestry_assoc_stats_dev with a zero phenotype plus gnx_ancestry_assoc_traits_dev, int8 X resident in
HBM, all SNP blocks walked and written) against gnx_ancestry_admixmap_dev on the same labels, Y and Z."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F64_MFMA_PEAK_TF = 78.6     # MI355X float64 matrix peak, TFLOP/s
W, N, K = 1431, 50000, 5


def timed(fn):
    import torch
    ms = []
    for it in range(12):                                  # the first call is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def existing_route(ctx, rng):
    """chr22 geometry, T = 64: the window blocks by the existing entries and by the new one"""
    import numpy as np
    import torch
    from gnomix_amd import _lib, admixmap, assoc
    N2, C, M, W2, A, T = 10000, 317408, 1000, 317, 7, 64
    n = N2 // 2
    lab = torch.from_numpy(rng.randint(0, A, size=(N2, W2)).astype(np.int32)).cuda()
    Z = torch.from_numpy(np.concatenate([np.ones((n, 1)), rng.normal(size=(n, K - 1))], 1)).cuda()
    Y = torch.from_numpy(rng.normal(size=(n, T))).cuda()
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    X = (torch.rand((N2, C), device="cuda", generator=g) < 0.3).to(torch.int8)
    new = lambda shape, dt: torch.empty(shape, dtype={np.int32: torch.int32, np.float64: torch.float64}[dt], device="cuda")
    sb = assoc.stats_buffers(A, K, 0, C, M, W2, empty=new)
    tb = assoc.trait_buffers(A, K, T, 0, C, M, W2, empty=new)
    ab = admixmap.stats_buffers(A, K, T, 0, W2, empty=new)
    n_bad = ctypes.c_int64(0)

    def stats():
        ctx.check(ctx.lib.gnx_ancestry_assoc_stats_dev(ctx.h, X.data_ptr(), _lib.GNX_ROWS_INT8, C, lab.data_ptr(), W2, N2, C, M, W2, A, zero.data_ptr(),
                                                       Z.data_ptr(), K, None, 1, 0, C, *(b.data_ptr() for b in sb), ctypes.byref(n_bad)))

    def traits():
        ctx.check(ctx.lib.gnx_ancestry_assoc_traits_dev(ctx.h, X.data_ptr(), _lib.GNX_ROWS_INT8, C, lab.data_ptr(), W2, N2, C, M, W2, A, Y.data_ptr(), T, T,
                                                        Z.data_ptr(), K, None, 1, 0, C, *(b.data_ptr() for b in tb), ctypes.byref(n_bad)))

    def admix():
        ctx.check(ctx.lib.gnx_ancestry_admixmap_dev(ctx.h, lab.data_ptr(), W2, N2, W2, A, Y.data_ptr(), T, T, Z.data_ptr(), K, None, 0, W2,
                                                    *(b.data_ptr() for b in ab), ctypes.byref(n_bad)))
    out = []
    for what, fn, nbytes in (("existing route 1/2: gnx_ancestry_assoc_stats_dev, zero phenotype", stats, sum(b.numel() * b.element_size() for b in sb)),
                             ("existing route 2/2: gnx_ancestry_assoc_traits_dev", traits, sum(b.numel() * b.element_size() for b in tb)),
                             ("gnx_ancestry_admixmap_dev on the same labels, Y and Z", admix, sum(b.numel() * b.element_size() for b in ab))):
        med, lo, hi = timed(fn)
        out.append({"what": what, "N": N2, "C": C, "M": M, "W": W2, "A": A, "K": K, "T": T, "ms_median": round(med, 3), "ms_min": round(lo, 3),
                    "ms_max": round(hi, 3), "MB_out": round(nbytes / 1e6, 1), "runs": 11})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    import numpy as np
    import torch
    from gnomix_amd import _lib, admixmap
    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream(0).cuda_stream)
    rng = np.random.RandomState(0)
    out_path = os.path.join(ROOT, "profiles", "admixmap_bench.jsonl")
    lines = []
    for A in (7, 12):
        lab = torch.from_numpy(rng.randint(0, A, size=(N, W)).astype(np.int32)).cuda()
        Z = torch.from_numpy(np.concatenate([np.ones((N // 2, 1)), rng.normal(size=(N // 2, K - 1))], 1)).cuda()
        for T in (1, 64, 1024):
            Y = torch.from_numpy(rng.normal(size=(N // 2, T))).cuda()
            bufs = admixmap.stats_buffers(A, K, T, 0, W, empty=lambda shape, dt: torch.empty(shape, dtype={np.int32: torch.int32, np.float64: torch.float64}[dt], device="cuda"))
            n_bad = ctypes.c_int64(0)
            ms = []
            for it in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(ctx.lib.gnx_ancestry_admixmap_dev(ctx.h, lab.data_ptr(), W, N, W, A, Y.data_ptr(), T, T, Z.data_ptr(), K, None, 0, W,
                                                            *(b.data_ptr() for b in bufs), ctypes.byref(n_bad)))
                e1.record()
                e1.synchronize()
                if it:
                    ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            ldt = (T + 15) // 16 * 16
            mfma = W * ((N // 2 + 3) // 4) * ((K + A + 15) // 16) * (ldt // 16)
            st = admixmap.split_blocks(*(b.cpu().numpy() for b in bufs), A, K, T)
            t0 = time.perf_counter()
            res = admixmap.finish(st, K)
            fin = time.perf_counter() - t0
            lines.append({"what": "gnx_ancestry_admixmap_dev", "s_host_finish": round(fin, 3), "fitted_windows": int((res.status == 0).sum()), "W": W, "N": N, "A": A, "K": K, "T": T, "ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                          "mfma_per_s": mfma / (med * 1e-3), "mfma_share": mfma / (med * 1e-3) / (F64_MFMA_PEAK_TF * 1e12 / 2048), "runs": len(ms)})
            print(json.dumps(lines[-1]), flush=True)
    lines += existing_route(ctx, rng)
    with open(out_path, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
