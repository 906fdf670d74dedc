#!/usr/bin/env python3
"""gnx_ancestry_assoc_stats_dev at the bench's config-2 geometry (N = 10 000 haplotypes, chr22: C = 317 408 SNPs, M = 1 000, W = 317,
A = 7) with K = 5 covariates on ONE GPU, one run: HIP events around the entry point on device-resident inputs (prep, window and SNP
kernels and the verdict's read-back), median of 11 calls after a warm-up, for int8 and 2-bit rows, next to the bytes that leave HBM's
side of the analysis (the blocks) and the host finish of the whole chromosome (gnomix_amd/assoc.py, wall clock).

Beside it the route the library offered before: gnx_ancestry_dosage_dev once per ancestry (two (N / 2, C) uint8 matrices each), the
matrices copied to the host, and the same blocks and finish computed there with numpy.  That route is run on the first C_SMALL SNPs only
(the matrices of the whole chromosome do not fit a sensible host budget) and its times are SCALED by C / C_SMALL: labelled as scaled.
One JSON line per measurement goes to --out (profiles/assoc_bench.jsonl).

  python scripts/bench_assoc.py [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N, C, M, A, K = 10_000, 317_408, 1_000, 7, 5
W = C // M
C_SMALL = 4_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from gnomix_amd import _lib, assoc, resident
    ctx = _lib.default_context(0)
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
    y = rng.normal(size=n_ind)
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, K - 1))], 1)
    y_t, Z_t = torch.from_numpy(y).cuda(), torch.from_numpy(Z).cuda()
    NF, NI, NWF, NWI = assoc.layout(A, K)
    sf, si = torch.empty((C, NF), dtype=torch.float64, device="cuda"), torch.empty((C, NI), dtype=torch.int32, device="cuda")
    wf, wi = torch.empty((W, NWF), dtype=torch.float64, device="cuda"), torch.empty((W, NWI), dtype=torch.int32, device="cuda")
    out_bytes = C * (NF * 8 + NI * 4) + W * (NWF * 8 + NWI * 4)
    n_bad = ctypes.c_int64(0)
    recs = []
    first = None
    with resident.torch_stream(ctx):
        for name, rows, kind, ld in (("int8 rows", X, _lib.GNX_ROWS_INT8, C), ("2-bit rows", P, _lib.GNX_ROWS_PACKED2, P.shape[1])):
            ms = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(ctx.lib.gnx_ancestry_assoc_stats_dev(ctx.h, rows.data_ptr(), kind, ld, lab_t.data_ptr(), W, N, C, M, W, A, y_t.data_ptr(),
                                                               Z_t.data_ptr(), K, None, 1, 0, C, sf.data_ptr(), si.data_ptr(), wf.data_ptr(),
                                                               wi.data_ptr(), ctypes.byref(n_bad)))
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            got = [t.cpu().numpy().copy() for t in (sf, si, wf, wi)]
            if first is None:
                first = got
            assert all(np.array_equal(u, v) for u, v in zip(first, got)), "the two row forms disagree"
            recs.append(dict(what="gnx_ancestry_assoc_stats_dev, " + name, N=N, C=C, M=M, W=W, A=A, K=K, ms_median_of_11=round(statistics.median(ms), 3),
                             ms_min=round(min(ms), 3), MB_out=round(out_bytes / 1e6, 2), MB_rows=round(N * ld / 1e6, 2),
                             note="events around the entry point: prep, window and SNP kernels and the verdict's read-back; one run on one box; "
                                  "the ALT frequency is drawn as u^3 / 2 (most SNPs rare, mean 0.125): most (individual, SNP) cells take the early "
                                  "exit and the figure says little about SNPs where ALT is common"))
        t0 = time.perf_counter()
        st = assoc.split_blocks(*first, A, K, 0, C, M, W)
        res = assoc.finish(st, A, K)
        t_fin = time.perf_counter() - t0
        recs.append(dict(what="host finish of the whole chromosome (gnomix_amd.assoc.finish, numpy)", C=C, A=A, K=K, s_wall=round(t_fin, 3),
                         fitted_snps=int((res[8] == 0).sum())))
        # the former route on the first C_SMALL SNPs: the dosage matrices of every ancestry, materialised, copied out, reduced on the host
        Cs, Ws = C_SMALL, C_SMALL // M
        Xs, labs = X[:, :Cs].contiguous(), lab_t[:, :Ws].contiguous()
        dos = [torch.empty((n_ind, Cs), dtype=torch.uint8, device="cuda") for _ in range(2 * A)]
        ms = []
        for i in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for anc in range(A):
                ctx.check(ctx.lib.gnx_ancestry_dosage_dev(ctx.h, Xs.data_ptr(), _lib.GNX_ROWS_INT8, Cs, labs.data_ptr(), Ws, N, Cs, M, Ws, A, anc,
                                                          dos[2 * anc].data_ptr(), Cs, dos[2 * anc + 1].data_ptr(), Cs))
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        host = [t.cpu().numpy() for t in dos]
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        zy = np.concatenate([Z, y[:, None]], 1)
        blocks_f = np.zeros((Cs, A, K + 1))
        blocks_dd, blocks_dh = np.zeros((Cs, A, A)), np.zeros((Cs, A, A - 1))
        for c0 in range(0, Cs, 500):
            D = np.stack([host[2 * anc][:, c0:c0 + 500] for anc in range(A)], 2).astype(np.float64).transpose(1, 2, 0)   # (c, A, n)
            H = np.stack([host[2 * anc + 1][:, c0:c0 + 500] for anc in range(A - 1)], 2).astype(np.float64).transpose(1, 0, 2)
            blocks_f[c0:c0 + 500] = D @ zy
            blocks_dd[c0:c0 + 500] = D @ D.transpose(0, 2, 1)
            blocks_dh[c0:c0 + 500] = D @ H
        t_host = time.perf_counter() - t0
        assert np.array_equal(blocks_dd[:, 0, 0], first[1][:Cs, 0])
        scale = C / Cs
        recs.append(dict(what="former route, SCALED from the first %d SNPs by %.1f: gnx_ancestry_dosage_dev per ancestry, copy to the host, blocks "
                              "with numpy (the finish after it is the same)" % (Cs, scale), ms_device_scaled=round(statistics.median(ms) * scale, 1),
                         s_copy_scaled=round(t_copy * scale, 1), s_host_blocks_scaled=round(t_host * scale, 1),
                         GB_matrices_scaled=round(2 * A * n_ind * C / 1e9, 2), measured_on_snps=Cs))
    with open(a.out, "w") as f:      # one run = the whole file
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
