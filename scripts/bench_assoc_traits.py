#!/usr/bin/env python3
"""gnx_ancestry_assoc_traits_dev (D^T Y on v_mfma_f64_16x16x4_f64, k_ancestry_assoc_traits.hip) at the bench's config-2 geometry
(N = 10 000 haplotypes, chr22: C = 317 408 SNPs, M = 1 000, W = 317, A = 7) with K = 5 covariates on ONE GPU, in one process, next to
the single-trait entry it is measured against (gnx_ancestry_assoc_stats_dev) and the host finish of both.

Per ALT-frequency draw (scripts/bench_assoc.py's u^3 / 2, most SNPs rare; and 0.5 everywhere) and per T in {16, 64, 256}: HIP events
around the entry point on device-resident int8 rows (prep, window and SNP kernels and the verdict's read-back), one warm-up, median of
11 calls; the bytes of the three blocks; float64 MFMAs issued (tiles of 16 SNPs x A ancestries x T / 16 trait tiles x groups of 4
individuals) per second against F64_MFMA_PEAK_TF / 2048; the share of those MFMAs whose A operand can be non-zero at all (an individual
carries at most 2 of the A ancestries at a SNP: 2 / A, the dense-over-ancestries waste is the rest).  The single-trait entry once per
draw, the same way.  Host finish (wall clock, numpy, this box's CPU): assoc.finish of the whole chromosome, and assoc.finish_traits
chunk by chunk over the whole chromosome for T = 16 and 64 (results dropped chunk by chunk); for T = 256 on the first C_FIN_256 SNPs,
SCALED by C / C_FIN_256 and labelled so.  NOT measured: the kernels apart (the events bracket the entry), counters, the 2-bit rows
(bit-equal results, tested), the _gt2 path, the copies of the blocks to the host.  One JSON line per measurement goes to --out.

  python scripts/bench_assoc_traits.py [--out FILE]"""
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
TS = (16, 64, 256)
C_FIN_256 = 40_000
F64_MFMA_PEAK_TF = 78.6      # MI355X float64 matrix peak (vendor figure); one v_mfma_f64_16x16x4_f64 is 2 * 16 * 16 * 4 = 2048 flops
REPEATS = 11


def timed(fn):
    import torch
    ms = []
    for i in range(REPEATS + 1):                       # the first call is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_traits_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from gnomix_amd import _lib, assoc, resident
    ctx = _lib.default_context(0)
    rng = np.random.RandomState(1)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 25 + 1)), 25, axis=1)[:, :W]
    lab_t = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
    n_ind = N // 2
    y = rng.normal(size=n_ind)
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, K - 1))], 1)
    Yall = np.concatenate([y[:, None], rng.normal(size=(n_ind, max(TS) - 1))], 1)
    y_t, Z_t, zero_t = torch.from_numpy(y).cuda(), torch.from_numpy(Z).cuda(), torch.zeros(n_ind, dtype=torch.float64, device="cuda")
    NF, NI, NWF, NWI = assoc.layout(A, K)
    sf, si = torch.empty((C, NF), dtype=torch.float64, device="cuda"), torch.empty((C, NI), dtype=torch.int32, device="cuda")
    wf, wi = torch.empty((W, NWF), dtype=torch.float64, device="cuda"), torch.empty((W, NWI), dtype=torch.int32, device="cuda")
    n_bad = ctypes.c_int64(0)
    peak = F64_MFMA_PEAK_TF * 1e12 / 2048.0
    recs = []

    def emit(r):
        recs.append(r)
        print(json.dumps(r), flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    with resident.torch_stream(ctx):
        for draw in ("u^3 / 2 (most SNPs rare, mean 0.125)", "0.5 everywhere"):
            if draw.startswith("u"):
                maf = torch.rand((1, C), device="cuda", generator=g) ** 3 * 0.5
            else:
                maf = torch.full((1, C), 0.5, device="cuda")
            X = (torch.rand((N, C), device="cuda", generator=g) < maf).to(torch.int8)
            X[torch.rand((N, C), device="cuda", generator=g) < 0.005] = 2

            def single(yy=y_t):
                ctx.check(ctx.lib.gnx_ancestry_assoc_stats_dev(ctx.h, X.data_ptr(), _lib.GNX_ROWS_INT8, C, lab_t.data_ptr(), W, N, C, M, W, A,
                                                               yy.data_ptr(), Z_t.data_ptr(), K, None, 1, 0, C, sf.data_ptr(), si.data_ptr(),
                                                               wf.data_ptr(), wi.data_ptr(), ctypes.byref(n_bad)))
            med1, min1 = timed(single)
            st1 = assoc.split_blocks(*[t.cpu().numpy().copy() for t in (sf, si, wf, wi)], A, K, 0, C, M, W)
            t0 = time.perf_counter()
            res1 = assoc.finish(st1, A, K)
            fin1 = time.perf_counter() - t0
            per_trait_single = med1 / 1e3 + fin1
            emit(dict(what="single-trait path: gnx_ancestry_assoc_stats_dev (int8 rows) + assoc.finish, ONE trait", alt_freq=draw, N=N, C=C, A=A,
                             K=K, ms_device_median_of_11=round(med1, 3), ms_device_min=round(min1, 3), s_host_finish=round(fin1, 3),
                             s_per_trait=round(per_trait_single, 3), fitted_snps=int((res1[8] == 0).sum())))
            single(zero_t)                                     # the trait-independent blocks of the many-trait path: the same entry, y = 0
            st0 = assoc.split_blocks(*[t.cpu().numpy().copy() for t in (sf, si, wf, wi)], A, K, 0, C, M, W)
            for T in TS:
                ldt = assoc.trait_ldt(T)
                Y_t = torch.from_numpy(np.ascontiguousarray(Yall[:, :T])).cuda()
                sy, wy, wyy = assoc.trait_buffers(A, K, T, 0, C, M, W, empty=lambda shape, dt: torch.empty(shape, dtype=torch.float64, device="cuda"))

                def many():
                    ctx.check(ctx.lib.gnx_ancestry_assoc_traits_dev(ctx.h, X.data_ptr(), _lib.GNX_ROWS_INT8, C, lab_t.data_ptr(), W, N, C, M, W, A,
                                                                    Y_t.data_ptr(), T, T, Z_t.data_ptr(), K, None, 1, 0, C, sy.data_ptr(),
                                                                    wy.data_ptr(), wyy.data_ptr(), ctypes.byref(n_bad)))
                med, mn = timed(many)
                mfmas = ((C + 15) // 16) * A * (ldt // 16) * ((n_ind + 3) // 4)
                out_bytes = (C * A + W * (K + A - 1) + W) * ldt * 8
                rec = dict(what="gnx_ancestry_assoc_traits_dev, int8 rows", alt_freq=draw, T=T, N=N, C=C, A=A, K=K, ms_device_median_of_11=round(med, 3),
                           ms_device_min=round(mn, 3), MB_out=round(out_bytes / 1e6, 1), f64_mfmas=mfmas, mfmas_per_s=float("%.4g" % (mfmas / (med / 1e3))),
                           of_matrix_peak=round(mfmas / (med / 1e3) / peak, 4), ms_at_matrix_peak=round(mfmas / peak * 1e3, 2),
                           useful_share_of_mfmas=round(2.0 / A, 3),
                           note="events around the entry point: prep, window and SNP kernels and the verdict's read-back; one run on one box")
                if draw.startswith("u"):                       # the host finish does not depend on the draw's device time: measured once
                    Cf = C if T < 256 else C_FIN_256
                    step = assoc.traits_snps_per_chunk(A, K, T)
                    t_fin = t_copy = 0.0
                    fitted = 0
                    for c0 in range(0, Cf, step):
                        c1 = min(c0 + step, Cf)
                        t0 = time.perf_counter()
                        w0, w1 = c0 // M if c0 // M < W - 1 else W - 1, min((c1 - 1) // M, W - 1)
                        ts = assoc.split_traits(sy[c0:c1].cpu().numpy(), wy[w0:w1 + 1].cpu().numpy(), wyy[w0:w1 + 1].cpu().numpy(), T, c0, c1, M, W)
                        sub = assoc.AssocStats(st0.dtz[c0:c1], st0.dty[c0:c1], st0.dtd[c0:c1], st0.dth[c0:c1], st0.sum_d[c0:c1], st0.n_miss[c0:c1],
                                               st0.gram[w0:w1 + 1], st0.n[w0:w1 + 1], st0.sum_h[w0:w1 + 1], ts.window, 0)
                        t_copy += time.perf_counter() - t0
                        t0 = time.perf_counter()
                        out = assoc.finish_traits(sub, ts, A, K)
                        t_fin += time.perf_counter() - t0
                        fitted += int((out[8] == 0).sum())
                    scale = C / Cf
                    rec.update(s_host_finish=round(t_fin * scale, 3), s_block_copies_to_host=round(t_copy * scale, 3), host_finish_measured_on_snps=Cf,
                               host_finish_scaled_by=round(scale, 3), fitted_snps_in_those=fitted,
                               s_per_trait=round((med / 1e3 + med1 / 1e3 + t_fin * scale) / T, 4), s_per_trait_single_path=round(per_trait_single, 3),
                               per_trait_note="(trait kernels + the one single-trait call for the trait-independent blocks + finish_traits) / T")
                emit(rec)
                del sy, wy, wyy, Y_t
            del X
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:      # one run = the whole file
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
