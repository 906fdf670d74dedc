#!/usr/bin/env python3
"""gnx_ancestry_score_dev at the bench's config-2 geometry (N = 10 000 haplotypes, chr22: C = 317 408 SNPs, M = 1 000, W = 317, A = 7)
with S = 1 and S = 8 scores on ONE GPU, one run: HIP events around the entry point on device-resident inputs (the checking pass, both
kernels and the verdict's read-back), median of 11 calls after a warm-up, for int8 and 2-bit rows.  Beside the time: the bytes the pass
must move (X once, labels, weights once, the partials' workspace written and read, the outputs) and the share of the measured HBM read
rate (6.29 TB/s, a float4 copy) that reading the X bytes alone in that time amounts to.

Beside it the route the library offered before: gnx_ancestry_dosage_dev once per ancestry, the uint8 matrix widened to float64 and
multiplied with the ancestry's weights by torch.matmul on the device.  That route is run on the first C_SMALL SNPs only (seven float64
matrices of the whole chromosome are 89 GB) and its time is SCALED by C / C_SMALL: labelled as scaled.
One JSON line per measurement goes to --out (profiles/score_bench.jsonl).

  python scripts/bench_score.py [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N, C, M, A = 10_000, 317_408, 1_000, 7
W = C // M
C_SMALL = 4_000
HBM_READ = 6.29e12      # bytes / s, measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from gnomix_amd import _lib, resident
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
    eff_t = torch.ones(C, dtype=torch.uint8, device="cuda")
    n_bad = ctypes.c_int64(0)
    recs = []
    with resident.torch_stream(ctx):
        for S in (1, 8):
            w = rng.normal(size=(C, A, S)) * np.exp2(rng.randint(-20, 21, size=(C, A, S)).astype(np.float64))
            w_t = torch.from_numpy(w).cuda()
            score = torch.empty((n_ind, A, S), dtype=torch.float64, device="cuda")
            cnt = [torch.empty((n_ind, A), dtype=torch.int32, device="cuda") for _ in range(3)]
            first = None
            for name, rows, kind, ld in (("int8 rows", X, _lib.GNX_ROWS_INT8, C), ("2-bit rows", P, _lib.GNX_ROWS_PACKED2, P.shape[1])):
                ms = []
                for i in range(12):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ctx.check(ctx.lib.gnx_ancestry_score_dev(ctx.h, rows.data_ptr(), kind, ld, lab_t.data_ptr(), W, N, C, M, W, A, w_t.data_ptr(), S,
                                                             eff_t.data_ptr(), score.data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr(),
                                                             0, 0, ctypes.byref(n_bad)))
                    e1.record()
                    torch.cuda.synchronize()
                    if i:
                        ms.append(e0.elapsed_time(e1))
                got = [t.cpu().numpy().copy() for t in [score] + cnt]
                if first is None:
                    first = got
                assert all(np.array_equal(u, v) for u, v in zip(first, got)), "the two row forms disagree"
                med = statistics.median(ms)
                x_bytes = N * ld
                ws_bytes = 2 * N * W * (S * 8 + 13)                                      # partials, counts and label bytes: written, then read
                moved = x_bytes + N * W * 4 + C * A * S * 8 + C + ws_bytes + n_ind * A * (S * 8 + 12)
                recs.append(dict(what="gnx_ancestry_score_dev, " + name, N=N, C=C, M=M, W=W, A=A, S=S, ms_median_of_11=round(med, 3),
                                 ms_min=round(min(ms), 3), MB_rows=round(x_bytes / 1e6, 2), MB_moved_at_least=round(moved / 1e6, 2),
                                 x_read_share_of_6p29_TBps=round(x_bytes / (med * 1e-3) / HBM_READ, 4),
                                 note="events around the entry point: the checking pass over weights and effect with its read-back, both kernels "
                                      "and the verdict's read-back; one run on one box; the weights are re-read by every tile of 256 rows (from "
                                      "L2 / MALL mostly) and counted once here; the ALT frequency is drawn as u^3 / 2 (mean 0.125)"))
            # the former route on the first C_SMALL SNPs: per ancestry the dosage matrix, widened to float64, times the weights
            Cs, Ws = C_SMALL, C_SMALL // M
            Xs, labs = X[:, :Cs].contiguous(), lab_t[:, :Ws].contiguous()
            ws_t = w_t[:Cs].contiguous()
            dos = torch.empty((n_ind, Cs), dtype=torch.uint8, device="cuda")
            ref = torch.empty((n_ind, A, S), dtype=torch.float64, device="cuda")
            ms = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for anc in range(A):
                    ctx.check(ctx.lib.gnx_ancestry_dosage_dev(ctx.h, Xs.data_ptr(), _lib.GNX_ROWS_INT8, Cs, labs.data_ptr(), Ws, N, Cs, M, Ws, A, anc,
                                                              dos.data_ptr(), Cs, None, 0))
                    ref[:, anc, :] = torch.matmul(dos.to(torch.float64), ws_t[:, anc, :])
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            ctx.check(ctx.lib.gnx_ancestry_score_dev(ctx.h, Xs.data_ptr(), _lib.GNX_ROWS_INT8, Cs, labs.data_ptr(), Ws, N, Cs, M, Ws, A, ws_t.data_ptr(), S,
                                                     eff_t.data_ptr(), score.data_ptr(), None, None, None, 0, 0, ctypes.byref(n_bad)))
            torch.cuda.synchronize()
            scale_ref = float(torch.matmul(Xs.eq(1).to(torch.float64), ws_t.abs().amax(1)).max())
            err = float((score - ref).abs().max())
            assert err <= Cs * 2.0 ** -52 * max(scale_ref, 1e-300), "the fused pass and the former route disagree: %g" % err
            scale = C / Cs
            recs.append(dict(what="former route, SCALED from the first %d SNPs by %.1f: gnx_ancestry_dosage_dev per ancestry, the matrix widened "
                                  "to float64 and torch.matmul with the weights, on the device" % (Cs, scale), S=S,
                             ms_scaled=round(statistics.median(ms) * scale, 1), ms_measured=round(statistics.median(ms), 3), measured_on_snps=Cs,
                             GB_uint8_matrices_scaled=round(A * n_ind * C / 1e9, 2), max_abs_difference_to_the_fused_pass=err))
    with open(a.out, "w") as f:      # one run = the whole file
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
