#!/usr/bin/env python3
"""gnx_ancestry_pair_counts_dev at the bench's config-2 geometry (N = 10 000 haplotypes, chr22: C = 317 408 SNPs, M = 1 000, W = 317,
A = 7), ONE ancestry, on ONE GPU, one run: HIP events around the entry point on device-resident inputs (the label count, the kernel and
the verdict's read-back), median of three calls after a warm-up, for int8 and 2-bit rows; and a few-individuals shape (N = 400) where
the SNP range is split over workgroups and the tables are combined with atomic adds.  Beside the time: the tables' bytes, the rows'
bytes and the v_mfma_i32_16x16x64_i8 instructions the kernel issues (4 waves x 2 K-steps x 16 per chunk of an off-diagonal tile pair,
12 on the diagonal).

Beside it the route the library offered before, on the same box in the same run: gnx_ancestry_dosage_dev for d, an observed-call mask
under the same labels for o (torch), both widened to float32 and multiplied by torch.matmul on the device (three products).  Float32 is
exact here: every partial sum is an integer below 4 C < 2^24.  Its tables must equal the kernel's.
One JSON line per measurement goes to --out (profiles/pairs_bench.jsonl).

  python scripts/bench_pairs.py [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

C, M, A, ANC = 317_408, 1_000, 7, 2
W = C // M
TILE, CHUNK = 64, 128


def mfma_count(n, c):
    t = (n + TILE - 1) // TILE
    chunks = (c + CHUNK - 1) // CHUNK
    return chunks * 2 * 4 * (16 * (t * (t - 1) // 2) + 12 * t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from gnomix_amd import _lib, resident
    ctx = _lib.default_context(0)
    n_bad = ctypes.c_int64(0)
    recs = []

    def timed(fn, runs=3):
        ms = []
        for i in range(runs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1))
        return ms

    with resident.torch_stream(ctx):
        for N in (10_000, 400):
            n = N // 2
            rng = np.random.RandomState(1)
            lab = np.repeat(rng.randint(0, A, size=(N, W // 25 + 1)), 25, axis=1)[:, :W]
            lab_t = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
            g = torch.Generator(device="cuda").manual_seed(1)
            maf = torch.rand((1, C), device="cuda", generator=g) ** 3 * 0.5                 # most SNPs rare, as in real panels
            X = (torch.rand((N, C), device="cuda", generator=g) < maf).to(torch.int8)
            X[torch.rand((N, C), device="cuda", generator=g) < 0.005] = 2
            x = X.to(torch.uint8)
            P = (x[:, 0::4] | (x[:, 1::4] << 2) | (x[:, 2::4] << 4) | (x[:, 3::4] << 6)).contiguous()
            del x
            tabs = [torch.empty((n, n), dtype=torch.int32, device="cuda") for _ in range(3)]
            first = None
            for name, rows, kind, ld in (("int8 rows", X, _lib.GNX_ROWS_INT8, C), ("2-bit rows", P, _lib.GNX_ROWS_PACKED2, P.shape[1])):
                def call():
                    ctx.check(ctx.lib.gnx_ancestry_pair_counts_dev(ctx.h, rows.data_ptr(), kind, ld, lab_t.data_ptr(), W, N, C, M, W, A, ANC, 0, C,
                                                                   tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), n, 0, ctypes.byref(n_bad)))
                ms = timed(call)
                got = [t.clone() for t in tabs]
                if first is None:
                    first = got
                assert all(torch.equal(u, v) for u, v in zip(first, got)), "the two row forms disagree"
                med = statistics.median(ms)
                n_mfma = mfma_count(n, C)
                recs.append(dict(what="gnx_ancestry_pair_counts_dev, " + name, N=N, individuals=n, C=C, M=M, W=W, A=A, ancestry=ANC,
                                 ms_median_of_3=round(med, 3), ms_min=round(min(ms), 3), MB_rows=round(N * ld / 1e6, 2),
                                 MB_tables=round(3 * n * n * 4 / 1e6, 2), mfma_i32_16x16x64_i8=n_mfma,
                                 int8_TOPS=round(n_mfma * 2 * 16 * 16 * 64 / (med * 1e-3) / 1e12, 2),
                                 note="events around the entry point: the label count, the kernel and the verdict's read-back; one run on one box; "
                                      "the ALT frequency is drawn as u^3 / 2 (mean 0.125)"))
            # the former route: the dosage matrix of the ancestry, an observed-call mask for o, float32 matmul on the device
            win = torch.clamp(torch.arange(C, device="cuda") // M, max=W - 1)
            dos = torch.empty((n, C), dtype=torch.uint8, device="cuda")
            ref = [None] * 3

            def former():
                ctx.check(ctx.lib.gnx_ancestry_dosage_dev(ctx.h, X.data_ptr(), _lib.GNX_ROWS_INT8, C, lab_t.data_ptr(), W, N, C, M, W, A, ANC,
                                                          dos.data_ptr(), C, None, 0))
                obs = (lab_t[:, win] == ANC) & ((X == 0) | (X == 1))
                o = (obs[0::2].to(torch.float32) + obs[1::2].to(torch.float32))
                del obs
                d = dos.to(torch.float32)
                ref[0], ref[1], ref[2] = torch.matmul(d, d.T), torch.matmul(d, o.T), torch.matmul(o, o.T)
            ms = timed(former)
            same = all(torch.equal(r.to(torch.int32), t) for r, t in zip(ref, first))
            assert same, "the kernel and the former route disagree"
            recs.append(dict(what="former route: gnx_ancestry_dosage_dev for d, an observed-call mask for o, float32 torch.matmul (3 products), on the "
                                  "device", N=N, individuals=n, C=C, ms_median_of_3=round(statistics.median(ms), 3), ms_min=round(min(ms), 3),
                             GB_float32_operands=round(2 * n * C * 4 / 1e9, 2), tables_equal_the_kernels=same))
            del X, P, dos, ref, first, tabs
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:      # one run = the whole file
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
