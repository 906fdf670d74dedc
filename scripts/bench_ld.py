#!/usr/bin/env python3
"""gnx_ancestry_ld_counts_dev at the bench's config-2 geometry (chr22: C = 317 408 SNPs, M = 1 000, W = 317, A = 7), ONE ancestry, band 256,
for N = 10 000 and N = 400 haplotypes, on ONE GPU, one run: HIP events around the entry point on device-resident inputs (the label
count, the kernel and the verdict's read-back), median of three calls after a warm-up, for int8 and 2-bit rows.  Beside the time: the
tables' bytes, the rows' bytes and the v_mfma_i32_16x16x64_i8 instructions the kernel issues (4 waves x 2 K-steps x 16 per chunk of 128
haplotypes and tile pair).

Beside it the route the library offered before, on the same box in the same run: the masks o and d built in torch from the labels and X
(what gnx_ancestry_dosage_dev's inputs give per haplotype), widened to float32, and a block-banded torch.matmul: per block of 2 048 SNPs
four products (block)^T x (block + band), from which the band is gathered.  Float32 is exact here: every sum is an integer <= N < 2^24.
Its tables must equal the kernel's.  One JSON line per measurement goes to --out (profiles/ld_bench.jsonl).

  python scripts/bench_ld.py [--out FILE] [--snps K]      (--snps: the range [0, K) instead of the whole chromosome)"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

C, M, A, ANC, BAND = 317_408, 1_000, 7, 2, 256
W = C // M
TILE, CHUNK, BLOCK = 64, 128, 2048


def mfma_count(N, c1, band):
    nI, nJ, nT = (c1 + TILE - 1) // TILE, (band + 62) // TILE + 1, (C + TILE - 1) // TILE
    pairs = sum(min(nJ, nT - bi) for bi in range(nI))
    return pairs * ((N + CHUNK - 1) // CHUNK) * 4 * 2 * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ld_bench.jsonl"))
    ap.add_argument("--snps", type=int, default=C)
    a = ap.parse_args()
    c1 = min(a.snps, C)
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
            tabs = [torch.empty((c1, BAND), dtype=torch.int32, device="cuda") for _ in range(4)]
            first = None
            for name, rows, kind, ld in (("int8 rows", X, _lib.GNX_ROWS_INT8, C), ("2-bit rows", P, _lib.GNX_ROWS_PACKED2, P.shape[1])):
                def call():
                    ctx.check(ctx.lib.gnx_ancestry_ld_counts_dev(ctx.h, rows.data_ptr(), kind, ld, lab_t.data_ptr(), W, N, C, M, W, A, ANC, 0, c1, BAND,
                                                                 tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(), BAND, 0,
                                                                 ctypes.byref(n_bad)))
                ms = timed(call)
                got = [t.clone() for t in tabs]
                if first is None:
                    first = got
                assert all(torch.equal(u, v) for u, v in zip(first, got)), "the two row forms disagree"
                med = statistics.median(ms)
                n_mfma = mfma_count(N, c1, BAND)
                recs.append(dict(what="gnx_ancestry_ld_counts_dev, " + name, N=N, C=C, c0=0, c1=c1, band=BAND, M=M, W=W, A=A, ancestry=ANC,
                                 ms_median_of_3=round(med, 3), ms_min=round(min(ms), 3), MB_rows=round(N * ld / 1e6, 2),
                                 MB_tables=round(4 * c1 * BAND * 4 / 1e6, 2), mfma_i32_16x16x64_i8=n_mfma,
                                 int8_TOPS=round(n_mfma * 2 * 16 * 16 * 64 / (med * 1e-3) / 1e12, 2),
                                 note="events around the entry point: the label count, the kernel and the verdict's read-back; one run on one box; "
                                      "the ALT frequency is drawn as u^3 / 2 (mean 0.125)"))
            # the former route: o and d in torch, float32, block-banded matmul, the band gathered
            win = torch.clamp(torch.arange(C, device="cuda") // M, max=W - 1)
            ref = [torch.zeros((c1, BAND), dtype=torch.int32, device="cuda") for _ in range(4)]
            kk = torch.arange(BAND, device="cuda")[None, :]

            def former():
                for b0 in range(0, c1, BLOCK):
                    b1, e1 = min(b0 + BLOCK, c1), min(b0 + BLOCK + BAND - 1, C)
                    Xb = X[:, b0:e1]
                    ob = (lab_t[:, win[b0:e1]] == ANC) & ((Xb == 0) | (Xb == 1))
                    o = ob.to(torch.float32)
                    d = (ob & (Xb == 1)).to(torch.float32)
                    rows_ = torch.arange(b1 - b0, device="cuda")[:, None]
                    col = rows_ + kk
                    ok = col < e1 - b0
                    col = torch.where(ok, col, torch.zeros_like(col))
                    for q, (u, v) in enumerate(((d, d), (d, o), (o, d), (o, o))):
                        full = torch.matmul(u[:, :b1 - b0].T, v)
                        ref[q][b0:b1] = torch.where(ok, torch.gather(full, 1, col), torch.zeros_like(full[:, :BAND])).to(torch.int32)
            ms = timed(former)
            same = all(torch.equal(r, t) for r, t in zip(ref, first))
            assert same, "the kernel and the former route disagree"
            recs.append(dict(what="former route: o and d masks in torch, float32, block-banded torch.matmul (4 products per block of %d SNPs), "
                                  "the band gathered, on the device" % BLOCK, N=N, C=C, c1=c1, band=BAND,
                             ms_median_of_3=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), tables_equal_the_kernels=same))
            del X, P, ref, first, tabs
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:      # one run = the whole file
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
