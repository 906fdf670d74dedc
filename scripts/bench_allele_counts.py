#!/usr/bin/env python3
"""gnx_ancestry_allele_counts_dev at the bench's config-2 geometry (N = 10 000 haplotypes, chr22: C = 317 408 SNPs, M = 1 000, W = 317,
A = 7) on ONE GPU, one run: int8 rows and 2-bit rows.  HIP events around the entry point on device-resident inputs (the call includes
the three tables' memsets, the flag's memset and the verdict's read-back), median of 11 calls after a warm-up, next to the algorithmic
bytes  N * ld_rows + 4 * N * W + 12 * A * C  and the fraction of 8 TB/s they come to.
One JSON line per row form goes to --out (profiles/allele_counts_bench.jsonl).

  python scripts/bench_allele_counts.py [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N, C, M, A = 10_000, 317_408, 1_000, 7
W = C // M
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "allele_counts_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from gnomix_amd import _lib, resident
    ctx = _lib.default_context(0)
    rng = np.random.RandomState(1)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 25 + 1)), 25, axis=1)[:, :W]
    lab_t = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    maf = torch.rand((1, C), device="cuda", generator=g) ** 3 * 0.5                     # most SNPs rare, as in real panels
    u = torch.rand((N, C), device="cuda", generator=g)
    X = (u < maf).to(torch.int8)
    X[torch.rand((N, C), device="cuda", generator=g) < 0.005] = 2
    del u
    ldp = (C + 3) // 4
    x = X.to(torch.uint8)
    P = (x[:, 0::4] | (x[:, 1::4] << 2) | (x[:, 2::4] << 4) | (x[:, 3::4] << 6)).contiguous()
    del x
    tabs = [torch.empty((A, C), dtype=torch.int32, device="cuda") for _ in range(3)]
    cases = {"int8 rows": (X, _lib.GNX_ROWS_INT8, C), "2-bit rows": (P, _lib.GNX_ROWS_PACKED2, ldp)}
    first = None
    with resident.torch_stream(ctx):
        for name, (rows, kind, ld) in cases.items():
            ms = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(ctx.lib.gnx_ancestry_allele_counts_dev(ctx.h, rows.data_ptr(), kind, ld, lab_t.data_ptr(), W, N, C, M, W, A,
                                                                 tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), 0, 0))
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            got = [t.cpu().numpy().copy() for t in tabs]
            if first is None:
                first = got
            assert all(np.array_equal(x_, y_) for x_, y_ in zip(first, got)), "the two row forms disagree"
            assert int((got[0] + got[2]).sum()) == N * C
            med = statistics.median(ms)
            b = N * ld + 4 * N * W + 12 * A * C
            rec = dict(what="gnx_ancestry_allele_counts_dev, " + name, N=N, C=C, M=M, W=W, A=A, ms_median_of_11=round(med, 4), ms_min=round(min(ms), 4),
                       MB_algorithmic=round(b / 1e6, 2), GB_per_s=round(b / med / 1e6, 1),
                       fraction_of_8TB_per_s=round(b / (med * 1e-3) / HBM_BYTES_PER_S, 4),
                       note="events around the entry point: table memsets, flag memset, kernel and the verdict's read-back; one run on one box")
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
