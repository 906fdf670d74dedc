#!/usr/bin/env python3
"""gnx_ancestry_summary_dev at chr22 geometry (N = 10 000 haplotypes, W = 317 windows, A = 7) on ONE GPU, one run:
labels only, labels with float32 probabilities, labels with float64 probabilities.  HIP events around the entry point on
device-resident inputs (the call includes the upload of the W weights, the flag's memset and the verdict's read-back), median of
11 calls after a warm-up, next to the bytes the case must move through HBM and the fraction of 8 TB/s that comes to.
One JSON line per case goes to --out (profiles/summary_bench.jsonl).

  python scripts/bench_summary.py [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N, W, A = 10_000, 317, 7
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from gnomix_amd import _lib, resident
    ctx = _lib.default_context(0)
    rng = np.random.RandomState(1)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 25 + 1)), 25, axis=1)[:, :W]
    flips = rng.rand(N, W) < 0.03
    lab[flips] = rng.randint(0, A, size=int(flips.sum()))
    lab_t = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
    p32 = torch.softmax(torch.randn((N, W, A), device="cuda"), dim=2).contiguous()
    p64 = p32.to(torch.float64)
    w = np.ascontiguousarray(rng.gamma(0.7, 0.3, size=W) + 1e-6)
    outs = [torch.empty((N, A), dtype=torch.float64, device="cuda") for _ in range(4)]
    cnt = torch.empty((N, A), dtype=torch.int32, device="cuda")
    out_bytes = N * A * (3 * 8 + 4)
    cases = {"labels only": (None, 0, N * W * 4, out_bytes),
             "labels + float32 probabilities": (p32, 0, N * W * 4 + N * W * A * 4, out_bytes + N * A * 8),
             "labels + float64 probabilities": (p64, 1, N * W * 4 + N * W * A * 8, out_bytes + N * A * 8)}
    with resident.torch_stream(ctx):
        for name, (p, f64, b_in, b_out) in cases.items():
            ms = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(ctx.lib.gnx_ancestry_summary_dev(ctx.h, lab_t.data_ptr(), W, p.data_ptr() if p is not None else None, f64, w.ctypes.data,
                                                           N, W, A, outs[0].data_ptr(), outs[1].data_ptr() if p is not None else None,
                                                           cnt.data_ptr(), outs[2].data_ptr(), outs[3].data_ptr()))
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            rec = dict(what="gnx_ancestry_summary_dev, " + name, N=N, W=W, A=A, ms_median_of_11=round(med, 4), ms_min=round(min(ms), 4),
                       MB_in=round(b_in / 1e6, 2), MB_out=round(b_out / 1e6, 3), GB_per_s=round((b_in + b_out) / med / 1e6, 1),
                       fraction_of_8TB_per_s=round((b_in + b_out) / (med * 1e-3) / HBM_BYTES_PER_S, 4),
                       note="events around the entry point: weights' upload, flag memset, kernel and the verdict's read-back; one run on one box")
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
