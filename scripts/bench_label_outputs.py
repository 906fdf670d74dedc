#!/usr/bin/env python3
"""The label outputs at chr22 geometry (W = 317 windows, C = 370 500 query SNPs) on ONE GPU and its host, one run:

  kernels   k_mode_filter (size 5) and k_label_runs at N = 10 000 haplotypes: HIP events around gnx_mode_filter_dev / gnx_label_runs_dev
            on device-resident labels, median of 11 calls after a warm-up (each call includes its 4- or 8-byte verdict read-back)
  writers   write_msp, write_lai and write_bed at N = 2 000 haplotypes into tmpfs, best and median of 3, with output bytes per second
  bed_ref   postprocess.msp_to_bed (the unchanged yardstick) on the same .msp, once
  lai_ref   postprocess.msp_to_lai on the same .msp, once, under --lai-timeout seconds (600 by default); when it does not finish,
            the comparison is repeated at N = 200 (write_lai and msp_to_lai both) and the record says so

Every step is a child process of its own under its own time limit; the first step that fails, faults or runs out of time ends the
run.  One JSON line per figure goes to --out (profiles/label_outputs_bench.jsonl).

  python scripts/bench_label_outputs.py [--out FILE] [--tmp DIR] [--lai-timeout S] [--steps kernels,writers,bed_ref,lai_ref]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

W, C_SNPS, A = 317, 370_500, 7
N_KERNEL, N_WRITE, N_SMALL = 10_000, 2_000, 200
LIMITS = {"kernels": 120, "writers": 240, "bed_ref": 600, "lai_small": 600}


def labels(N, seed=1):
    """ancestry tracts of a few dozen windows with single-window flips: what the smoother's argmax looks like"""
    rng = np.random.RandomState(seed)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 25 + 1)), 25, axis=1)[:, :W]
    flips = rng.rand(N, W) < 0.03
    lab[flips] = rng.randint(0, A, size=int(flips.sum()))
    return np.ascontiguousarray(lab, dtype=np.int32)


def query(N):
    from gnomix_amd import postprocess as pp
    pos = 16_000_000 + 95 * np.arange(C_SNPS)
    M = C_SNPS // W
    meta = pp.get_meta_data("22", pos, pos, W, M, np.array([16_000_000, 51_300_000]), np.array([0.0, 74.1]))
    return meta, pos, ["S%05d" % i for i in range(N // 2)], ["P%d" % a for a in range(A)]


def emit(out, **rec):
    rec["geometry"] = "chr22: W = %d, C = %d, A = %d" % (W, C_SNPS, A)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def step_kernels(a):
    import ctypes
    import torch
    from gnomix_amd import _lib, resident
    ctx = _lib.default_context(0)
    lab = torch.from_numpy(labels(N_KERNEL)).cuda()
    out = torch.empty_like(lab)
    counts = torch.empty(N_KERNEL, dtype=torch.int64, device="cuda")
    off = torch.empty(N_KERNEL + 1, dtype=torch.int64, device="cuda")
    tr = torch.empty((N_KERNEL * W, 3), dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(0)
    calls = {"k_mode_filter size 5": lambda: ctx.lib.gnx_mode_filter_dev(ctx.h, lab.data_ptr(), W, out.data_ptr(), W, N_KERNEL, W, A, 5),
             "k_label_runs (count, scan, fill)": lambda: ctx.lib.gnx_label_runs_dev(ctx.h, lab.data_ptr(), W, N_KERNEL, W, counts.data_ptr(),
                                                                                    off.data_ptr(), tr.data_ptr(), N_KERNEL * W,
                                                                                    ctypes.byref(total))}
    with resident.torch_stream(ctx):
        for name, call in calls.items():
            ms = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(call())
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            emit(a.out, step="kernels", what=name, N=N_KERNEL, ms_median_of_11=round(statistics.median(ms), 4), ms_min=round(min(ms), 4),
                 labels_MB=round(N_KERNEL * W * 4 / 1e6, 2), runs=int(total.value) if "runs" in name else None,
                 note="events around the entry point: kernel(s), flag memset and the verdict's read-back")


def _timed(fn, n=3):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def _write_all(a, N, what):
    from gnomix_amd import _lib, postprocess as pp
    meta, pos, samples, pops = query(N)
    lab = labels(N)
    prefix = os.path.join(a.tmp, "q%d" % N)
    if "msp" in what:
        ts = _timed(lambda: pp.write_msp(prefix, meta, lab, pops, samples))
        emit(a.out, step="writers", what="write_msp", N=N, s_best=round(min(ts), 4), s_median=round(statistics.median(ts), 4),
             bytes=os.path.getsize(prefix + ".msp"))
    if "lai" in what:
        def lai():
            if os.path.exists(prefix + ".lai"):
                os.remove(prefix + ".lai")      # a FRESH file every time: that is what the page-cache ceiling was measured on
            pp.write_lai(prefix, meta, lab, pos, samples, populations=pops)
        ts = _timed(lai)
        b = os.path.getsize(prefix + ".lai")
        emit(a.out, step="writers", what="write_lai", N=N, s_best=round(min(ts), 4), s_median=round(statistics.median(ts), 4), bytes=b,
             GB_per_s_best=round(b / min(ts) / 1e9, 3), page_cache_ceiling_GB_per_s="5.4-5.9 (305 MB in 0.052-0.056 s, postprocess.write_fb)")
    if "bed" in what:
        ctx = _lib.default_context(0)
        bed = prefix + "_bed"

        def run_bed():
            shutil.rmtree(bed, ignore_errors=True)
            pp.write_bed(bed, meta, lab, samples, pop_order=pops, ctx=ctx)
        ts = _timed(run_bed)
        b = _dir_bytes(bed)
        emit(a.out, step="writers", what="write_bed", N=N, files=N, s_best=round(min(ts), 4), s_median=round(statistics.median(ts), 4), bytes=b,
             MB_per_s_best=round(b / min(ts) / 1e6, 2), files_per_s_best=round(N / min(ts), 1))


def step_writers(a):
    _write_all(a, N_WRITE, ("msp", "lai", "bed"))


def step_bed_ref(a):
    from gnomix_amd import postprocess as pp
    _, _, _, pops = query(2)
    prefix = os.path.join(a.tmp, "q%d" % N_WRITE)
    t0 = time.perf_counter()
    pp.msp_to_bed(prefix + ".msp", prefix + "_bed_ref", pop_order=pops)
    t = time.perf_counter() - t0
    same = all(open(os.path.join(prefix + "_bed_ref", f), "rb").read() == open(os.path.join(prefix + "_bed", f), "rb").read()
               for f in os.listdir(prefix + "_bed_ref"))
    emit(a.out, step="bed_ref", what="msp_to_bed", N=N_WRITE, s=round(t, 3), bytes=_dir_bytes(prefix + "_bed_ref"), same_bytes_as_write_bed=same)


def _lai_ref(a, N):
    from gnomix_amd import postprocess as pp
    _, pos, _, _ = query(2)
    prefix = os.path.join(a.tmp, "q%d" % N)
    t0 = time.perf_counter()
    pp.msp_to_lai(prefix + ".msp", pos, prefix + "_ref.lai")
    t = time.perf_counter() - t0
    same = subprocess.call(["cmp", "-s", prefix + ".lai", prefix + "_ref.lai"]) == 0
    emit(a.out, step="lai_ref", what="msp_to_lai", N=N, s=round(t, 3), bytes=os.path.getsize(prefix + "_ref.lai"), same_bytes_as_write_lai=same)
    os.remove(prefix + "_ref.lai")


def step_lai_ref(a):
    _lai_ref(a, N_WRITE)


def step_lai_small(a):
    _write_all(a, N_SMALL, ("msp", "lai"))
    _lai_ref(a, N_SMALL)


STEPS = {"kernels": step_kernels, "writers": step_writers, "bed_ref": step_bed_ref, "lai_ref": step_lai_ref, "lai_small": step_lai_small}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_outputs_bench.jsonl"))
    p.add_argument("--tmp", default="/dev/shm/gnx_label_outputs")
    p.add_argument("--lai-timeout", type=int, default=600)
    p.add_argument("--steps", default="kernels,writers,bed_ref,lai_ref")
    p.add_argument("--step", help="(internal) run one step in this process")
    a = p.parse_args()
    if a.step:
        STEPS[a.step](a)
        return 0
    os.makedirs(a.tmp, exist_ok=True)
    open(a.out, "w").close()
    try:
        for name in a.steps.split(","):
            limit = a.lai_timeout if name == "lai_ref" else LIMITS[name]
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--out", a.out, "--tmp", a.tmp]
            rc = subprocess.call(cmd)
            if rc in (124, 137) and name == "lai_ref":
                emit(a.out, step="lai_ref", what="msp_to_lai", N=N_WRITE, finished=False, limit_s=limit,
                     note="did not finish within the limit: the comparison below is at N = %d" % N_SMALL)
                rc = subprocess.call(["timeout", "-k", "10", str(LIMITS["lai_small"]), sys.executable, os.path.abspath(__file__), "--step",
                                      "lai_small", "--out", a.out, "--tmp", a.tmp])
            if rc != 0:
                print("step %s ended with status %d: stopping" % (name, rc), file=sys.stderr)
                return rc
    finally:
        shutil.rmtree(a.tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
