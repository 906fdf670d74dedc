#!/usr/bin/env python3
"""Gnofix with search options against the default loop, device-resident, at config 5b's geometry (chr1 WGS: W = 1431, A = 12,
S = 75, 1200 trees; 2048 individuals with two switch errors each — scripts/bench_configs.py c5br).

  python scripts/bench_gnofix_opts.py [--individuals 2048] [--reps 2]

Times gnx_gnofix_dev (the default path: the yardstick) and gnx_gnofix_ex_dev once per option, and prints one JSON line: seconds,
individuals/s, mean accepted switches, the rows walked per candidate batch (2K switched rows against the default's 2) and the
slow-down against the default.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnomix_amd  # noqa: E402
from gnomix_amd import synth  # noqa: E402

OPTIONS = [
    ("prior_switch_prob=0.45", dict(prior_switch_prob=0.45)),
    ("prob_comp=prod", dict(prob_comp="prod")),
    ("padding=False", dict(padding=False)),
    ("max_center_offset=3", dict(max_center_offset=3)),
    ("non_lin_s=3", dict(non_lin_s=3)),
    ("check_criterion=disc_base", dict(check_criterion="disc_base")),
    ("check_criterion=disc_either", dict(check_criterion="disc_either")),
    ("check_criterion=all", dict(check_criterion="all")),
]


def rows_per_batch(opt):
    off, nls = opt.get("max_center_offset", 0), opt.get("non_lin_s", 0)
    return 2 * (2 * off + 1 + max(nls - 1, 0) + nls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--individuals", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--max-it", type=int, default=50)
    a = ap.parse_args()
    n_ind = a.individuals
    W, A, S = 1431, 12, 75
    C = 1000 * W + 500
    data = gnomix_amd.GnxModelData(C=C, M=1000, A=A, S=S, context=500, smooth_kind="xgb")
    for k, v in synth.synthetic_smoothing_trees(100, A, S, seed=6).items():
        setattr(data, k, v)
    model = gnomix_amd.DeviceModel(data)
    B = synth.synthetic_phased_individuals(n_ind, W, A, seed=3)
    Xd = torch.randint(0, 2, (2 * n_ind, C), dtype=torch.int8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    Bd = torch.from_numpy(B).cuda()

    def timed(**opt):
        best, ns = 1e9, None
        for rep in range(a.reps + 1):  # the first run sizes the workspaces
            w = Xd.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ns = model.gnofix_device(w, Bd, max_it=a.max_it, **opt)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = min(best, dt) if rep else best
        return best, float(ns.float().mean())

    t_def, sw_def = timed()
    res = {"geometry": "W=1431 A=12 S=75 1200 trees", "individuals": n_ind, "max_it": a.max_it,
           "default": {"seconds": t_def, "individuals_per_s": n_ind / t_def, "mean_switches": sw_def, "rows_per_batch": 2}, "options": {}}
    for name, opt in OPTIONS:
        t, sw = timed(**opt)
        res["options"][name] = {"seconds": t, "individuals_per_s": n_ind / t, "mean_switches": sw, "rows_per_batch": rows_per_batch(opt),
                                "slowdown_vs_default": t / t_def}
        print(name, res["options"][name], file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
