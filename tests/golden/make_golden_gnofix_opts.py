#!/usr/bin/env python3
"""Generate tests/golden/G24_gnofix_opts.npz by RUNNING THE REFERENCE's gnofix() (src/Gnofix/gnofix.py:58-208) with its search
options: check_criterion, max_center_offset, non_lin_s, prob_comp, prior_switch_prob, padding.  The oracle tree walker stands in
for the xgboost model (oracle.OracleXGBSmoother), as in make_golden.make_G5; the plotting packages the reference imports are
stubbed the same way.  Run where the reference is present (numpy >= 2: gnofix.py:171 compares float32 products under NEP 50);
it skips cleanly elsewhere.

Geometries: W = 2S with S = 3 and S = 5 (the smallest the loader allows; max_center_offset = (S-1)/2 reaches the switch at
window 0 there) and G5's shape W = 160, S = 75, A = 4 with offset 3 and non_lin_s 3.  Option sets: every option alone and two
combined sets.  Stored per geometry g: the trees (g_t_*), the inputs (g_X int8 (2n, C), g_B (2n, W, A)), the case list (g_cases:
JSON strings of the options incl. max_it) and per case k the reference's outputs g_k_oX (2n, C), g_k_oY (2n, W), g_k_trk (n, 2, W)
and g_k_nhist (n,) (history length: accepted switches + 2).

The generator ASSERTS that every option set changes the result against the defaults on at least one individual of its geometry,
and that an accepted double switch and an accepted single switch at window 0 occur — otherwise the fixture would show nothing.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: gnofix_opts_exact
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: oracle
import make_golden as G  # noqa: E402  (import_reference, handmade_smoothing_trees, trees_to_npz)

OUT = os.path.join(HERE, "G24_gnofix_opts.npz")


def option_sets(S, off, nls):
    return [
        dict(),
        dict(check_criterion="all"),
        dict(check_criterion="disc_base"),
        dict(check_criterion="disc_either"),
        dict(max_center_offset=off),
        dict(non_lin_s=nls),
        dict(prob_comp="prod"),
        dict(prior_switch_prob=0.35),
        dict(prior_switch_prob=0.65),
        dict(padding=False),
        dict(check_criterion="all", max_center_offset=off, non_lin_s=nls, prob_comp="prod", prior_switch_prob=0.45),
        dict(check_criterion="disc_either", max_center_offset=off, non_lin_s=nls, padding=False, prior_switch_prob=0.6),
    ]


def individuals(rng, n, W, A, C, noise, n_scramble):
    """piecewise-constant ancestry per haplotype, noisy base probabilities, phase scrambled at random windows"""
    X = rng.randint(0, 2, size=(2 * n, C)).astype(np.int8)
    B = np.empty((2 * n, W, A))
    for i in range(n):
        for h in range(2):
            y = np.empty(W, dtype=int)
            a = rng.randint(A)
            for w in range(W):
                if rng.rand() < 2.0 / W:
                    a = rng.randint(A)
                y[w] = a
            b = np.full((W, A), noise / (A - 1))
            b[np.arange(W), y] = 1 - noise
            b = b * rng.uniform(0.5, 1.5, size=b.shape)
            B[2 * i + h] = b / b.sum(1, keepdims=True)
        for s in rng.choice(np.arange(1, W), size=n_scramble, replace=False):
            B[2 * i, s:], B[2 * i + 1, s:] = B[2 * i + 1, s:].copy(), B[2 * i, s:].copy()
    return X, B


def main():
    if not G.import_reference():
        print("reference absent: G24 skipped")
        return
    from oracle import gnx_oracle as O
    from src.Gnofix.gnofix import gnofix
    from gnofix_opts_exact import gnofix_opts
    assert int(np.__version__.split(".")[0]) >= 2, "gnofix.py:171 must run under NEP 50 (numpy >= 2)"

    geoms = {
        # name: (W, A, S, Mw, rem, n_ind, trees, offset, non_lin_s, max_it, noise, scrambles)
        "s3": (6, 3, 3, 3, 2, 8, ("random", 3, 3, 31), 1, 1, 6, 0.45, 2),
        "s5": (10, 3, 5, 2, 1, 8, ("random", 4, 4, 52), 2, 2, 6, 0.45, 3),
        "g5": (160, 4, 75, 6, 3, 4, ("handmade",), 3, 3, 8, 0.55, 5),
    }
    d = {}
    saw_double = saw_zero = False
    for gi, (g, (W, A, S, Mw, rem, n, tr, off, nls, max_it, noise, nscr)) in enumerate(geoms.items()):
        Cn = W * Mw + rem
        T = G.handmade_smoothing_trees(A, S) if tr[0] == "handmade" else \
            O.random_trees(tr[1], A, S * A, depth=tr[2], seed=tr[3], leaf_scale=1.0)
        sm = O.OracleXGBSmoother(T, W, A, S)
        rows = lambda r: O.xgb_predict_proba(T, np.asarray(r, dtype=np.float32))
        labs = lambda b: O.smooth_xgb(T, b, S)[1]
        rng = np.random.RandomState(2400 + gi)
        X, B = individuals(rng, n, W, A, Cn, noise, nscr)
        d.update({g + "_W": W, g + "_A": A, g + "_S": S, g + "_C": Cn, g + "_X": X, g + "_B": B})
        d.update(G.trees_to_npz(g + "_t_", T))
        cases = option_sets(S, off, nls)
        d[g + "_cases"] = np.array([json.dumps(dict(c, max_it=max_it), sort_keys=True) for c in cases])
        results = []
        for k, opt in enumerate(cases):
            oX, oY, trk, nh = [], [], [], []
            for i in range(n):
                r = gnofix(X[2 * i].astype(int), X[2 * i + 1].astype(int), B=B[2 * i:2 * i + 2], smoother=sm, max_it=max_it, **opt)
                X_m, X_p, Y_m, Y_p, history, tracker = r
                oX += [X_m, X_p]; oY += [Y_m, Y_p]; trk.append(np.array(tracker)); nh.append(history.shape[-1] if history.ndim == 3 else 1)
                # the restatement on the same case: equal to the reference, and its event list says what was accepted
                ev = []
                e = gnofix_opts(X[2 * i], X[2 * i + 1], B[2 * i:2 * i + 2], S, rows, labs, max_it=max_it, events=ev, **opt)
                assert np.array_equal(e[0], X_m) and np.array_equal(e[1], X_p) and np.array_equal(e[2], Y_m) and np.array_equal(e[3], Y_p)
                assert np.array_equal(e[4], np.array(tracker)) and e[5] == nh[-1] - 2
                saw_double |= any(j2 is not None for (_, _, j2) in ev)
                saw_zero |= any(j2 is None and j1 == 0 for (_, j1, j2) in ev)
            res = (np.array(oX), np.array(oY), np.array(trk), np.array(nh))
            results.append(res)
            if k > 0:
                base = results[0]
                changed = [i for i in range(n) if not all(np.array_equal(a[i * (len(a) // n):(i + 1) * (len(a) // n)], b[i * (len(b) // n):(i + 1) * (len(b) // n)])
                                                            for a, b in zip(res, base))]
                assert changed, "%s: option set %r changes nothing against the defaults" % (g, opt)
                print("G24", g, opt, "changes individuals", changed, "switches", (res[3] - 2).tolist())
            else:
                print("G24", g, "defaults: switches", (res[3] - 2).tolist())
            d["%s_%d_oX" % (g, k)] = res[0].astype(np.int8)
            d["%s_%d_oY" % (g, k)] = res[1].astype(np.int8)
            d["%s_%d_trk" % (g, k)] = res[2].astype(np.int8)
            d["%s_%d_nhist" % (g, k)] = res[3].astype(np.int32)
    assert saw_double, "no accepted double switch in the fixture"
    assert saw_zero, "no accepted switch at window 0 in the fixture"
    d["geoms"] = np.array(list(geoms))
    np.savez_compressed(OUT, **d)
    print("G24 ok:", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
