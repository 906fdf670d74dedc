#!/usr/bin/env python3
"""Generate tests/golden/G26_gnofix_calibrated.npz by RUNNING THE REFERENCE's gnofix() (src/Gnofix/gnofix.py:58-208) with a
CALIBRATED smoother: the reference's own Smoother (src/Smooth/smooth.py) with `model` = the oracle tree walker
(oracle.OracleXGBSmoother, as in make_golden_gnofix_opts.py), `calibrator` = the reference's Calibrator fitted by scikit-learn and
`calibrate = True`.  smoother.predict(B) then returns argmax(Calibrator.transform(raw)) while smoother.model.predict_proba(rows)
(gnofix.py:157) stays the raw model.  Run where the reference is present (numpy >= 2); it skips cleanly elsewhere.

Geometries: "a3" (A = 3, S = 5, W = 20, 12 individuals) and "a2" (A = 2: Calibrator.normalize's p0 = 1 - p1 branch; S = 5,
W = 16, 8 individuals), a few shallow trees per class.  The calibrator is fitted on deliberately imbalanced labels (drawn from the
raw probabilities, then a share of the rows relabelled as class 0), so the maps are skewed and calibrated labels differ from the raw arg-max.  Option sets: the defaults,
prob_comp="prod", check_criterion="disc_either", and a combined set with non_lin_s.  Stored per geometry g: the trees (g_t_*), the
maps (g_calib_off / _x / _y; float32 fits), the inputs g_X (2n, C) int8 and g_B (2n, W, A), the initial labels g_Y0 (calibrated)
and g_Y0raw, the case list g_cases (JSON) and per case k the reference's outputs g_k_oX, g_k_oY, g_k_nhist (accepted switches + 2).
For case 0 also g_0_cX / g_0_cY / g_0_cnhist: the same run with the CANDIDATE probabilities calibrated too (a smoother whose
.model returns calibrated rows) — what a kernel that compared calibrated probabilities would give — and g_raw_witness, the
individuals where that differs.

The generator ASSERTS, per option set, that at least a quarter of the individuals end differently (Y, X or switch count) than the
same run with calibrate=False, that at least one initial label differs from the raw arg-max, and (a3) that a raw-probability
witness exists — otherwise the fixture would pass with calibration ignored or applied in the wrong place.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: oracle, gnomix_amd
import make_golden as G  # noqa: E402  (import_reference, trees_to_npz)
from make_golden_gnofix_opts import individuals  # noqa: E402

OUT = os.path.join(HERE, "G26_gnofix_calibrated.npz")


def option_sets(nls):
    return [
        dict(),
        dict(prob_comp="prod"),
        dict(check_criterion="disc_either"),
        dict(check_criterion="all", non_lin_s=nls, prob_comp="prod", prior_switch_prob=0.45),
    ]


class _CalibratedRows:
    """a model whose every probability is calibrated (rows and haplotypes): the WRONG reading of gnofix.py:157, for the witness"""

    def __init__(self, model, calibrator):
        self.model, self.calibrator = model, calibrator

    def predict_proba(self, B):
        return self.calibrator.transform(self.model.predict_proba(B))


def run(gnofix, X, B, sm, n, max_it, opt):
    oX, oY, nh = [], [], []
    for i in range(n):
        X_m, X_p, Y_m, Y_p, history, _ = gnofix(X[2 * i].astype(int), X[2 * i + 1].astype(int), B=B[2 * i:2 * i + 2], smoother=sm,
                                                max_it=max_it, **opt)
        oX += [X_m, X_p]; oY += [Y_m, Y_p]; nh.append(history.shape[-1] if history.ndim == 3 else 1)
    return np.array(oX), np.array(oY), np.array(nh)


def differing(a, b, n):
    return [i for i in range(n) if not (np.array_equal(a[0][2 * i:2 * i + 2], b[0][2 * i:2 * i + 2]) and
                                        np.array_equal(a[1][2 * i:2 * i + 2], b[1][2 * i:2 * i + 2]) and a[2][i] == b[2][i])]


def main():
    if not G.import_reference():
        print("reference absent: G26 skipped")
        return
    from oracle import gnx_oracle as O
    from src.Gnofix.gnofix import gnofix
    from src.Smooth.smooth import Smoother
    from src.Smooth.Calibration import Calibrator
    from gnomix_amd.convert import calibrator_arrays
    assert int(np.__version__.split(".")[0]) >= 2, "gnofix.py:171 must run under NEP 50 (numpy >= 2)"

    geoms = {
        # name: (W, A, S, Mw, rem, n_ind, (rounds, depth, seed), non_lin_s, max_it, noise, scrambles, share relabelled as class 0)
        "a3": (20, 3, 5, 2, 1, 12, (3, 3, 261), 2, 6, 0.45, 4, 0.15),
        "a2": (16, 2, 5, 3, 2, 8, (3, 3, 262), 2, 6, 0.4, 3, 0.08),
    }
    d = {}
    for gi, (g, (W, A, S, Mw, rem, n, tr, nls, max_it, noise, nscr, skew)) in enumerate(geoms.items()):
        Cn = W * Mw + rem
        T = O.random_trees(tr[0], A, S * A, depth=tr[1], seed=tr[2], leaf_scale=1.0)
        walker = O.OracleXGBSmoother(T, W, A, S)
        rng = np.random.RandomState(2600 + gi)
        X, B = individuals(rng, n, W, A, Cn, noise, nscr)
        # the calibrator: raw float32 probabilities of other haplotypes, labels drawn from them, then a share relabelled as class 0
        _, Bfit = individuals(rng, 40, W, A, Cn, noise, nscr)
        pfit = walker.predict_proba(Bfit).reshape(-1, A)
        assert pfit.dtype == np.float32
        q = pfit.astype(np.float64) ** 0.7
        yfit = np.array([rng.choice(A, p=r / r.sum()) for r in q])
        yfit[rng.rand(len(yfit)) < skew] = 0
        cal = Calibrator(A)
        cal.fit(pfit, yfit)

        def smoother(model, calibrate):
            sm = Smoother(n_windows=W, num_ancestry=A, smooth_window_size=S, model=model, calibrate=calibrate)
            sm.calibrator, sm.gnofix = cal, True
            return sm
        sm_cal, sm_raw = smoother(walker, True), smoother(walker, False)
        sm_wrong = smoother(_CalibratedRows(walker, cal), False)
        Y0, Y0raw = sm_cal.predict(B), sm_raw.predict(B)
        assert np.array_equal(Y0raw, O.smooth_xgb(T, B, S)[1])
        assert (Y0 != Y0raw).any(), "%s: no initial label differs from the raw arg-max" % g
        assert np.array_equal(sm_wrong.predict(B), Y0)
        print("G26", g, "initial labels that differ from the raw arg-max: %d of %d" % (int((Y0 != Y0raw).sum()), Y0.size))
        d.update({g + "_W": W, g + "_A": A, g + "_S": S, g + "_C": Cn, g + "_X": X, g + "_B": B,
                  g + "_Y0": Y0.astype(np.int8), g + "_Y0raw": Y0raw.astype(np.int8)})
        d.update(G.trees_to_npz(g + "_t_", T))
        ca = calibrator_arrays(cal.models)
        assert ca["calib_is_f32"]
        d.update({g + "_calib_off": ca["calib_off"], g + "_calib_x": ca["calib_x"], g + "_calib_y": ca["calib_y"]})
        cases = option_sets(nls)
        d[g + "_cases"] = np.array([json.dumps(dict(c, max_it=max_it), sort_keys=True) for c in cases])
        for k, opt in enumerate(cases):
            res = run(gnofix, X, B, sm_cal, n, max_it, opt)
            raw = run(gnofix, X, B, sm_raw, n, max_it, opt)
            ch = differing(res, raw, n)
            print("G26", g, opt, "switches", (res[2] - 2).tolist(), "differs from calibrate=False on", ch)
            assert 4 * len(ch) >= n, "%s %r: only %d of %d individuals differ from the uncalibrated run" % (g, opt, len(ch), n)
            d["%s_%d_oX" % (g, k)] = res[0].astype(np.int8)
            d["%s_%d_oY" % (g, k)] = res[1].astype(np.int8)
            d["%s_%d_nhist" % (g, k)] = res[2].astype(np.int32)
            if k == 0:
                wrong = run(gnofix, X, B, sm_wrong, n, max_it, opt)
                wit = differing(res, wrong, n)
                print("G26", g, "individuals where calibrated candidate probabilities would change the result:", wit)
                d[g + "_0_cX"], d[g + "_0_cY"] = wrong[0].astype(np.int8), wrong[1].astype(np.int8)
                d[g + "_0_cnhist"] = wrong[2].astype(np.int32)
                d[g + "_raw_witness"] = np.array(wit, np.int32)
                if g == "a3":
                    assert wit, "a3: no individual separates raw from calibrated candidate probabilities"
    d["geoms"] = np.array(list(geoms))
    np.savez_compressed(OUT, **d)
    print("G26 ok:", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
