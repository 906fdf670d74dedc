"""gnofix() of the reference with its search options (src/Gnofix/gnofix.py:58-208, src/Gnofix/phasing.py:182-198), restated in
plain numpy with `oracle.gnx_oracle.gnofix`'s calling convention plus the options.  Not a copy: index arithmetic instead of the
reference's list building, one place per quirk.  tests/test_gnofix_opts_host.py pins it to the reference's own outputs
(tests/golden/G24_gnofix_opts.npz) and, at the defaults, to oracle.gnofix; the GPU fuzz then uses it as the reference.

The quirks it reproduces on purpose:
  * np.argmax over the candidates: first maximum, candidates in the order singles, left doubles, right doubles;
  * gnofix.py:171 under numpy >= 2 (NEP 50): float32 * Python float stays float32, and 1 - prior is taken in double first;
  * an accepted double switch [j1, j2) exchanges B and the tracker on [j1, j2) but X only from j2 on (M_track is rebuilt from
    zeros for each index and only the last survives to correct_phase_error);
  * a single switch at window 0 exchanges all of B and leaves X alone (a constant M_track has no correction index).
"""
import numpy as np

CHECKS = ("disc_smooth", "all", "disc_base", "disc_either")
PROB_COMPS = ("max", "prod")
DEFAULTS = dict(check_criterion="disc_smooth", max_center_offset=0, non_lin_s=0, prob_comp="max", prior_switch_prob=0.5,
                padding=True)


def candidates(w, off, nls):
    """exchanged window ranges [j1, j2) of the candidates at w; j2 = None: a single switch (to the end)"""
    out = [(j, None) for j in range(w - off, w + off + 1)]
    out += [(w - j, w) for j in range(1, nls)]
    out += [(w, w + j + 1) for j in range(nls)]
    return out


def _exchange(a, b, j1, j2):
    a2, b2 = a.copy(), b.copy()
    a2[j1:j2], b2[j1:j2] = b[j1:j2], a[j1:j2]
    return a2, b2


def gnofix_opts(M_hap, P_hap, B, S, predict_rows, predict_labels, max_it=50, check_criterion="disc_smooth", max_center_offset=0,
                non_lin_s=0, prob_comp="max", prior_switch_prob=0.5, padding=True, events=None, stats=None):
    """One individual.  predict_rows(rows (R, S*A)) -> (R, A) float32; predict_labels(B (2, W, A)) -> (2, W).
    Returns X_m, X_p, Y_m, Y_p, tracker (2, W), n_switches.  `events`, if a list, receives (w, j1, j2) of every accepted switch; `stats`, if a dict, the number of sweeps run and whether
    the loop ended at the iteration cap (max_it sweeps without the convergence stop)."""
    assert check_criterion in CHECKS and prob_comp in PROB_COMPS
    B = np.array(B, copy=True)
    _, W, A = B.shape
    ws = len(M_hap) // W
    half = (S - 1) // 2
    assert 0 <= max_center_offset <= half and 0 <= non_lin_s <= half
    X_m, X_p = np.array(M_hap, dtype=int, copy=True), np.array(P_hap, dtype=int, copy=True)
    Y = np.asarray(predict_labels(B)).reshape(2, W)
    c_lo, c_hi = half, W - 1 - half
    windows = range(1, W) if padding else range(c_lo, c_hi + 1)
    trk_m, trk_p = np.zeros(W, dtype=int), np.ones(W, dtype=int)
    prior32 = np.float32(prior_switch_prob)
    rest32 = np.float32(1.0 - prior_switch_prob)  # double subtraction, then float32
    seen, n_switch, converged = [], 0, False
    for _ in range(max_it):
        if any(np.array_equal(X_m, s) for s in seen):
            converged = True
            break
        seen.append(X_m.copy())
        for w in windows:
            smooth = Y[0, w] != Y[0, w - 1] or Y[1, w] != Y[1, w - 1]
            am = np.argmax(B[:, w - 1:w + 1, :], axis=2)
            base = am[0, 0] != am[0, 1] or am[1, 0] != am[1, 1]
            go = {"all": True, "disc_smooth": smooth, "disc_base": base, "disc_either": base or smooth}[check_criterion]
            if not go:
                continue
            inside = c_lo <= w <= c_hi
            center = min(max(w, c_lo), c_hi)
            lo, hi = center - half, center + half + 1
            cands = candidates(w, max_center_offset if inside else 0, non_lin_s if inside else 0)
            rows = [B[0, lo:hi], B[1, lo:hi]]
            for (j1, j2) in cands:
                m, p = _exchange(B[0], B[1], j1, W if j2 is None else j2)
                rows += [m[lo:hi], p[lo:hi]]
            outs = np.asarray(predict_rows(np.stack(rows).reshape(len(rows), -1)), dtype=np.float32).reshape(-1, 2, A)
            top = outs.max(axis=2)                                     # (1 + K, 2) float32
            probs = top[:, 0] * top[:, 1] if prob_comp == "prod" else top.max(axis=1)
            k = int(np.argmax(probs[1:]))
            if np.float32(probs[1 + k]) * prior32 > np.float32(probs[0]) * rest32:
                j1, j2 = cands[k]
                e2 = W if j2 is None else j2
                B = np.stack(_exchange(B[0], B[1], j1, e2))
                trk_m, trk_p = _exchange(trk_m, trk_p, j1, e2)
                last = j1 if j2 is None else j2                       # the only index correct_phase_error sees
                if last >= 1:
                    X_m, X_p = _exchange(X_m, X_p, last * ws, len(X_m))
                Y = np.asarray(predict_labels(B)).reshape(2, W)
                n_switch += 1
                if events is not None:
                    events.append((w, j1, j2))
    if stats is not None:
        stats.update(sweeps=len(seen), capped=not converged and max_it > 0)
    return X_m, X_p, Y[0], Y[1], np.stack([trk_m, trk_p]), n_switch
