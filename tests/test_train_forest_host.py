"""The restatement of the boosted-tree base trainer (tests/gbt_base_exact.py) against brute force, on the CPU: every node's split is
re-derived by enumerating all three partitions of every feature with the gains in exact rational arithmetic, and one stump is worked
by hand.  The GPU trainer is then held to the restatement bit for bit (tests/test_gpu_train_forest.py)."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbt_base_exact as E  # noqa: E402

ONE = 2 ** 30


def _brute_best(Xw, g, h, rows, lam, gamma, mcw):
    """the best (gain, feature, candidate) of a node by enumeration, gains as Fractions; None when no candidate is valid"""
    G, H = sum(g[n] for n in rows), sum(h[n] for n in rows)
    lamf, floor_ = Fraction(lam), max(Fraction(gamma), Fraction(1e-6))
    score = lambda a, b: Fraction(a, ONE) ** 2 / (Fraction(b, ONE) + lamf)
    best = None
    for j in range(Xw.shape[1]):
        parts = {1: [n for n in rows if Xw[n, j] == 0], 2: [n for n in rows if Xw[n, j] in (0, 2)], 3: [n for n in rows if Xw[n, j] in (0, 1)]}
        for c in (1, 2, 3):
            GL, HL = sum(g[n] for n in parts[c]), sum(h[n] for n in parts[c])
            if Fraction(HL, ONE) < Fraction(mcw) or Fraction(H - HL, ONE) < Fraction(mcw):
                continue
            gain = score(GL, HL) + score(G - GL, H - HL) - score(G, H)
            if gain > floor_ and (best is None or gain > best[0]):
                best = (gain, j, c)
    return best, G, H


@pytest.mark.parametrize("N,width,A,depth,seed", [(12, 5, 3, 3, 0), (12, 4, 2, 2, 1), (9, 5, 2, 3, 2), (11, 3, 3, 2, 3), (12, 5, 3, 5, 4)])
def test_restatement_equals_brute_force(N, width, A, depth, seed):
    rng = np.random.RandomState(seed)
    Xw = rng.choice(3, size=(N, width), p=[0.45, 0.4, 0.15]).astype(np.int8)
    Xw[:, width - 1] = Xw[:, 0]          # a feature tie: the lower index must win
    y = rng.randint(A, size=N)
    eta, lam, gamma, mcw = 0.3, 1.0, 0.0, 0.25
    trace = []
    trees, losses, _ = E.train_window(Xw, y, A, n_rounds=3, max_depth=depth, eta=eta, lam=lam, gamma=gamma, mcw=mcw, trace=trace)
    assert len(trace) == 3 * (1 if A == 2 else A)
    n_split = 0
    for t in trace:
        for nd in t["nodes"]:
            best, G, H = _brute_best(Xw, t["g"], t["h"], nd["rows"], lam, gamma, mcw)
            assert (G, H) == (nd["G"], nd["H"])
            at_depth_limit = nd["node"] >= 2 ** depth - 1
            if nd["split"] is None:
                assert best is None or at_depth_limit
                exact = Fraction(eta) * (-Fraction(G, ONE) / (Fraction(H, ONE) + Fraction(lam)))
                # float32 rounding (2^-24 relative) of a float64 value three roundings (2^-53 each) from the exact one
                assert abs(Fraction(float(nd["value"])) - exact) <= abs(exact) * Fraction(2 ** 20 + 1, 2 ** 44)
            else:
                assert best is not None and not at_depth_limit
                assert nd["split"] == (best[1], best[2])
                assert nd["split"][0] != width - 1 or not np.array_equal(Xw[:, 0], Xw[:, width - 1])
                assert abs(nd["gain"] - float(best[0])) <= 1e-12 * max(1.0, float(best[0]))
                n_split += 1
    assert n_split >= 3
    assert np.allclose(losses[0], math.log(A), rtol=0, atol=1e-15)     # uniform probabilities before the first round


def test_hand_computed_stump():
    """N = 4, one SNP, A = 2 (binary), one round of depth 1, eta 0.1, lambda 1, min_child_weight 0.5.
    Margin 0 -> p = 1/2 for every row: g = +1/2 (y = 0) or -1/2 (y = 1), h = 1/4, i.e. +-2^29 and 2^28 in fixed point.
    Root G = 0, H = 1.  Candidate 1 ({0} | {1}): GL = 1, HL = 1/2, GR = -1, HR = 1/2: gain = 1/1.5 + 1/1.5 - 0 = 4/3.  Candidate 2 is
    the same partition (no missing rows) and loses the tie; candidate 3 has an empty right child.
    Leaves: -0.1 * (+1 / 1.5) = -1/15 on the left, +1/15 on the right, as float32 0.06666667014360428.
    Loss: ln 2 before; after, every row has p_y = sigmoid(1/15): -log = log(1 + exp(-0.06666667014360428)) = 0.6603692982514406."""
    Xw = np.array([[0], [0], [1], [1]], np.int8)
    y = np.array([0, 0, 1, 1])
    trace = []
    trees, losses, F = E.train_window(Xw, y, 2, n_rounds=1, max_depth=1, eta=0.1, lam=1.0, gamma=0.0, mcw=0.5, trace=trace)
    t = trace[0]
    assert t["g"] == [2 ** 29, 2 ** 29, -2 ** 29, -2 ** 29] and t["h"] == [2 ** 28] * 4
    root = [nd for nd in t["nodes"] if nd["node"] == 0][0]
    assert (root["G"], root["H"], root["split"]) == (0, 2 ** 30, (0, 1))
    assert root["gain"] == pytest.approx(4.0 / 3.0, rel=0, abs=1e-15)
    nodes, k = trees[0]
    assert k == 0 and nodes[0] == ("split", 0, 1)
    assert float(nodes[1][1]) == -0.06666667014360428 and float(nodes[2][1]) == 0.06666667014360428
    assert F[:, 0].tolist() == [np.float32(-1 / 15)] * 2 + [np.float32(1 / 15)] * 2
    assert np.allclose(losses[0], 0.6931471805599453, rtol=0, atol=1e-15)
    assert np.allclose(losses[1], 0.6603692982514406, rtol=0, atol=1e-15)
    # the same through train(): the fb_* layout of one window
    X = np.array([[0, 0], [0, 0], [1, 1], [1, 1]], np.int8)
    X3 = np.concatenate([X, X[:, :1]], axis=1)      # C = 3, M = 2, ctx = 0: one window of width 3
    fb, loss = E.train(X3, y[:, None], 2, 0, 2, n_rounds=1, max_depth=1, eta=0.1, lam=1.0, gamma=0.0, mcw=0.5)
    assert fb["fb_win_tree0"].tolist() == [0, 1] and fb["fb_tree_off"].tolist() == [0, 3]
    assert fb["fb_left"].tolist() == [1, -1, -1] and fb["fb_right"].tolist() == [2, -1, -1] and fb["fb_feat"].tolist() == [0, 0, 0]
    assert fb["fb_cond"].tolist() == [0.5, np.float32(-1 / 15), np.float32(1 / 15)] and fb["fb_default_left"].tolist() == [0, 0, 0]
    assert loss.tolist() == pytest.approx([0.6931471805599453, 0.6603692982514406], rel=0, abs=1e-15)


def test_missing_direction_candidates():
    """missing rows carry the signal: {0, 1} | {missing} (candidate 3) must win, and with the codes 1 <-> 2 exchanged candidate 2"""
    y = np.array([0] * 6 + [1] * 6)
    Xw = np.zeros((12, 2), np.int8)
    Xw[:6, 1] = 2
    Xw[6:, 1] = np.array([0, 1, 0, 1, 0, 1])
    Xw[:, 0] = np.array([0, 1] * 6)
    trees, _, _ = E.train_window(Xw, y, 2, n_rounds=1, max_depth=1)
    assert trees[0][0][0] == ("split", 1, 3)
    Xw2 = Xw.copy()
    Xw2[:6, 1] = 0
    Xw2[6:, 1] = 1
    Xw2[0, 1] = 2               # class 0's missing row belongs with the zeros: {0, missing} | {1} separates the classes
    trees, _, _ = E.train_window(Xw2, y, 2, n_rounds=1, max_depth=1)
    assert trees[0][0][0] == ("split", 1, 2)
