"""CPU side of the tree bases' edge tests (tests/test_gpu_forest_edges.py): what those tests take for granted about their own models,
their reference and the oracle, checked without a device.
  - the numpy reference (tests/forest_cases.reference: a walk of the original tree arrays over the padded slice) and the C oracle
    agree on every case: bit for bit in float64 for the random forest, within the project's float32 bar (_close_f32 of
    tests/test_gpu_parity.py) for the boosted trees — the two differ in expf alone (glibc's against float(exp(double)));
  - the split rules are xgboost's (missing -> default child, else left iff float(v) < threshold) and scikit-learn's (left iff
    float32(v) <= threshold), checked on stumps against the rule written out per SNP value;
  - every case reaches the launch paths it claims, under the launch arithmetic restated in tests/forest_cases.py, and the whole list
    reaches every path of the two kernels' run machinery at a run length above 1;
  - every window of every model splits on the positions tests/forest_cases.required_positions demands;
  - at the sizes of the suite's parity tests the launchers' own cost models choose a run length of 1 (why the knob is forced)."""
import numpy as np
import pytest

import forest_cases as FC

IDS = [c.name for c in FC.CASES]


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_reference_against_oracle(oracle, case):
    ref, got = FC.reference(case.name), FC.oracle_output(oracle, case)
    g = case.g
    assert ref.shape == got.shape == (case.N, g.W, case.A)
    if case.rf:
        assert ref.dtype == got.dtype == np.float64
        assert np.array_equal(ref, got)
        assert np.max(np.abs(ref.sum(-1) - 1)) < 1e-12
    else:
        print("%s: %d of %d cells differ, max |diff| %.3g" % (case.name, np.count_nonzero(ref != got), ref.size, np.max(np.abs(ref - got))))
        FC.close_f32(ref, got)
        # the outputs move: a reference that ignored its trees would pass the comparison of two such references
        assert np.ptp(ref[..., 0]) > 1e-3


@pytest.mark.parametrize("missing", range(4))
def test_xgb_split_rule_on_stumps(oracle, missing):
    """one stump per (threshold, default direction) on SNP 0 of a single window: the leaf each SNP value takes, by xgboost's rule"""
    f32 = np.float32
    X = np.zeros((4, 17), np.int8)
    X[:, 0] = np.arange(4)
    for thr in FC.XGB_THR:
        for dl in (0, 1):
            T = oracle.Trees([0, 3], [1, -1, -1], [2, -1, -1], [0, 0, 0], [thr, -1.0, 1.0], [0], 2, 0.5, default_left=[dl, 0, 0])
            p = oracle.base_forest(T, [0, 1], X, 16, 0, 2, missing=missing)[:, 0, 1]
            for v in range(4):
                left = bool(dl) if v == missing else f32(v) < f32(thr)
                assert (p[v] < 0.5) == left, (thr, dl, v)


def test_rf_split_rule_on_stumps(oracle):
    X = np.zeros((4, 17), np.int8)
    X[:, 0] = np.arange(4)
    value = np.array([[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]])
    for thr in FC.RF_THR:
        rf = dict(win_tree0=[0, 1], tree_off=[0, 3], left=[1, -1, -1], right=[2, -1, -1], feat=[0, 0, 0], thr=[thr, -2.0, -2.0], value=value)
        p = oracle.base_rforest(rf, X, 16, 0, 2)[:, 0, 0]
        for v in range(4):
            assert (p[v] == 1.0) == (np.float64(np.float32(v)) <= thr), (thr, v)


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_claimed_paths(case):
    p = FC.paths(case)
    assert case.claims.keys() <= p.keys()
    for k, v in case.claims.items():
        assert p[k] == v, (case.name, k, p[k], v)
    g, runs = case.g, case.run_lengths()
    assert p["forest2"], "GNX_FOREST_IMPL=0 must run k_base_forest2 on every case"
    assert 1 in runs and max(runs) > 1 and all(1 <= e <= g.W - 1 for e in p["wrun_eff"].values())
    assert g.rem > 0 and g.C >= 16 and case.depth <= 8
    if case.rf:
        assert case.A <= FC.H2 * FC.CG2


def test_run_lengths_of_the_geometry_cases():
    """1, 2, 3, one that does not divide the main windows and one the launcher has to clamp, on every geometry"""
    for case in FC.CASES:
        if case.wruns is None:
            nw, r = case.g.W - 1, case.run_lengths()
            assert {1, 2, 3} <= set(r) and any(nw % x for x in r) and any(x >= nw for x in r) and max(r) > nw
            assert FC.paths(case)["wrun_eff"][max(r)] == nw


def test_every_path_is_reached_with_runs():
    """over the whole list, at a run length above 1"""
    pre, tpre, ring_same, counts, tpw = set(), set(), set(), set(), {}
    for case in FC.CASES:
        p = FC.paths(case)
        assert max(p["wrun_eff"].values()) > 1
        if not case.rf:
            pre |= {("x", k) for k in p["pre"]}
            tpre |= {("x", t) for t in p["tpre"]}
            for n, b in p["f2_batches"].items():
                tpw.setdefault(p["f2_tpw"], set()).add(n)
        else:
            pre |= {("r", k) for k in p["pre"]}
            tpre |= {("r", t) for t in p["tpre"]}
        ring_same.add((case.kind, p["ring"][0] == p["ring"][1]))
        counts.add(case.N)
    for kind in "xr":
        assert {(kind, k) for k in ("true", "pad", "size")} <= pre
        assert {(kind, True), (kind, False)} <= tpre
        assert {(kind, True), (kind, False)} <= ring_same
    assert {1, 129, 257} <= counts
    assert set(FC.ALL_COUNTS_D4) <= tpw[10]
    assert {7, 9, 17} <= tpw[8] and {5, 7, 13} <= tpw[6]      # TPW - 1, TPW + 1, 2 TPW + 1
    names = {c.name for c in FC.CASES}
    assert {"%s-depth%d" % (k, D) for k in "xr" for D in range(1, 9)} <= names
    assert {c.A for c in FC.CASES if not c.rf} >= {2, 3, 5} and {c.A for c in FC.CASES if c.rf} >= {9, 17, 32}
    assert any(FC.paths(c)["empty_class"] for c in FC.CASES) and any(FC.paths(c)["unequal"] for c in FC.CASES)
    assert {c.missing for c in FC.CASES if c.enumerate_splits and not c.rf} == {0, 1, 2, 3}
    p = FC.paths(FC.BY_NAME[FC.HALVES_CASE])
    assert p["f1_halves"] == 2 and FC.paths(FC.BY_NAME[FC.HALVES_CASE], halves_knob=1)["f1_halves"] == 1


def test_geometry_properties():
    G, ww = FC.GEO, FC.window_words
    assert {(w * 100) & 15 for w in range(G["drift"].W)} == {0, 4, 8, 12} and G["drift"].M % 16 == 4
    g = G["ringchg"]
    assert (g.width, g.width_last, FC.ring_words(g.width), FC.ring_words(g.width_last), g.M % 16) == (224, 264, 16, 32, 0)
    g = G["noov"]
    assert all(ww(g, w)[1] == ww(g, w + 1)[0] for w in range(g.W - 2))
    g = G["share1"]
    assert {ww(g, w)[1] - ww(g, w + 1)[0] for w in range(g.W - 2)} == {0, 1}
    g = G["deepctx"]
    assert g.ctx > g.M
    kinds = [FC.forest1_pre(g, w) for w in range(g.W - 2)]
    assert kinds[0] == "true" and kinds[-1] == "pad" and kinds.count("pad") >= 2 and "size" not in kinds
    assert sum(1 for w in range(g.W) if w * g.M < g.ctx) >= 3 and sum(1 for w in range(g.W) if w * g.M + g.width_of(w) > g.ctx + g.C) >= 3
    g = G["odd"]
    assert g.M % 2 == 1 and g.ctx % 2 == 1
    g = G["wide"]
    assert all(ww(g, w + 1)[1] - ww(g, w)[1] > 64 for w in range(g.W - 2)) and FC.ring_words(g.width) == 128


def test_the_cost_models_choose_single_windows_at_test_sizes():
    """the largest forest shape of tests/test_gpu_parity.py (N = 70, 40 windows: 40 blocks), and every case here, left to the launchers"""
    lds2 = FC.forest2_lds_bytes(7, FC.ring_words(200), 140, 4, False)
    assert FC.forest2_wrun(70, 39, lds2) == 1 and FC.forest1_wrun(70, 39, 128) == 1
    assert FC.forest2_wrun(300, 24, FC.forest2_lds_bytes(3, 16, 15, 2, False)) == 1
    for case in FC.CASES:
        assert FC.paths(case)["wrun_auto"] == (1, 1)
    # chr22 / 10 000 haplotypes: both choose long runs
    assert FC.forest2_wrun(10000, 369, FC.forest2_lds_bytes(7, 128, 140, 4, False)) > 1
    assert FC.forest1_wrun(10000, 369, 256) > 1


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_placed_splits(case):
    wt0, off, left, right, feat = FC.tree_arrays(case)
    g = case.g
    counts = case.window_counts()
    assert len(wt0) == g.W + 1
    depth = 0
    for w in range(g.W):
        on = set()
        assert wt0[w + 1] - wt0[w] == counts[w].sum() >= 1
        for t in range(wt0[w], wt0[w + 1]):
            o, n = off[t], off[t + 1] - off[t]
            inner = left[o:o + n] != -1
            on.update(feat[o:o + n][inner].tolist())
            d = np.zeros(n, np.int64)                 # preorder: children come after their parent
            for k in range(n):
                if inner[k]:
                    d[left[o + k]] = d[right[o + k]] = d[k] + 1
            depth = max(depth, int(d.max()))
            if not case.rf and case.A > 2:
                assert 0 <= FC.build(case.name)["fb_tree_class"][t] < case.A
        need = FC.required_positions(g, w)
        assert set(need) <= on, (case.name, w, sorted(set(need) - on))
        assert max(on) < g.width_of(w)
        s = w * g.M                                   # the demanded positions, spelled out once more
        assert {0, g.width_of(w) - 1} <= set(need)
        for b in range(16 * ((s >> 4) + 1), s + g.width_of(w), 16):
            assert {b - 1 - s, b - s} <= set(need)
    assert depth == case.depth
    if not case.rf and case.A > 2:
        cls = FC.build(case.name)["fb_tree_class"]
        assert all(np.array_equal(np.bincount(cls[wt0[w]:wt0[w + 1]], minlength=case.A), counts[w]) for w in range(g.W))
    if case.enumerate_splits:
        m = FC.build(case.name)
        inner = left != -1
        if case.rf:
            assert set(m["rf_thr"][inner].tolist()) == set(FC.RF_THR)
        else:
            assert {(float(t), int(d)) for t, d in zip(m["fb_cond"][inner], m["fb_default_left"][inner])} == {(t, d) for t in FC.XGB_THR for d in (0, 1)}
        assert set(np.unique(FC.inputs(case.name)).tolist()) == {0, 1, 2, 3}
