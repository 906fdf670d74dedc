"""CPU side of the CRF smoother's edge tests (tests/test_gpu_crf_smooth_edges.py): what those tests take for granted about their own
inputs, their references and the oracle, checked without a device.
  - the arbiter (log-space forward-backward in longdouble) computes the true marginals: on the tiny chains it agrees within 1e-17
    with a sum over all label paths in 60-digit arithmetic, and with zero transitions it is softmax(theta' B);
  - the oracle (float64, scaled at every window) lies within tests/crf_smooth_cases.bound of the arbiter on every case, and has its
    labels on every grid, threshold and far case;
  - the label comparison rule (compare where the arbiter's top-two gap exceeds twice the bound) leaves out no window of any grid,
    threshold or far case;
  - the tie cases are what they claim: the pair wins often enough, `low_word` puts two marginals into one high word with each of the
    two as the winner, `dead` runs the oracle's sum == 0 branch and gives zeros;
  - each threshold case has the r it claims, as gnx_build_crf computes it, and the scale interval that goes with it."""
import numpy as np
import pytest

import crf_smooth_cases as SC


def _oracle_error(oracle, cid):
    B, state, trans = SC.inputs(cid)
    p_ref, l_ref, _ = SC.reference(cid)
    p, lab = oracle.smooth_crf(np.asarray(B, np.float64), state, trans)
    return float(np.max(np.abs(p.astype(SC.LD) - p_ref))), lab, l_ref


@pytest.mark.parametrize("cid", SC.ENUM_CASES, ids=lambda c: "N%d-W%d-A%d" % c)
def test_arbiter_is_the_sum_over_all_paths(cid):
    N, W, A = cid
    rng = np.random.RandomState(SC._seed(5, N, W, A))
    B = rng.dirichlet(np.ones(A) * 0.5, size=(N, W))
    state, trans = SC.trained_weights(rng, A)
    p, _ = SC.marginals_longdouble(B, state, trans)
    q = SC.marginals_enumerated(B, state, trans)
    err = float(np.max(np.abs(p - q)))
    print("longdouble vs enumeration: %.3g" % err)
    assert err <= 1e-17
    assert float(np.max(np.abs(q.sum(-1) - 1))) <= 1e-18


@pytest.mark.parametrize("cid", [c for c in SC.TIE_IDS if c[1] in ("duplicate", "low_word")], ids=SC.name)
def test_arbiter_is_the_softmax_where_transitions_are_zero(cid):
    B, state, trans = SC.inputs(cid)
    assert not np.any(trans)
    s = np.einsum("nta,al->ntl", B.astype(SC.LD), state.astype(SC.LD))
    e = np.exp(s - s.max(-1, keepdims=True))
    assert float(np.max(np.abs(e / e.sum(-1, keepdims=True) - SC.reference(cid)[0]))) <= 1e-17


@pytest.mark.parametrize("cid", [c for c in SC.ALL_IDS if c[:2] != ("tie", "dead")], ids=SC.name)
def test_oracle_is_within_the_bound_of_the_arbiter(oracle, cid):
    N, W, A = SC.shape(cid)
    B, state, trans = SC.inputs(cid)
    err, lab, l_ref = _oracle_error(oracle, cid)
    b = SC.bound(W, A, state, trans)
    print("oracle vs longdouble: %.3g, bound %.3g, bar %.3g, min gap %.3g" % (err, b, SC.bar(cid), SC.reference(cid)[2].min()))
    assert err <= b                  # measured: at most 6.8e-15 against bounds of 1e-13 .. 6e-11
    ok = SC.comparable(cid)
    assert np.array_equal(lab[ok], l_ref[ok])
    if cid[0] != "tie":
        assert ok.all()              # the rule leaves out no window: the GPU tests compare every label of these cases
        assert np.array_equal(lab, l_ref)


def test_grids_cover_what_they_are_chosen_for():
    A_label = [A for (_, _, A) in SC.LABEL_CASES]
    assert set(A_label) >= {8, 9, 12, 13, 16, 17, 24, 25, 32} and {64 // A for A in A_label if A > 16} == {3, 2}
    for A in (5, 12):
        Ws = {W for (_, W, a) in SC.CHAIN_CASES if a == A}
        assert Ws >= {1, 2, 8, 9, 16, 17, 24, 25}
        plain = {W: sum(1 for t0 in range(8, W, 8) if t0 + 8 < W) for W in Ws}      # segments on the default kernel's fast path
        assert [plain[W] for W in (16, 17, 24, 25, 33)] == [0, 1, 1, 2, 3]
        assert {(W + 3) // 4 for W in Ws} >= {1, 2, 3, 4}                           # chunks in the scan's three-slot ring
    per_block = {(12, "ck"): 4, (12, "row"): 16, (4, "scan"): 64, (20, "lanes"): 12, (7, "lanes"): 36}
    for (A, _), n in per_block.items():
        Ns = {N for (N, _, a) in SC.BLOCK_CASES if a == A}
        assert {n - 1, n, n + 1} <= Ns
    for v in SC.VARIANTS:
        assert SC.resolves_to(v, 20) == "lanes" and SC.resolves_to(v, 8) == v
    assert SC.resolves_to("scan", 9) == "ck"


@pytest.mark.parametrize("cid", SC.THRESHOLD_IDS, ids=SC.name)
def test_threshold_cases_have_the_r_they_claim(cid):
    _, N, W, A, r, above, two = cid
    B, state, trans = SC.inputs(cid)
    got = SC.builder_r(state, trans)
    assert got == (np.nextafter(r, np.inf) if above else r) and got == float(np.max(np.abs(state)) + np.max(np.abs(trans)))
    masks = {37.5: (7, 3), 75.0: (3, 1), 150.0: (1, 0)}
    assert SC.norm_mask(state, trans) == masks[r][int(above)]
    assert np.allclose(B.sum(-1), 2.0 if two else 1.0, rtol=0, atol=1e-14)
    assert (W - 1) & 7 in (7, 0)     # W = 24: the last window is a scale window at every interval; W = 25: at none but 1


@pytest.mark.parametrize("cid", [c for c in SC.TIE_IDS if c[1] in ("duplicate", "low_word")], ids=SC.name)
def test_the_pair_wins_often_enough(cid):
    _, kind, A, j, k, sign = cid
    p, lab, _ = SC.reference(cid)
    wins = SC.pair_wins(cid)
    print("pair wins %d of %d windows" % (wins.sum(), wins.size))
    assert 3 * wins.sum() >= wins.size
    if kind == "duplicate":
        assert np.array_equal(p[..., j], p[..., k]) and np.all(lab[wins] == j)
    else:
        # the higher index must win where its column is the larger one, the lower where it is not; the gap clears the bound
        assert np.all(lab[wins] == (k if sign > 0 else j))
        assert SC.comparable(cid)[wins].all()
        pj, pk = p[..., j].astype(np.float64), p[..., k].astype(np.float64)
        same = SC.high_word(pj)[wins] == SC.high_word(pk)[wins]
        print("share a high word in %d of %d" % (same.sum(), same.size))
        assert 2 * same.sum() >= same.size and np.all(pj[wins] != pk[wins])


def test_low_word_has_both_orders_of_winner():
    for A in {c[2] for c in SC.TIE_IDS if c[1] == "low_word"}:
        winners = set()
        for cid in [c for c in SC.TIE_IDS if c[1] == "low_word" and c[2] == A]:
            winners |= set(np.unique(SC.reference(cid)[1][SC.pair_wins(cid)]))
        assert winners == {cid[3], cid[4]}


@pytest.mark.parametrize("cid", [c for c in SC.TIE_IDS if c[1] == "uniform"], ids=SC.name)
def test_uniform_in_the_oracle(oracle, cid):
    B, state, trans = SC.inputs(cid)
    p, lab = oracle.smooth_crf(B, state, trans)
    assert np.all(p == p[..., :1]) and not np.any(lab)
    assert np.max(np.abs(p - 1.0 / B.shape[2])) <= SC.bar(cid)


@pytest.mark.parametrize("cid", [c for c in SC.TIE_IDS if c[1] == "duplicate"], ids=SC.name)
def test_duplicate_in_the_oracle(oracle, cid):
    _, _, A, j, k, _ = cid
    B, state, trans = SC.inputs(cid)
    p, lab = oracle.smooth_crf(B, state, trans)
    assert np.array_equal(p[..., j], p[..., k])
    assert np.all(lab[SC.pair_wins(cid)] == j)


@pytest.mark.parametrize("cid", [c for c in SC.TIE_IDS if c[1] == "dead"], ids=SC.name)
def test_dead_in_the_oracle(oracle, cid):
    """every potential of one window underflows to 0: the oracle's `sum != 0 ? 1 / sum : 1` branch; all marginals 0, all labels 0"""
    B, state, trans = SC.inputs(cid)
    N, W, A = B.shape
    td = SC.dead_windows(N, W)
    assert np.all((td > 0) & (td < W - 1)) and len(set(td)) == 3
    s = np.einsum("nta,al->ntl", B, state)
    assert np.all(np.exp(s[np.arange(N), td]) == 0.0) and np.all(np.delete(s, td, axis=1) > -100)
    p, lab = oracle.smooth_crf(B, state, trans)
    assert np.all(np.isfinite(p)) and not np.any(p) and not np.any(lab)


@pytest.mark.parametrize("cid", [c for c in SC.TIE_IDS if c[1] in ("b_onehot", "b_uniform")], ids=SC.name)
def test_base_probabilities_at_their_edges(cid):
    B, _, _ = SC.inputs(cid)
    assert set(np.unique(B)) == ({0.0, 1.0} if cid[1] == "b_onehot" else {1.0 / B.shape[2]})


def test_float32_cases_are_float32_and_referenced_from_the_widened_values():
    for cid in SC.F32_IDS:
        B, state, trans = SC.inputs(cid)
        assert B.dtype == np.float32
        p, _ = SC.marginals_longdouble(B.astype(np.float64), state, trans)
        assert np.array_equal(p, SC.reference(cid)[0])
