"""CPU side of the CRF trainer's edge tests (tests/test_gpu_train_crf_edges.py): what those tests take for granted about their
own inputs and about the oracle, checked without a device.
  - tests/crf_cases.py's generator is tests/test_train_crf.py's wherever that one is defined and N >= 2 A;
  - the direction check can fail: on every case with A > 2 a transposed state block, a transposed transition block and exchanged
    halves each move the oracle's unit gradient by > 1e-3 (the bar on the device is ~1e-9);
  - W = 1 has no edge: the oracle's g_trans is 2 c2 trans exactly;
  - the oracle is finite on the far-weight cases, and its own error there — against a longdouble restatement of its recursion —
    is a quarter of the bars at most, so the bars (1e-10 |f|, 1e-9 |g|) need no widening."""
import numpy as np
import pytest

import crf_cases as CC


def _points():
    """every (case id, B, y, state0, trans0, c2) the GPU tests evaluate away from zero weights"""
    for (N, W, A) in CC.GRID:
        B, y, st0, tr0 = CC.case(N, W, A)
        yield (N, W, A, "grid"), B, y, st0, tr0, 1.0
    for (N, W, A) in CC.F32_CASES:
        B, y, st0, tr0 = CC.case(N, W, A, dtype=np.float32)
        yield (N, W, A, "f32"), B, y, st0, tr0, 1.0
    for (N, W, A) in CC.LABEL_CASES:
        for kind in CC.LABEL_KINDS:
            B, y, st0, tr0 = CC.case(N, W, A, kind=kind)
            yield (N, W, A, kind), B, y, st0, tr0, 1.0
    for (N, W, A) in CC.C2_CASES:
        for c2 in CC.C2S:
            B, y, st0, tr0 = CC.case(N, W, A)
            yield (N, W, A, c2), B, y, st0, tr0, c2
    for (N, W, A) in CC.FAR_CASES:
        for s in CC.FAR_SCALES:
            B, y, _, _ = CC.case(N, W, A)
            st0, tr0 = CC.far_start(N, W, A, s)
            yield (N, W, A, "far", s), B, y, st0, tr0, 1e-6


def test_generator_is_the_existing_one_where_that_is_defined():
    from test_train_crf import _tracts
    for (N, W, A) in [(40, 30, 4), (9, 5, 2), (65, 4, 17), (33, 4, 5)]:
        B0, y0 = _tracts(np.random.RandomState(5), N, W, A)
        B1, y1 = CC.tracts(np.random.RandomState(5), N, W, A)
        assert np.array_equal(y0, y1) and np.array_equal(B0, B1)
    B, y = CC.tracts(np.random.RandomState(5), 9, 7, 16)             # fewer sequences than labels: _tracts cannot build these
    assert B.shape == (9, 7, 16) and np.any(y[:, 1:] != y[:, :-1]) and np.allclose(B.sum(-1), 1.0, rtol=0, atol=1e-15)


def test_every_kernel_instantiation_is_on_the_grid():
    assert {CC.kp(A) for (_, _, A) in CC.GRID} == {1, 4, 16}
    assert [CC.kp(A) for A in (2, 8, 9, 16, 17, 32)] == [1, 1, 4, 4, 16, 16]
    assert {A for (_, _, A) in CC.KP_CASES} >= {8, 9, 16, 17, 32}


def test_indexing_slips_move_the_direction_on_every_case(oracle):
    seen = 0
    for cid, B, y, st0, tr0, c2 in _points():
        A = B.shape[2]
        if A <= 2:
            continue
        _, gs, gt = oracle.crf_objective(B, y, st0, tr0, c2)
        v = CC.unit(gs, gt)
        for name, m in CC.mutations(gs, gt).items():
            assert np.max(np.abs(m - v)) > 1e-3, (cid, name)
        # at zero weights the state block and the halves are told apart as well (g_trans there is symmetric wherever every
        # sequence keeps its label or W = 1: its transposition is seen from the N(0, 0.5) start above)
        _, gs, gt = oracle.crf_objective(B, y, np.zeros((A, A)), np.zeros((A, A)), c2)
        v, m = CC.unit(gs, gt), CC.mutations(gs, gt)
        assert np.max(np.abs(m["state_transposed"] - v)) > 1e-3 and np.max(np.abs(m["halves_swapped"] - v)) > 1e-3, cid
        seen += 1
    assert seen >= len(CC.GRID) - 1


@pytest.mark.parametrize("N,W,A", [c for c in CC.GRID if c[1] == 1])
def test_a_single_window_has_no_edge_term(oracle, N, W, A):
    B, y, st0, tr0 = CC.case(N, W, A)
    for c2 in (1.0, 0.01):
        _, _, gt = oracle.crf_objective(B, y, st0, tr0, c2)
        assert np.array_equal(gt, 2.0 * c2 * tr0)


@pytest.mark.parametrize("s", CC.FAR_SCALES)
@pytest.mark.parametrize("N,W,A", CC.FAR_CASES)
def test_oracle_is_finite_and_accurate_far_from_zero(oracle, N, W, A, s):
    B, y, _, _ = CC.case(N, W, A)
    st0, tr0 = CC.far_start(N, W, A, s)
    f, gs, gt = oracle.crf_objective(B, y, st0, tr0, 1e-6)
    assert np.isfinite(f) and np.all(np.isfinite(gs)) and np.all(np.isfinite(gt))
    fl, gsl, gtl = CC.crf_objective_longdouble(B, y, st0, tr0, 1e-6)
    gn, gnl = np.sqrt(np.sum(gs * gs) + np.sum(gt * gt)), np.sqrt(np.sum(gsl * gsl) + np.sum(gtl * gtl))
    ef, eg, ev = float(abs(f - fl) / abs(fl)), float(abs(gn - gnl) / gnl), float(np.max(np.abs(CC.unit(gs, gt) - CC.unit(gsl, gtl))))
    print("oracle vs longdouble: f %.3g, |g| %.3g, direction %.3g" % (ef, eg, ev))
    # measured: f 5e-16 .. 2e-15, |g| 9e-13 .. 1.2e-11, direction 3e-13 .. 6e-12 (largest at (7, 400, 5), s = 20)
    assert 4 * ef <= 1e-10 and 4 * eg <= 1e-9 and 4 * ev <= 1e-9


def test_longdouble_restatement_is_the_oracles_function(oracle):
    B, y, st0, tr0 = CC.case(9, 7, 9)
    f, gs, gt = oracle.crf_objective(B, y, st0, tr0, 0.01)
    fl, gsl, gtl = CC.crf_objective_longdouble(B, y, st0, tr0, 0.01)
    assert abs(f - float(fl)) <= 1e-14 * abs(f)
    assert np.max(np.abs(gs - gsl.astype(np.float64))) <= 1e-13 and np.max(np.abs(gt - gtl.astype(np.float64))) <= 1e-13
