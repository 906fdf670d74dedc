"""The tree bases (csrc/k_base_forest2.hip, csrc/k_base_forest.hip) where the parity tests do not reach: runs of windows per block,
a ring that changes between the main and the last launch, depths 1 .. 8, tree counts around the batch loops, split edges.

tests/test_gpu_parity.py holds both kernels to the oracle at eleven shapes, every one of which the launchers run with one window per
block.  Here the run length is forced (GNX_FOREST_WRUN, one context per value: the knobs are read once per context) on the cases of
tests/forest_cases.py, whose models put splits on every window edge, word boundary and padding seam, and whose claims about the
paths they reach tests/test_forest_cases_host.py asserts on the CPU.  For every case, kernel and run length:
  random forest   b64 bit-equal to the oracle and to the numpy reference, b32 its float32 cast;
  boosted trees   b32 within the project's float32 bar of the oracle (_close_f32 of tests/test_gpu_parity.py: 2.4e-7, at most
                  max(3, size / 20) unequal cells) and of the numpy reference, b64 its float64 cast;
  run invariance  every run length gives the bits of run length 1: a run changes what is staged when, never the order of a sum;
  labels          the arg-max is the reference's wherever the reference's top two differ by more than the bar."""
import numpy as np
import pytest

import forest_cases as FC

pytestmark = pytest.mark.gpu

KNOBS = ("GNX_FOREST_IMPL", "GNX_FOREST_WRUN", "GNX_FOREST_H", "GNX_FOREST_T", "GNX_FOREST_FLAGS")
IMPLS = {"forest2": "0", "forest1": "1"}


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _new_context(**knobs):
    from gnomix_amd import _lib
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in knobs.items():
            mp.setenv(k, str(v))
        return _lib.Context(0)          # the knobs are read here, once


def _predict(ga, data, X, **knobs):
    """one context at a time: made for the launch, closed after it"""
    ctx = _new_context(**knobs)
    try:
        return ga.DeviceModel(data, ctx=ctx).base_predict(X, want_f32=True, want_f64=True)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def oracle_of(oracle):
    """case name -> the oracle's output, computed once for both kernels"""
    made = {}

    def get(case):
        if case.name not in made:
            made[case.name] = FC.oracle_output(oracle, case)
            made[case.name].setflags(write=False)
        return made[case.name]
    return get


def _check(case, b32, b64, ora, what):
    ref = FC.reference(case.name)
    if case.rf:
        assert np.array_equal(b64, ora), what
        assert np.array_equal(b64, ref), what
        assert np.array_equal(b32, ora.astype(np.float32)), what
    else:
        print("%s %s: %d of %d cells differ from the oracle, %d from the reference, max |diff| %.3g / %.3g"
              % (case.name, what, np.count_nonzero(b32 != ora), b32.size, np.count_nonzero(b32 != ref),
                 np.max(np.abs(b32 - ora)), np.max(np.abs(b32 - ref))))
        FC.close_f32(b32, ora)
        FC.close_f32(b32, ref)
        assert np.array_equal(b64, b32.astype(np.float64)), what
    top = np.sort(ref, axis=-1)
    sure = top[..., -1] - top[..., -2] > FC.TOL
    assert np.array_equal(np.argmax(b32, -1)[sure], np.argmax(ref, -1)[sure]), what
    assert np.array_equal(np.argmax(b64, -1)[sure], np.argmax(ref, -1)[sure]), what
    assert sure.mean() > 0.9


@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("case", FC.CASES, ids=[c.name for c in FC.CASES])
def test_forest_case(ga, oracle_of, case, impl):
    data, X, ora = FC.model_data(ga, case), FC.inputs(case.name), oracle_of(case)
    # longest runs first: a ring slot that a run fails to refresh then holds what an earlier launch left in the LDS, not the very word
    # a launch with one window per block has just staged there for the same haplotypes
    got = {}
    for wrun in sorted(case.run_lengths(), reverse=True):
        got[wrun] = _predict(ga, data, X, GNX_FOREST_IMPL=IMPLS[impl], GNX_FOREST_WRUN=wrun)
        _check(case, got[wrun][0], got[wrun][1], ora, "%s wrun=%d" % (impl, wrun))
    for wrun, (b32, b64) in got.items():
        assert np.array_equal(b32, got[1][0]) and np.array_equal(b64, got[1][1]), "run length %d changed the output" % wrun


def test_forest1_wave_groups(ga, oracle_of):
    """k_base_forest with two wave groups per tile (the default for more than two classes) and with one (GNX_FOREST_H=1), in runs:
    the groups split the classes, so the bits are the same"""
    case = FC.BY_NAME[FC.HALVES_CASE]
    data, X, ora = FC.model_data(ga, case), FC.inputs(case.name), oracle_of(case)
    base = _predict(ga, data, X, GNX_FOREST_IMPL=1, GNX_FOREST_WRUN=1)
    for h in (0, 1):
        b32, b64 = _predict(ga, data, X, GNX_FOREST_IMPL=1, GNX_FOREST_WRUN=3, GNX_FOREST_H=h)
        _check(case, b32, b64, ora, "forest1 wrun=3 H=%d" % h)
        assert np.array_equal(b32, base[0]) and np.array_equal(b64, base[1]), h


def test_both_kernels_give_the_same_bits(ga):
    """the two kernels add the same leaves in the same order: one case of each base, in runs"""
    for name in ("x-ringchg", "r-deepctx"):
        case = FC.BY_NAME[name]
        data, X = FC.model_data(ga, case), FC.inputs(name)
        a = _predict(ga, data, X, GNX_FOREST_IMPL=0, GNX_FOREST_WRUN=3)
        b = _predict(ga, data, X, GNX_FOREST_IMPL=1, GNX_FOREST_WRUN=3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
