"""CPU tests of the ancestry-specific pair counts and MDS: the restatement (tests/pairs_exact.py) against a plain triple loop and
against direct haplotype-pair counting, asmds.select's rule, PairCounts' addition, classical_mds, write_asmds' bytes, the ABI symbols
and the command line's refusal."""
import ctypes
import os

import numpy as np
import pytest

import pairs_cases as PC
import pairs_exact as PE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,C,M,A", [(2, 1, 1, 1), (6, 7, 2, 3), (8, 13, 5, 2), (4, 9, 9, 3), (6, 10, 1, 4)])
def test_restatement_equals_the_triple_loop(N, C, M, A):
    M, W = PC.geometry(C, M)
    X, lab = PC.case(N, C, M, W, A, bad=1 if N > 2 else 0)
    for a in range(A):
        for c0, c1 in ((0, C), (C // 3, max(C // 3 + 1, C - 1))):
            got = PE.tables(X, lab, M, A, a, c0, c1)
            want = PE.tables_loop(X, lab, M, A, a, c0, c1)
            for g, w in zip(got[:3], want):
                assert g.dtype == np.int64 and np.array_equal(g, w), (a, c0, c1)
    assert PE.tables(X, lab, M, A, 0)[3] == (1 if N > 2 else 0)


def test_mismatches_and_comparisons_are_the_haplotype_pair_counts():
    from gnomix_amd import asmds
    C, M, A = 41, 6, 3
    M, W = PC.geometry(C, M)
    X, lab = PC.case(10, C, M, W, A, seed=4)
    for a in range(A):
        DD, DO, OO, _ = PE.tables(X, lab, M, A, a)
        pc = asmds.PairCounts(DD.astype(np.int32), DO.astype(np.int32), OO.astype(np.int32))
        mism, comp = PE.hap_pair_counts(X, lab, M, a)
        assert np.array_equal(pc.mismatches(), mism) and np.array_equal(pc.comparisons(), comp)
        assert pc.mismatches().dtype == np.int64 and not np.array_equal(DO, DO.T)
        delta = pc.distances(min_sites=5)
        assert delta.dtype == np.float64 and (np.diagonal(delta) == 0).all()
        off = ~np.eye(5, dtype=bool)
        assert np.array_equal(np.isnan(delta) & off, (comp < 5) & off)
        ok = (comp >= 5) & off
        assert np.array_equal(delta[ok], mism[ok] / comp[ok])


def _counts(OO):
    from gnomix_amd import asmds
    OO = np.asarray(OO, np.int32)
    z = np.zeros_like(OO)
    return asmds.PairCounts(z, z, OO)


def test_select_rule_and_tie_breaks():
    from gnomix_amd import asmds
    big = 100
    OO = np.full((5, 5), big)
    assert list(asmds.select(_counts(OO), 10, 10)) == [0, 1, 2, 3, 4]
    # step 1: the diagonal alone decides
    OO1 = OO.copy()
    OO1[2, 2] = 9
    OO1[2, :2] = OO1[:2, 2] = 0            # pairs of an individual that is not kept do not count
    assert list(asmds.select(_counts(OO1), 10, 10)) == [0, 1, 3, 4]
    # step 2: individual 1 has two short pairs, 0 and 3 one each: dropping 1 settles it
    OO2 = OO.copy()
    OO2[1, 0] = OO2[0, 1] = OO2[1, 3] = OO2[3, 1] = 3
    assert list(asmds.select(_counts(OO2), 10, 10)) == [0, 2, 3, 4]
    # one short pair (0, 4), one each: the smaller OO[i, i] goes
    OO3 = OO.copy()
    OO3[0, 4] = OO3[4, 0] = 3
    OO3[0, 0] = 50
    assert list(asmds.select(_counts(OO3), 10, 10)) == [1, 2, 3, 4]
    OO3[0, 0], OO3[4, 4] = big, 50
    assert list(asmds.select(_counts(OO3), 10, 10)) == [0, 1, 2, 3]
    # the same diagonal too: the larger index goes
    OO3[4, 4] = big
    assert list(asmds.select(_counts(OO3), 10, 10)) == [0, 1, 2, 3]
    # a chain 0-1, 1-2, 2-3 of short pairs: 1 and 2 have two each, equal diagonals -> 2 goes, then (0, 1) remains -> 1 goes
    OO4 = OO.copy()
    for i, j in ((0, 1), (1, 2), (2, 3)):
        OO4[i, j] = OO4[j, i] = 0
    assert list(asmds.select(_counts(OO4), 10, 10)) == [0, 3, 4]
    assert asmds.select(_counts(np.zeros((3, 3))), 1, 1).size == 0 and asmds.select(_counts(np.zeros((0, 0))), 1, 1).size == 0


def test_pair_counts_add_in_int64_and_refuse_overflow():
    from gnomix_amd import asmds
    rng = np.random.RandomState(0)
    a = asmds.PairCounts(*(rng.randint(0, 1000, size=(4, 4)).astype(np.int32) for _ in range(3)))
    b = asmds.PairCounts(*(rng.randint(0, 1000, size=(4, 4)).astype(np.int32) for _ in range(3)))
    s = a + b
    assert isinstance(s, asmds.PairCounts) and all(t.dtype == np.int32 for t in s)
    assert all(np.array_equal(t, x + y) for t, x, y in zip(s, a, b))
    top = np.full((4, 4), 2 ** 31 - 1, np.int32)
    one = np.zeros((4, 4), np.int32)
    one[1, 2] = 1
    with pytest.raises(OverflowError):
        asmds.PairCounts(top, top, top) + asmds.PairCounts(one, one, one)
    half = np.full((4, 4), 2 ** 30, np.int32)
    edge = asmds.PairCounts(half, half, half) + asmds.PairCounts(half - 1, half - 1, half - 1)      # 2^31 - 1: still int32
    assert (edge.DD == 2 ** 31 - 1).all()
    with pytest.raises(ValueError):
        a + asmds.PairCounts(*(np.zeros((3, 3), np.int32),) * 3)


# classical_mds on points in R^3: the LARGEST error of the checks below, measured on the CPU this file was written on (numpy with
# OpenBLAS LAPACK), was 1.6e-14 for the distances (absolute; coordinates of standard deviation 3, 1.5 and 0.5; n = 150) and 3.5e-16 for
# |lambda_4| / lambda_1 (n = 40).  LAPACK builds differ in eigh, so 16 x the measured value is allowed: MDS_DIST_TOL and MDS_EIG_TOL.
# (DESIGN.md 4.21 records the same numbers.)
MDS_MEASURED_DIST, MDS_MEASURED_EIG, MDS_FACTOR = 1.6e-14, 3.5e-16, 16
MDS_DIST_TOL, MDS_EIG_TOL = MDS_FACTOR * MDS_MEASURED_DIST, MDS_FACTOR * MDS_MEASURED_EIG


def mds_errors(n, seed):
    """-> (largest |recovered distance - given distance|, |lambda_4| / lambda_1) of classical_mds on n points drawn in R^3"""
    from gnomix_amd import asmds
    P = np.random.RandomState(seed).normal(size=(n, 3)) * np.array([3.0, 1.5, 0.5])
    delta = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    res = asmds.classical_mds(delta, 3)
    assert res.coords.shape == (n, 3) and res.kept is None
    back = np.sqrt(((res.coords[:, None, :] - res.coords[None, :, :]) ** 2).sum(-1))
    four = asmds.classical_mds(delta + 0.0, 3)
    assert np.array_equal(four.coords, res.coords)
    D2 = delta * delta
    J = np.eye(n) - 1.0 / n
    lam = np.linalg.eigvalsh(-0.5 * J @ D2 @ J)[::-1]
    assert np.all(np.diff(res.eigenvalues) <= 0) and abs(res.explained.sum() - 1) < 1e-9
    for q in range(3):                                     # the sign rule
        assert res.coords[int(np.argmax(np.abs(res.coords[:, q]))), q] > 0
    return float(np.abs(back - delta).max()), float(abs(lam[3]) / lam[0])


@pytest.mark.parametrize("n,seed", [(5, 0), (12, 1), (40, 2), (150, 3)])
def test_classical_mds_recovers_points_in_r3(n, seed):
    dist_err, eig = mds_errors(n, seed)
    print("classical_mds n=%d: distance error %.3g, |lambda_4| / lambda_1 %.3g" % (n, dist_err, eig))
    assert dist_err <= MDS_DIST_TOL and eig <= MDS_EIG_TOL


def test_classical_mds_refusals_and_no_individual_dropped():
    from gnomix_amd import asmds
    P = np.random.RandomState(5).normal(size=(6, 2))
    delta = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    with pytest.raises(ValueError, match="positive eigenvalues"):
        asmds.classical_mds(delta, 4)                      # points of a plane have two
    with pytest.raises(ValueError):
        asmds.classical_mds(delta, 7)
    bad = delta.copy()
    bad[0, 1] = bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        asmds.classical_mds(bad, 2)
    # through ancestry_mds: tables whose every pair has sites enough keep everyone, so the comparison above hides nothing
    OO = np.full((6, 6), 1000, np.int32)
    DO = np.full((6, 6), 500, np.int32)
    DD = (500 - np.rint(250 * delta)).astype(np.int32)     # mism = 2 * 500 - 2 DD = 500 delta (rounded)
    res = asmds.ancestry_mds(asmds.PairCounts(DD, DO, OO), k=2, min_sites=100)
    assert list(res.kept) == list(range(6)) and (res.n_sites == 1000).all()
    back = np.sqrt(((res.coords[:, None, :] - res.coords[None, :, :]) ** 2).sum(-1))
    assert np.abs(back - 0.5 * delta).max() < 2e-3         # the rounding of DD to integers: 1 / 1000 per distance
    assert asmds.ancestry_mds(asmds.PairCounts(DD, DO, OO), k=2, min_sites=2000) is None
    assert asmds.ancestry_mds(asmds.PairCounts(DD[:2, :2], DO[:2, :2], OO[:2, :2]), k=2, min_sites=1) is None   # fewer than k + 1


def test_write_asmds_round_trip(tmp_path):
    from gnomix_amd import asmds
    from gnomix_amd import postprocess as pp
    coords = np.array([[0.1, -2.0], [1 / 3, 1e-300], [2.0 ** -60, 5.0]])
    r0 = asmds.AncestryMDS(coords, np.array([2.0, 1.0]), np.array([0.6, 0.3]), np.array([0, 2, 3]), np.array([11, 12, 13]))
    pp.write_asmds(str(tmp_path / "q"), [r0, None], ["AFR", "EUR"], ["s0", "s1", "s2", "s3"])
    lines = (tmp_path / "q.asmds.tsv").read_text().splitlines()
    head = "sample\tpopulation\tn_sites\tkept\tPC1\tPC2"
    assert lines[0] == head and lines[5] == head and len(lines) == 6          # EUR: the header line and no rows
    assert lines[2] == "s1\tAFR\tNA\t0\tNA\tNA"
    rows = [ln.split("\t") for ln in lines[1:5]]
    assert [r[0] for r in rows] == ["s0", "s1", "s2", "s3"] and [r[3] for r in rows] == ["1", "0", "1", "1"]
    back = np.array([[float(v) for v in r[4:]] for r in rows if r[3] == "1"])
    assert np.array_equal(back, coords) and [r[2] for r in rows] == ["11", "NA", "12", "13"]
    with pytest.raises(ValueError):
        pp.write_asmds(str(tmp_path / "bad"), [r0], ["AFR", "EUR"], ["s0", "s1", "s2", "s3"])


def test_abi_symbols_are_built_and_declared():
    from gnomix_amd import _lib
    lib = _lib.load()
    for name, n_args in (("gnx_ancestry_pair_counts", 20), ("gnx_ancestry_pair_counts_dev", 20), ("gnx_ancestry_pair_counts_gt2", 15)):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int and len(_lib.SYMBOLS[name][1]) == n_args
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16
    hdr = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    for name in ("gnx_ancestry_pair_counts_dev(", "gnx_ancestry_pair_counts(", "gnx_ancestry_pair_counts_gt2(", "NOT gnx_ancestry_dosage's hapcount"):
        assert name in hdr
    from gnomix_amd.model import DeviceModel
    from gnomix_amd.gnomix import HipGnomix
    for name in ("ancestry_pair_counts", "ancestry_pair_counts_device", "ancestry_pair_counts_gt2"):
        assert callable(getattr(DeviceModel, name))
    assert callable(HipGnomix.ancestry_pair_counts) and callable(HipGnomix.ancestry_mds)


def test_run_inference_refuses_the_key_with_phase_before_any_work(tmp_path):
    from gnomix_amd import cli
    args = {"query_file": str(tmp_path / "none.vcf"), "chm": "22", "output_basename": str(tmp_path), "phase": True}
    with pytest.raises(ValueError, match="ancestry_mds_output with phase=True"):
        cli.run_inference(args, None, ancestry_mds_output=True)
    with pytest.raises(ValueError, match="must be >= 1"):
        cli.run_inference(dict(args, phase=False), None, ancestry_mds_output=True, ancestry_mds_components=0)
    assert os.listdir(str(tmp_path)) == []
