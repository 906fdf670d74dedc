"""CPU tests of the ancestry-specific LD layer: the restatement (tests/ld_exact.py) against a plain triple loop, LDCounts' r against
np.corrcoef, .pair and +, band_for, ld.clump against clump_literal, weights_from_assoc(index_of=), write_clumps' round trip, the ABI symbols
and the command line's refusals."""
import ctypes
import os

import numpy as np
import pytest

import ld_cases as LC
import ld_exact as LE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# |LDCounts.r() - np.corrcoef| over R_CASES, numpy against numpy on the CPU (the device has no part in it): the largest difference measured
# is 2.0e-15 (r from integer sufficient statistics with one division and one square root, corrcoef from centred float sums); 16 x that is
# allowed, because sqrt and the summation orders differ across numpy builds.
R_MEASURED = 1.9984014443252818e-15
R_TOL = 16 * R_MEASURED
R_CASES = ((65, 40, 5, 3, 12), (129, 33, 33, 2, 33), (5, 17, 1, 2, 17), (257, 24, 7, 7, 9))       # N, C, M, A, band


def _counts(X, lab, M, A, a, c0=0, c1=None, band=1):
    from gnomix_amd import ld
    t = LE.tables(X, lab, M, A, a, c0, c1, band)
    return ld.LDCounts(*(v.astype(np.int32) for v in t[:4]), c0, band)


@pytest.mark.parametrize("N,C,M,A,c0,c1,band", [(5, 9, 2, 3, 2, 8, 4), (7, 13, 13, 2, 0, 13, 15)])
def test_restatement_equals_the_triple_loop(N, C, M, A, c0, c1, band):
    M, W = LC.geometry(C, M)
    X, lab = LC.case(N, C, M, W, A, bad=1)
    asym = False
    for a in range(A):
        got = LE.tables(X, lab, M, A, a, c0, c1, band)
        want = LE.tables_loop(X, lab, M, A, a, c0, c1, band)
        for g, w in zip(got[:4], want):
            assert g.dtype == np.int64 and g.shape == (c1 - c0, band) and np.array_equal(g, w), a
        asym = asym or not np.array_equal(got[1], got[2])
    assert asym
    assert LE.n_bad(lab, M, A, C, 0, C, 1) == 1


def r_differences():
    """-> the largest |r - corrcoef| over R_CASES; asserts that NaN occurs exactly where corrcoef's inputs are empty or have no variance"""
    worst = 0.0
    n_nan = n_num = 0
    for N, C, M, A, band in R_CASES:
        M, W = LC.geometry(C, M)
        X = LC.linked(N, C, seed=N)
        X[:, C // 2] = np.where(X[:, C // 2] == 2, 2, 1)                # a SNP that is ALT wherever it is called: no variance
        lab = LC.case(N, C, M, W, A)[1]
        for a in range(A):
            o, d = LE.o_d(X, lab, M, a)
            r = _counts(X, lab, M, A, a, 0, C, band).r()
            assert r.dtype == np.float64 and r.shape == (C, band)
            for c in range(C):
                for k in range(band):
                    if c + k >= C:
                        assert np.isnan(r[c, k])
                        continue
                    both = (o[:, c] & o[:, c + k]).astype(bool)
                    x, y = d[both, c].astype(np.float64), d[both, c + k].astype(np.float64)
                    if x.size == 0 or x.min() == x.max() or y.min() == y.max():
                        assert np.isnan(r[c, k]), (N, a, c, k)
                        n_nan += 1
                    else:
                        assert np.isfinite(r[c, k]), (N, a, c, k)
                        worst = max(worst, abs(r[c, k] - np.corrcoef(x, y)[0, 1]))
                        n_num += 1
    assert n_nan > 50 and n_num > 1000
    return worst


def test_r_equals_corrcoef_and_is_nan_exactly_where_there_is_no_variance():
    worst = r_differences()
    print("largest |r - corrcoef| = %.3g (allowed %.3g)" % (worst, R_TOL))
    assert worst <= R_TOL


def test_r2_pair_symmetry_and_addition():
    from gnomix_amd import ld
    N, C, M, A, a, band = 65, 40, 5, 3, 1, 12
    M, W = LC.geometry(C, M)
    X, lab = LC.case(N, C, M, W, A)
    whole = _counts(X, lab, M, A, a, 0, C, band)
    r = whole.r()
    assert np.array_equal(np.isnan(whole.r2()), np.isnan(r)) and np.array_equal(whole.r2()[~np.isnan(r)], (r * r)[~np.isnan(r)])
    o, d = LE.o_d(X, lab, M, a)
    swapped = False
    for c, c2 in ((3, 9), (9, 3), (7, 7), (28, 39), (39, 28)):
        n11, n1o, no1, noo = whole.pair(c, c2)
        both = o[:, c] & o[:, c2]
        assert (n11, n1o, no1, noo) == (int((d[:, c] & d[:, c2]).sum()), int((d[:, c] & both).sum()), int((d[:, c2] & both).sum()), int(both.sum()))
        back = whole.pair(c2, c)
        assert back == (n11, no1, n1o, noo)
        swapped = swapped or n1o != no1
    assert swapped
    for bad in ((3, 3 + band), (C, C), (-1, 0)):
        with pytest.raises(IndexError):
            whole.pair(*bad)
    parts = _counts(X, lab, M, A, a, 0, 7, band) + _counts(X, lab, M, A, a, 7, 30, band) + _counts(X, lab, M, A, a, 30, C, band)
    assert isinstance(parts, ld.LDCounts) and parts.c0 == 0 and parts.band == band and parts.c1 == C
    assert all(np.array_equal(g, w) and g.dtype == np.int32 for g, w in zip(parts[:4], whole[:4]))
    with pytest.raises(ValueError):
        _counts(X, lab, M, A, a, 0, 7, band) + _counts(X, lab, M, A, a, 8, 30, band)
    with pytest.raises(ValueError):
        _counts(X, lab, M, A, a, 0, 7, band) + _counts(X, lab, M, A, a, 7, 30, band + 1)
    # products beyond int32: noo n11 at N = 2^20 haplotypes is exact in int64
    big = ld.LDCounts(*(np.array([[v]], np.int32) for v in (2 ** 19, 2 ** 19, 2 ** 19, 2 ** 20)), 0, 1)
    assert big.r()[0, 0] == 1.0


def test_band_for():
    from gnomix_amd import ld
    pos = np.array([100, 200, 1100, 1101, 1150, 5000, 9000])
    assert ld.band_for(pos, 1) == 4                       # 200 reaches 1100, 1101, 1150 (1200 would be the last)
    assert ld.band_for(pos, 0.05) == 3                    # 1100 reaches 1101 and 1150
    assert ld.band_for(pos, 0.9) == 3 and ld.band_for(pos, 0.0005) == 1 and ld.band_for(pos, 1000) == 7
    assert ld.band_for(np.array([5, 5, 5]), 0) == 3 and ld.band_for(np.array([], np.int64), 10) == 1
    dense = np.arange(ld.GNX_LD_MAX_BAND + 1)
    assert ld.band_for(dense[:-1], 1000) == ld.GNX_LD_MAX_BAND
    with pytest.raises(ValueError, match=str(ld.GNX_LD_MAX_BAND + 1)):
        ld.band_for(dense, 1000)


@pytest.mark.parametrize("seed,kb,tight", [(0, 3.0, False), (1, 1.2, True), (2, 0.5, True), (3, 3.0, False)])
def test_clump_equals_the_literal_loops(seed, kb, tight):
    from gnomix_amd import ld
    N, C, M, A, a = 129, 90, 8, 2, seed % 2
    M, W = LC.geometry(C, M)
    rng = np.random.RandomState(seed)
    X = LC.linked(N, C, seed=seed)
    X[:, 11] = 1                                                         # monomorphic: its r^2 is NaN, it joins nobody
    lab = LC.case(N, C, M, W, A)[1]
    pos = np.cumsum(rng.randint(20, 400, size=C))
    p = np.round(10.0 ** rng.uniform(-7, 0, size=C), 7 if seed else 3)     # seed 0: three decimals, many ties
    p[rng.choice(C, 6, replace=False)] = np.nan
    p[11], p[12], p[40], p[41] = 1e-6, 1e-6, 2e-5, 2e-5                  # ties in p among candidates; a candidate with a NaN r^2
    band = ld.band_for(pos, kb) + (20 if tight else 0)                   # tight: the kb limit bites before the band does
    full = LE.tables(X, lab, M, A, a, 0, C, band)[:4]
    asked = []

    def counts_for(c0, c1):
        asked.append((c0, c1))
        return ld.LDCounts(*(t[c0:c1].astype(np.int32) for t in full), c0, band)
    opts = dict(p1=1e-3, p2=5e-2, r2=0.3, kb=kb)
    got = ld.clump(p, pos, counts_for, **opts)
    want = LE.clump_literal(p, pos, full, band, **opts)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (got == np.arange(C)).sum() >= 3 and ((got >= 0) & (got != np.arange(C))).sum() >= 3 and (got == -1).any()
    assert got[11] == 11 and (got == 11).sum() == 1 and (got[np.isnan(p)] == -1).all() and np.isnan(p).sum() >= 2
    assert all(0 <= c0 < c1 <= C for c0, c1 in asked) and len(asked) <= (got == np.arange(C)).sum()
    if tight:       # a SNP inside the band and strongly linked, yet beyond kb, stays out
        r2 = ld.LDCounts(*(t.astype(np.int32) for t in full), 0, band).r2()
        far = [(c, k) for c in np.nonzero(got == np.arange(C))[0] for k in range(1, band) if c + k < C and pos[c + k] - pos[c] > kb * 1000
               and r2[c, k] >= 0.3 and p[c + k] <= 5e-2]
        assert all(got[c + k] != c for c, k in far)
    with pytest.raises(ValueError, match="band"):
        ld.clump(p, pos, lambda c0, c1: ld.LDCounts(*(t[c0:c1, :1].astype(np.int32) for t in full), c0, 1), **opts)
    assert np.array_equal(ld.clump(np.full(C, np.nan), pos, counts_for), np.full(C, -1))
    cache = ld.BlockCache(counts_for, C, block=32)
    assert np.array_equal(ld.clump(p, pos, cache, **opts), want) and len(cache.have) <= 3


def test_weights_from_assoc_takes_the_clumps():
    import collections
    from gnomix_amd import score
    Res = collections.namedtuple("Res", "beta p")
    beta = np.array([[0.5, -1.0], [np.nan, 2.0], [0.25, np.inf], [1.5, 3.0]])
    p = np.array([[1e-9, 0.2], [1e-9, 1e-5], [0.5, 1e-9], [np.nan, 1e-3]])
    res = Res(beta, p)
    before = np.where(np.isfinite(beta), beta, 0.0)
    assert np.array_equal(score.weights_from_assoc(res), before) and np.array_equal(score.weights_from_assoc(res, index_of=None), before)
    assert np.array_equal(score.weights_from_assoc(res, 1e-4), np.array([[0.5, 0.0], [0.0, 2.0], [0.0, 0.0], [0.0, 0.0]]))
    index_of = np.array([[0, -1], [0, 1], [-1, 1], [3, 3]], np.int64)
    assert np.array_equal(score.weights_from_assoc(res, index_of=index_of), np.array([[0.5, 0.0], [0.0, 2.0], [0.0, 0.0], [1.5, 3.0]]))
    assert np.array_equal(score.weights_from_assoc(res, 1e-4, index_of), np.array([[0.5, 0.0], [0.0, 2.0], [0.0, 0.0], [0.0, 0.0]]))
    with pytest.raises(ValueError, match="index_of"):
        score.weights_from_assoc(res, index_of=index_of[:, :1])


def test_write_clumps_round_trip(tmp_path):
    from gnomix_amd import postprocess as pp
    pos = np.array([11, 25, 30, 47, 52, 90])
    index_of = np.array([[0, -1], [0, 1], [-1, 1], [3, 5], [0, 5], [-1, 5]], np.int64)
    p = np.array([[1e-9, 0.5], [3e-3, 1e-300], [0.7, 2e-3], [1.25e-5, 1e-3], [1e-2, 1e-3], [np.nan, 0.1 + 0.2 - 0.3]])
    pp.write_clumps(str(tmp_path / "q"), "22", pos, index_of, p, ["AFR", "EUR"])
    lines = (tmp_path / "q.clumped.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["chm", "pos", "population", "p", "n_members", "members"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [(r[1], r[2]) for r in rows] == [("11", "AFR"), ("47", "AFR"), ("25", "EUR"), ("90", "EUR")]
    back = np.full(index_of.shape, -1, np.int64)
    where = {int(v): c for c, v in enumerate(pos)}
    for chm, ps, pop, pv, n, members in rows:
        c, a = where[int(ps)], ["AFR", "EUR"].index(pop)
        assert chm == "22" and float(pv) == p[c, a]                    # repr reads back to the same float64
        back[c, a] = c
        mem = [] if members == "." else [where[int(v)] for v in members.split(",")]
        assert len(mem) == int(n) and mem == sorted(mem)
        back[mem, a] = c
    assert np.array_equal(back, index_of)
    with pytest.raises(ValueError):
        pp.write_clumps(str(tmp_path / "bad"), "22", pos, index_of[:, :1], p, ["AFR", "EUR"])


def test_abi_symbols_are_built_and_declared():
    from gnomix_amd import _lib, ld
    lib = _lib.load()
    for name, n_args in (("gnx_ancestry_ld_counts", 22), ("gnx_ancestry_ld_counts_dev", 22), ("gnx_ancestry_ld_counts_gt2", 17)):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int and len(_lib.SYMBOLS[name][1]) == n_args
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16           # nothing existing changed
    hdr = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    for name in ("gnx_ancestry_ld_counts_dev(", "gnx_ancestry_ld_counts(", "gnx_ancestry_ld_counts_gt2(", "#define GNX_LD_MAX_BAND %d" % ld.GNX_LD_MAX_BAND):
        assert name in hdr
    assert _lib.GNX_LD_MAX_BAND == ld.GNX_LD_MAX_BAND
    from gnomix_amd.model import DeviceModel
    from gnomix_amd.gnomix import HipGnomix
    for name in ("ancestry_ld_counts", "ancestry_ld_counts_device", "ancestry_ld_counts_gt2"):
        assert callable(getattr(DeviceModel, name))
    assert callable(HipGnomix.ancestry_ld) and callable(HipGnomix.ancestry_clump)


def test_run_inference_refuses_the_key_with_phase_before_any_work(tmp_path):
    from gnomix_amd import cli
    args = {"query_file": str(tmp_path / "none.vcf"), "chm": "22", "output_basename": str(tmp_path), "phase": True}
    with pytest.raises(ValueError, match="ancestry_clump_output with phase=True"):
        cli.run_inference(args, None, ancestry_clump_output=True, ancestry_assoc_output=True, phenotype_file="none.tsv")
    with pytest.raises(ValueError, match="ancestry_clump_output needs inference.ancestry_assoc_output"):
        cli.run_inference(dict(args, phase=False), None, ancestry_clump_output=True)
    assert os.listdir(str(tmp_path)) == []
