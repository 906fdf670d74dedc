"""CPU tests (-m "not gpu") of the many-trait ancestry-specific association: the host finish (gnomix_amd.assoc.finish_traits) fed the
restatement's math.fsum blocks (tests/assoc_traits_exact.py, tests/assoc_exact.py) against numpy.linalg.lstsq per trait, the shared
integer fields, T = 1 against the single-trait finish, the trait / covariate file readers, the max_bytes refusal and the ABI symbols.

TOLERANCE: tests/assoc_cases.py's, per SNP and trait: |got - want| <= C_TOL p kappa^2 2^-53 max_a |beta_want| with C_TOL = 400.
Measured here (the largest ratio err / (p kappa^2 2^-53 max|beta|) over A = 2, 3, 7 and the three traits): 42.8 (A = 2, trait 1; trait 0
gives 20.8 there, under this test's smaller set of participants), 5.5 at A = 3, 0.85 at A = 7."""
import ctypes
import os

import numpy as np
import pytest

import assoc_cases as AC
import assoc_exact as XE
import assoc_traits_cases as TC
import assoc_traits_exact as TE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_blocks = {}


def _stats(X, lab, M, A, Y, Z, use, slow=True):
    """-> assoc.AssocStats (the trait-independent blocks: a zero phenotype under the traits' participation) and assoc.TraitStats, both
    from math.fsum sums"""
    from gnomix_amd import assoc
    C, W, K, T = X.shape[1], lab.shape[1], Z.shape[1], Y.shape[1]
    use2 = TE.base_participation(Y, Z, use).astype(np.uint8)
    b = (XE.blocks_slow if slow else XE.blocks)(X, lab, M, A, np.zeros(len(Y)), Z, use2, 0, C)
    st = assoc.split_blocks(b[0], b[1], b[2], b[3], A, K, 0, C, M, W, b[4])
    sy, wy, wyy, n_bad = TE.blocks(X, lab, M, A, Y, Z, use, 0, C)
    return st, assoc.split_traits(sy, wy, wyy, T, 0, C, M, W, n_bad)


def _regression(A):
    if A not in _blocks:
        X, lab, Y, Z, use = TC.regression_traits(A)
        _blocks[A] = _stats(X, lab, AC.M, A, Y, Z, use)
    return _blocks[A]


@pytest.mark.parametrize("A", [2, 3, 7])
def test_finish_traits_against_lstsq_per_trait(A):
    from gnomix_amd import assoc
    X, lab, Y, Z, use = TC.regression_traits(A)
    st, ts = _regression(A)
    beta, se, t, n_alt, n_hap, n, df, n_miss, status = assoc.finish_traits(st, ts, A, AC.K)
    assert beta.shape == se.shape == t.shape == (AC.C, A, 3) and status.shape == (AC.C,)
    want = TE.fit(X, lab, AC.M, A, Y, Z, use)
    assert (n == AC.N_IND - 3).all()                      # two use zeros and the NaN of trait 1: complete cases across the traits
    worst = 0.0
    for k, w in enumerate(want):
        for g, name in ((n_alt, "n_alt"), (n_hap, "n_hap"), (n, "n"), (df, "df"), (n_miss, "n_miss"), (status, "status")):
            assert g.dtype == np.int32 and np.array_equal(g, w[name]), (name, k)
        r, left_out = AC.ratios(beta[:, :, k], se[:, :, k], t[:, :, k], w)
        print("A = %d trait %d: ratio %.4g, SNPs left out %.3f" % (A, k, r, left_out))
        assert left_out < 0.05
        worst = max(worst, r)
    assert worst <= AC.C_TOL
    p = assoc.p_values_traits(t, df)
    assert p.shape == t.shape and np.array_equal(np.isnan(p), np.isnan(t)) and np.nanmax(p) <= 1 and np.nanmin(p) >= 0
    assert np.array_equal(p[:, :, 1], assoc.p_values(t[:, :, 1], df), equal_nan=True)


def test_one_trait_agrees_with_the_single_trait_finish():
    from gnomix_amd import assoc
    A = 3
    X, lab, y, Z, use = AC.regression_case(A)
    Y = y[:, None]
    st0, ts = _stats(X, lab, AC.M, A, Y, Z, use)
    b = XE.blocks_slow(X, lab, AC.M, A, y, Z, use, 0, AC.C)
    st = assoc.split_blocks(b[0], b[1], b[2], b[3], A, AC.K, 0, AC.C, AC.M, AC.W, b[4])
    for name in ("dtz", "dtd", "dth", "sum_d", "n_miss", "n", "sum_h"):          # T = 1: exactly the single-trait participation
        assert np.array_equal(getattr(st0, name), getattr(st, name)), name
    P = AC.K + A - 1
    assert np.array_equal(st0.gram[:, :P, :P], st.gram[:, :P, :P])
    one = assoc.finish(st, A, AC.K)
    many = assoc.finish_traits(st0, ts, A, AC.K)
    for a, b in zip(one[3:], many[3:]):
        assert np.array_equal(a, b)
    want = AC.regression_fit(A)
    ok = (want["status"] == 0) & (want["kappa"] <= AC.KAPPA_MAX)
    scale = want["p_kept"][ok] * want["kappa"][ok] ** 2 * 2.0 ** -53 * np.nanmax(np.abs(want["beta"][ok]), axis=1)
    for a, b in zip(one[:3], many[:3]):
        assert np.array_equal(np.isnan(a), np.isnan(b[:, :, 0]))
        assert (np.nanmax(np.abs(a[ok] - b[ok][:, :, 0]), axis=1) <= AC.C_TOL * scale).all()


@pytest.mark.parametrize("n_ind,T,A,K", TC.GRID[:4])
def test_column_rule_and_statuses_of_the_small_cases(n_ind, T, A, K):
    """the integer fields and the status are shared by all traits and equal the restatement's; status 2 where df < 1 (window 1), status 1
    where nobody carries ancestry A - 1 (window 2) wherever df >= 1"""
    from gnomix_amd import assoc
    X, lab, Y, Z, use = TC.small_case(n_ind, T, A, K)
    st, ts = _stats(X, lab, TC.M, A, Y, Z, use)
    assert ts.n_bad == n_ind - 1
    got = assoc.finish_traits(st, ts, A, K, TC.MIN_AC)
    want = TE.fit(X, lab, TC.M, A, Y, Z, use, min_ac=TC.MIN_AC)
    for w in want:
        for g, name in zip(got[3:], ("n_alt", "n_hap", "n", "df", "n_miss", "status")):
            assert np.array_equal(g, w[name]), name
    status, df = got[8], got[6]
    assert (status[8:16] == 2).all() and (df[8:16] < 1).all()
    assert ((status[16:24] == 1) | (df[16:24] < 1)).all()
    assert np.isnan(got[0][status != 0]).all() and np.isnan(got[0][5]).all() and np.isnan(got[0][6]).all()
    for k, w in enumerate(want):
        assert np.array_equal(np.isnan(got[0][:, :, k]), np.isnan(w["beta"]))


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_trait_and_covariate_file_readers(tmp_path):
    from gnomix_amd import assoc
    samples = ["s0", "s1", "s2", "s3"]
    tf = _write(tmp_path / "traits.tsv", "sample\theight\tbmi\ns0\t1.5\t2\ns2\tNA\t3.25\nnobody\t9\t9\ns3\t4\t.\n")
    cf = _write(tmp_path / "cov.tsv", "sample\tage\ns0\t30\ns1\t41\ns2\t52\n")
    Y, Z, use, names, cov = assoc.read_traits(tf, samples)
    assert names == ["height", "bmi"] and cov == ["intercept"] and Z.shape == (4, 1) and (Z == 1).all()
    assert use.dtype == np.uint8 and use.tolist() == [1, 0, 1, 1]                       # s1 is absent from the file
    assert Y[0].tolist() == [1.5, 2.0] and np.isnan(Y[1]).all() and np.isnan(Y[2, 0]) and Y[2, 1] == 3.25 and np.isnan(Y[3, 1])
    Y2, Z2, use2, _, cov2 = assoc.read_traits(tf, samples, cf)
    assert cov2 == ["intercept", "age"] and np.array_equal(Y2, Y, equal_nan=True)
    assert use2.tolist() == [1, 0, 1, 0] and Z2[:3, 1].tolist() == [30.0, 41.0, 52.0] and np.isnan(Z2[3, 1]) and (Z2[:, 0] == 1).all()
    # complete cases: s2 (an NA trait) and s3 (an NA trait, no covariates) take no part
    _, _, _, part = assoc.trait_covariates(4, Y2, Z2, use2)
    assert part.tolist() == [1, 0, 0, 0]
    dup = _write(tmp_path / "dup.tsv", "sample\th\ns0\t1\ns0\t2\n")
    with pytest.raises(ValueError, match="listed twice"):
        assoc.read_traits(dup, samples)
    with pytest.raises(ValueError, match="listed twice"):
        assoc.read_traits(tf, samples, _write(tmp_path / "dupc.tsv", "sample\tage\ns1\t1\ns1\t2\n"))
    with pytest.raises(ValueError, match="header"):
        assoc.read_traits(_write(tmp_path / "bad.tsv", "id\th\ns0\t1\n"), samples)
    with pytest.raises(ValueError, match="not a number"):
        assoc.read_traits(_write(tmp_path / "bad2.tsv", "sample\th\ns0\tx\n"), samples)
    with pytest.raises(ValueError, match="cells"):
        assoc.read_traits(_write(tmp_path / "bad3.tsv", "sample\th\tb\ns0\t1\n"), samples)


def test_max_bytes_refusal_names_the_byte_count():
    from gnomix_amd import assoc
    C, A, T = 317408, 7, 1024
    need = assoc.traits_result_bytes(C, A, T)
    assert need > 4 * C * A * T * 8

    def never():
        raise AssertionError("no chunk may be computed")
        yield
    with pytest.raises(ValueError, match=str(need)):
        assoc.traits_concat(never(), C, A, T)
    with pytest.raises(ValueError, match=str(assoc.traits_result_bytes(100, 2, 3))):
        assoc.traits_concat(never(), 100, 2, 3, max_bytes=1000)
    assert assoc.TRAITS_MAX_BYTES == 2 << 30
    # the chunks hold the device blocks and the results of one chunk below the module's limit
    step = assoc.traits_snps_per_chunk(A, 5, T)
    NF, NI, _, _ = assoc.layout(A, 5)
    assert step >= 1 and step * 4 * A * T * 8 <= assoc.STATS_CHUNK_BYTES and step * (NF * 8 + NI * 4 + A * 1024 * 8) <= assoc.STATS_CHUNK_BYTES
    assert assoc.traits_snps_per_chunk(32, 16, 65536) == 1
    with pytest.raises(ValueError, match="at most"):
        assoc.trait_covariates(2, np.zeros((2, assoc.MAX_T + 1)))
    with pytest.raises(ValueError, match="Y must be"):
        assoc.trait_covariates(2, np.zeros(2))


def test_chunked_write_assoc_equals_the_whole_file(tmp_path):
    from gnomix_amd import assoc, postprocess as pp
    st, ts = _regression(2)
    beta, se, t, n_alt, n_hap, n, df, n_miss, status = assoc.finish_traits(st, ts, 2, AC.K)
    res = assoc.AncestryAssoc(beta[:, :, 1], se[:, :, 1], t[:, :, 1], assoc.p_values(t[:, :, 1], df), n_alt, n_hap, n, df, n_miss, status)
    pos = 100 + 7 * np.arange(AC.C)
    pp.write_assoc(str(tmp_path / "whole"), "22", pos, AC.M, AC.W, res, ["P", "Q"])
    for c0, c1 in ((0, 50), (50, 51), (51, AC.C)):
        pp.write_assoc(str(tmp_path / "parts"), "22", pos, AC.M, AC.W, assoc.AncestryAssoc(*(v[c0:c1] for v in res)), ["P", "Q"], c0=c0, name="bmi")
    assert (tmp_path / "parts.assoc.bmi.tsv").read_bytes() == (tmp_path / "whole.assoc.tsv").read_bytes()


def test_header_and_library_carry_the_entry_points():
    from gnomix_amd import _lib
    text = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    for name in ("gnx_ancestry_assoc_traits", "gnx_ancestry_assoc_traits_dev", "gnx_ancestry_assoc_traits_gt2"):
        assert ("int %s(" % name) in text, name
        assert name in _lib.SYMBOLS, name
    assert "#define GNX_ASSOC_MAX_T 65536" in text and "#define GNX_ABI_VERSION 16" in text
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("gnx_ancestry_assoc_traits", "gnx_ancestry_assoc_traits_dev", "gnx_ancestry_assoc_traits_gt2"):
        assert hasattr(lib, name), name
    lib.gnx_abi_version.restype = ctypes.c_int
    assert lib.gnx_abi_version() == 16 == _lib.GNX_ABI_VERSION
