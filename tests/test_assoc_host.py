"""CPU tests (-m "not gpu") of the ancestry-specific association: the numpy restatement (tests/assoc_exact.py) against a hand-worked
case, the host finish (gnomix_amd/assoc.py) fed the restatement's blocks against the restatement's lstsq, the column rule and the
statuses, the phenotype-file reader, write_assoc's bytes and the ABI symbols."""
import ctypes
import os
import types

import numpy as np
import pytest

import assoc_cases as AC
import assoc_exact as XE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _finish(X, lab, M, A, y, Z, use=None, min_ac=1, slow=True):
    from gnomix_amd import assoc
    C, W, K = X.shape[1], lab.shape[1], np.asarray(Z).shape[1]
    b = (XE.blocks_slow if slow else XE.blocks)(X, lab, M, A, y, Z, use, 0, C)
    st = assoc.split_blocks(b[0], b[1], b[2], b[3], A, K, 0, C, M, W, b[4])
    return assoc.finish(st, A, K, min_ac)


# the hand-worked case: A = 2, K = 1, one SNP, one window; columns [1, h_0, d_0] (d_1 is all zero and dropped)
#   labels (0,0) (0,1) (1,1) (0,1); ALT on the first haplotype of individuals 0 and 3  ->  rows (1,2,1) (1,1,0) (1,0,0) (1,1,1)
#   y = 1 + 1 h_0 + 2 d_0 + r with r = (1,-1,1,-1) orthogonal to all three columns: y = (6, 1, 2, 3), RSS = 4, df = 1
#   X^T X = [[4,4,2],[4,6,3],[2,3,2]], det 4, cofactor (d_0, d_0) = 8: (X^T X)^-1 = 2 there; se = sqrt(4 * 2), t = 2 / sqrt(8)
HW_X = np.array([[1], [0], [0], [0], [0], [0], [1], [0]], np.int8)
HW_LAB = np.array([[0], [0], [0], [1], [1], [1], [0], [1]], np.int32)
HW_Y = np.array([6.0, 1.0, 2.0, 3.0])
HW_Z = np.ones((4, 1))


def test_restatement_on_the_hand_worked_case():
    r = XE.fit(HW_X, HW_LAB, 1, 2, HW_Y, HW_Z)
    assert r["status"][0] == 0 and r["n"][0] == 4 and r["df"][0] == 1 and r["n_miss"][0] == 0
    assert r["n_alt"].tolist() == [[2, 0]] and r["n_hap"].tolist() == [[4, 4]]
    assert abs(r["beta"][0, 0] - 2.0) < 1e-12 and abs(r["se"][0, 0] - np.sqrt(8.0)) < 1e-12 and abs(r["t"][0, 0] - 2 / np.sqrt(8.0)) < 1e-12
    assert np.isnan(r["beta"][0, 1]) and np.isnan(r["se"][0, 1]) and np.isnan(r["t"][0, 1])
    for blocks in (XE.blocks_slow, XE.blocks):
        sf, si, wf, wi, n_bad = blocks(HW_X, HW_LAB, 1, 2, HW_Y, HW_Z, None, 0, 1)
        assert sf.tolist() == [[2.0, 9.0, 0.0, 0.0]]                       # [a][k]: D^T Z, D^T y
        assert si.tolist() == [[2, 0, 0, 3, 0, 2, 0, 0]]                   # D^T D (00, 01, 11), D^T H (0, 1), sum d, n_miss
        assert wf.reshape(3, 3).tolist() == [[4, 4, 12], [4, 6, 16], [12, 16, 50]]
        assert wi.tolist() == [[4, 4, 4]] and n_bad == 0


def test_fast_blocks_equal_the_literal_ones():
    rng = np.random.RandomState(2)
    N, C, M, W, A, K = 14, 23, 5, 4, 3, 2
    X = rng.choice([0, 1, 2, -1], size=(N, C), p=[0.45, 0.4, 0.1, 0.05]).astype(np.int8)
    lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
    lab[4, 1] = A          # out of range: individual 2 takes no part at window 1
    y = rng.randint(-1024, 1025, size=N // 2).astype(np.float64)
    Z = rng.randint(-1024, 1025, size=(N // 2, K)).astype(np.float64)
    y[5] = np.nan
    use = np.ones(N // 2, np.uint8)
    use[0] = 0
    for c0, c1 in ((0, C), (3, 17)):
        a, b = XE.blocks_slow(X, lab, M, A, y, Z, use, c0, c1), XE.blocks(X, lab, M, A, y, Z, use, c0, c1)
        for u, v in zip(a[:4], b[:4]):
            assert u.dtype == v.dtype and np.array_equal(u, v)
        assert a[4] == b[4] == 1


def test_finish_on_the_hand_worked_case():
    beta, se, t, n_alt, n_hap, n, df, n_miss, status = _finish(HW_X, HW_LAB, 1, 2, HW_Y, HW_Z)
    assert status.tolist() == [0] and n.tolist() == [4] and df.tolist() == [1] and n_alt.tolist() == [[2, 0]] and n_hap.tolist() == [[4, 4]]
    assert abs(beta[0, 0] - 2.0) < 1e-12 and abs(se[0, 0] - np.sqrt(8.0)) < 1e-12 and abs(t[0, 0] - 2 / np.sqrt(8.0)) < 1e-12
    assert np.isnan(beta[0, 1]) and np.isnan(se[0, 1]) and np.isnan(t[0, 1])


def test_finish_against_lstsq_and_the_constant():
    """the host finish fed the restatement's blocks (math.fsum) against lstsq on the full design over the GPU test's inputs; the largest
    ratio err / (p kappa^2 2^-53 max|beta|) must leave the margin of 8 that C_TOL holds for the device's summation order"""
    worst = 0.0
    for A in (2, 3, 7):
        X, lab, y, Z, use = AC.regression_case(A)
        want = AC.regression_fit(A)
        beta, se, t, n_alt, n_hap, n, df, n_miss, status = _finish(X, lab, AC.M, A, y, Z, use)
        for g, name in ((n_alt, "n_alt"), (n_hap, "n_hap"), (n, "n"), (df, "df"), (n_miss, "n_miss"), (status, "status")):
            assert np.array_equal(g, want[name]), name
        r, left_out = AC.ratios(beta, se, t, want)
        print("A = %d: ratio %.4g, SNPs left out %.3f, max kappa %.4g" % (A, r, left_out, np.nanmax(want["kappa"])))
        assert left_out < 0.05          # the restatement alone meets the cap on the cases left out
        assert (want["status"] == 0).all()
        worst = max(worst, r)
    print("largest ratio %.4g (assoc_cases.MEASURED_RATIO = %.4g, C_TOL = %.4g)" % (worst, AC.MEASURED_RATIO, AC.C_TOL))
    assert worst <= AC.C_TOL / 8


def _small(seed=0, n_ind=12, C=6, A=2):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, A, size=(2 * n_ind, 1)).astype(np.int32)
    X = rng.randint(0, 2, size=(2 * n_ind, C)).astype(np.int8)
    y = rng.normal(size=n_ind)
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, 1))], 1)
    return X, lab, y, Z


def test_column_rule_min_ac_and_statuses():
    X, lab, y, Z = _small()
    A, C = 2, X.shape[1]
    X[:, 0] = 0                         # SNP 0: no ALT at all: both dosage columns dropped, the fit of the rest stands
    X[:, 1] = 0
    X[np.where(lab[:, 0] == 1)[0][0], 1] = 1     # SNP 1: one ALT copy on ancestry 1: kept at min_ac = 1, dropped at min_ac = 2
    X[:, 2] = 1                         # SNP 2: every call ALT: d_a == h_a, the design is rank-deficient: status 1
    for min_ac in (1, 2):
        want = XE.fit(X, lab, C, A, y, Z, min_ac=min_ac)
        beta, se, t, n_alt, n_hap, n, df, n_miss, status = _finish(X, lab, C, A, y, Z, min_ac=min_ac)
        assert np.array_equal(status, want["status"]) and np.array_equal(df, want["df"])
        assert status[0] == 0 and np.isnan(beta[0]).all() and df[0] == n[0] - 3
        assert status[2] == 1 and np.isnan(beta[2]).all() and np.isnan(se[2]).all() and np.isnan(t[2]).all()
        assert np.array_equal(np.isnan(beta), np.isnan(want["beta"]))
        ok = ~np.isnan(want["beta"])
        assert np.allclose(beta[ok], want["beta"][ok], rtol=1e-9, atol=1e-12) and np.allclose(se[ok], want["se"][ok], rtol=1e-9, atol=1e-12)
        assert n_alt[1].tolist() == [0, 1]
        assert np.isnan(beta[1, 1]) == (min_ac == 2) and df[1] == n[1] - (4 if min_ac == 1 else 3)
    # a window where ancestry 0 is absent: its hapcount column is dropped, not a reason for status 1
    lab1 = np.ones_like(lab)
    want = XE.fit(X, lab1, C, A, y, Z)
    res = _finish(X, lab1, C, A, y, Z)
    assert res[8][3] == 0 and want["status"][3] == 0 and want["p_kept"][3] == 3 and np.isnan(res[0][3, 0]) and np.isfinite(res[0][3, 1])
    # df < 1: four individuals, p_kept = 4 -> status 2; use = 0 takes individuals out
    use = np.zeros(len(y), np.uint8)
    use[:4] = 1
    want = XE.fit(X, lab, C, A, y, Z, use)
    res = _finish(X, lab, C, A, y, Z, use)
    assert np.array_equal(res[8], want["status"]) and (res[5] == 4).all() and (res[8][res[6] < 1] == 2).all() and (res[6] < 1).any()
    assert np.isnan(res[0][res[8] == 2]).all()
    with pytest.raises(ValueError):
        _finish(X, lab, C, A, y, Z, min_ac=0)


def test_p_values_are_scipys_two_sided_t():
    from scipy import stats
    from gnomix_amd import assoc
    t = np.array([[0.0, 2.0], [np.nan, -3.5]])
    p = assoc.p_values(t, np.array([10, 3]))
    assert p[0, 0] == 1.0 and abs(p[0, 1] - 2 * stats.t.sf(2.0, 10)) < 1e-15 and np.isnan(p[1, 0]) and abs(p[1, 1] - 2 * stats.t.sf(3.5, 3)) < 1e-15


def test_phenotype_file_reader(tmp_path):
    from gnomix_amd import assoc
    path = tmp_path / "pheno.tsv"
    path.write_text("sample\tpheno\tage\tpc1\n" "s2\t1.5\t40\t0.1\n" "s0\tNA\t30\t0.2\n" "s3\t2.5\tinf\t0.3\n" "zz\t9\t9\t9\n" "s4\t-1\t\t0.5\n")
    y, Z, use, names = assoc.read_phenotypes(str(path), ["s0", "s1", "s2", "s3", "s4"])
    assert names == ["intercept", "age", "pc1"] and Z.shape == (5, 3) and (Z[:, 0] == 1).all()
    assert use.tolist() == [0, 0, 1, 1, 1]                      # s0: a missing value; s1: unknown to the file; zz: unknown to the query
    assert np.isnan(y[0]) and np.isnan(y[1]) and y[2] == 1.5 and y[3] == 2.5 and y[4] == -1
    assert Z[2].tolist() == [1, 40, 0.1] and np.isinf(Z[3, 1]) and np.isnan(Z[4, 1]) and np.isnan(Z[1, 1:]).all()
    lab = np.zeros((10, 1), np.int32)
    assert XE.participation(lab, 1, y, Z, use)[:, 0].tolist() == [False, False, True, False, False]   # non-finite covariates take no part
    bad = tmp_path / "bad.tsv"
    bad.write_text("id\tpheno\ns0\t1\n")
    with pytest.raises(ValueError):
        assoc.read_phenotypes(str(bad), ["s0"])
    bad.write_text("sample\tpheno\ns0\t1\ns0\t2\n")
    with pytest.raises(ValueError):
        assoc.read_phenotypes(str(bad), ["s0"])
    bad.write_text("sample\tpheno\ns0\tabc\n")
    with pytest.raises(ValueError):
        assoc.read_phenotypes(str(bad), ["s0"])


def test_write_assoc_bytes(tmp_path):
    from gnomix_amd import assoc, postprocess as pp
    r = XE.fit(HW_X, HW_LAB, 1, 2, HW_Y, HW_Z)
    p = assoc.p_values(r["t"], r["df"])
    res = assoc.AncestryAssoc(r["beta"], r["se"], r["t"], p, r["n_alt"], r["n_hap"], r["n"], r["df"], r["n_miss"], r["status"])
    pp.write_assoc(str(tmp_path / "q"), "22", [12345], 1, 1, res, ["AFR", "EUR"])
    got = (tmp_path / "q.assoc.tsv").read_text()
    assert got == XE.assoc_text("22", [12345], 1, 1, r, p, ["AFR", "EUR"])
    assert got == ("chm\tpos\twindow\tn\tdf\tstatus\tn_miss\tAFR.n_hap\tAFR.n_alt\tAFR.beta\tAFR.se\tAFR.t\tAFR.p\tEUR.n_hap\tEUR.n_alt\tEUR.beta\tEUR.se\tEUR.t\tEUR.p\n"
                   "22\t12345\t0\t4\t1\t0\t0\t4\t2\t2\t2.82843\t0.707107\t0.608173\t4\t0\tnan\tnan\tnan\tnan\n")
    with pytest.raises(ValueError):
        pp.write_assoc(str(tmp_path / "q"), "22", [1, 2], 1, 1, res, ["AFR", "EUR"])


def test_abi_symbols_are_built_and_declared():
    from gnomix_amd import _lib
    lib = _lib.load()
    for name in ("gnx_ancestry_assoc_stats", "gnx_ancestry_assoc_stats_dev", "gnx_ancestry_assoc_stats_gt2"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16
    hdr = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    assert "GNX_ASSOC_MAX_K 16" in hdr
    from gnomix_amd import assoc
    assert assoc.layout(7, 5) == (42, 28 + 42 + 7 + 1, 144, 8) and assoc.snps_per_chunk(7, 5) * (42 * 8 + 78 * 4) <= assoc.STATS_CHUNK_BYTES


def test_run_inference_refuses_the_key_with_phase_before_any_work(tmp_path):
    from gnomix_amd import cli
    args = {"query_file": str(tmp_path / "none.vcf"), "chm": "22", "output_basename": str(tmp_path), "phase": True}
    with pytest.raises(ValueError, match="ancestry_assoc_output with phase=True"):
        cli.run_inference(args, None, ancestry_assoc_output=True, phenotype_file=str(tmp_path / "p.tsv"))
    with pytest.raises(ValueError, match="phenotype_file"):
        cli.run_inference(dict(args, phase=False), None, ancestry_assoc_output=True)
    assert os.listdir(str(tmp_path)) == []
