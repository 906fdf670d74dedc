"""Admixture mapping, the host half on the CPU (gnomix_amd/admixmap.py): the finish fed the restatement's exact blocks against lstsq, the
p-values, the permutations and their adjusted p-values, the .msp reader and the .admixmap writer, the refusals of the front."""
import os

import numpy as np
import pytest

import admixmap_cases as MC
import admixmap_exact as XE
import assoc_cases as AC
from gnomix_amd import admixmap, postprocess


def _stats(key, Ycols=None):
    """AdmixStats of case(*key) from the restatement's blocks (rounded to float64 once)"""
    lab, Y, Z, use = MC.case(*key)
    Y = Y if Ycols is None else Ycols
    A, K = key[3], key[4]
    return admixmap.split_blocks(*XE.float_blocks(lab, A, Y, Z, use, 0, lab.shape[1]), A, K, Y.shape[1])


def _exact_fields(res, want):
    for name in ("n", "df1", "df2", "status"):
        assert np.array_equal(getattr(res, name), want[name]), name
    assert np.array_equal(res.n_hap, want["hs"]) and np.array_equal(res.kept, want["kept"])
    for name in ("beta", "se", "t", "F"):
        assert np.array_equal(np.isnan(getattr(res, name)), np.isnan(want[name])), name
    assert np.array_equal(np.isnan(res.p), np.isnan(want["t"])) and np.array_equal(np.isnan(res.p_joint), np.isnan(want["F"]))


def result_ratio(res, want):
    """the largest err / (p kappa^2 2^-53 max|beta|) of beta, se and t over the compared windows (the project's bound is C_TOL of it)"""
    cells = MC.compared(want)[:, None, None]
    worst = 0.0
    with np.errstate(invalid="ignore"):
        bmax = np.nanmax(np.abs(np.where(np.isnan(want["beta"]), 0.0, want["beta"])), axis=1)
        scale = ((want["p_kept"] * want["kappa"] ** 2 * 2.0 ** -53)[:, None] * bmax)[:, None, :]
        for name in ("beta", "se", "t"):
            r = np.where(cells, np.abs(getattr(res, name) - want[name]) / scale, np.nan)
            worst = max(worst, float(np.nanmax(r)))
    return worst


def f_reference_error():
    """r_ref: the largest relative difference between the float64-lstsq F and the Fraction F over the compared cells of the FIT cases"""
    r = 0.0
    for key in MC.FIT:
        want = MC.check_fit_case(key)
        ok = MC.compared(want)
        f, fe = want["F"][ok], want["F_exact"][ok]
        m = ~np.isnan(f)
        r = max(r, float(np.max(np.abs(f[m] - fe[m]) / np.abs(fe[m]))))
    return r


def f_ratio(res, want):
    ok = MC.compared(want)
    f, fe = res.F[ok], want["F_exact"][ok]
    m = ~np.isnan(fe)
    return float(np.max(np.abs(f[m] - fe[m]) / np.abs(fe[m])))


@pytest.mark.parametrize("key", MC.FIT + [MC.FIT_RAW])
def test_finish_against_lstsq(key):
    """beta, se and t within C_TOL p kappa^2 2^-53 max|beta|; the integer fields, kept, status, df1, df2 and the NaN patterns exact; p and
    p_joint against scipy at the asserted t and F"""
    from scipy import special
    want = MC.check_fit_case(key)
    res = admixmap.finish(_stats(key), key[4], MC.MIN_HAP)
    _exact_fields(res, want)
    ratio = result_ratio(res, want)
    print("largest ratio", key, ratio)
    assert ratio <= AC.C_TOL
    df = (want["n"] - key[4] - 1).astype(np.float64)
    m = ~np.isnan(res.t)
    assert np.array_equal(res.p[m], (2.0 * special.stdtr(df[:, None, None], -np.abs(res.t)))[m])
    m = ~np.isnan(res.F)
    assert np.array_equal(res.p_joint[m], special.fdtrc(res.df1[:, None].astype(float), res.df2[:, None].astype(float), res.F)[m])


@pytest.mark.parametrize("key", MC.GRID)
def test_finish_exact_fields_on_the_grid(key):
    """the small cases of the device grid: the integer fields, status and the NaN patterns (they have no fitted window to compare)"""
    lab, Y, Z, use = MC.case(*key)
    want = XE.fit(lab, key[3], Y, Z, use, MC.MIN_HAP, exact_F=False)
    _exact_fields(admixmap.finish(_stats(key), key[4], MC.MIN_HAP), want)


def test_F_tolerance():
    """F within 64 r_ref of the Fraction F, r_ref the reference's own error (float64 lstsq against Fraction arithmetic, both computed here).
    Measured on the CPU: r_ref = 3.24e-11 (a cell whose F is small: RSS0 - RSS1 cancels in the float64 reference); the finish's largest error is
    7.88e-14 = 2.4e-3 r_ref."""
    r_ref = f_reference_error()
    worst = max(f_ratio(admixmap.finish(_stats(key), key[4], MC.MIN_HAP), MC.fit_of(key)) for key in MC.FIT)
    print("r_ref", r_ref, "finish", worst, "ratio", worst / r_ref)
    assert worst <= 64 * r_ref


def test_permutation_columns_equal_the_restatement():
    lab, Y, Z, use = MC.case(*MC.PERM)
    got = admixmap.permutation_columns(Y, Z, use, MC.SEED, 2, 6)
    want = XE.permutation_columns(Y, Z, use, MC.SEED, 2, 6)
    assert np.array_equal(got, want, equal_nan=True) and got.shape == (MC.PERM[0], 4 * MC.PERM[1])
    assert np.array_equal(admixmap.permutation_columns(Y, Z, use, MC.SEED, 0, 7)[:, 2 * 2:6 * 2], got, equal_nan=True)


def _meta(W):
    return {"chm": ["22"] * W, "spos": np.arange(W) * 100 + 1, "epos": np.arange(W) * 100 + 100, "sgpos": np.arange(W) * 0.5,
            "egpos": np.arange(W) * 0.5 + 0.25, "n snps": np.full(W, 100)}


def _host_run(lab, A, Y, Z, use, n_perm, chunk_bytes=None):
    """admixmap.run over the restatement's blocks in place of the device"""
    def stats_fn(Yc, Zc, uc):
        return admixmap.split_blocks(*XE.float_blocks(lab, A, Yc, Zc, uc, 0, lab.shape[1]), A, Zc.shape[1], Yc.shape[1])
    return admixmap.run(stats_fn, lab.shape[1], A, Y, Z, use, MC.MIN_HAP, n_perm, MC.SEED, chunk_bytes)


def test_adjusted_p_values_exact():
    want, mt, mF = MC.perm_reference()
    lab, Y, Z, use = MC.case(*MC.PERM)
    res = _host_run(lab, MC.PERM[3], Y, Z, use, MC.N_PERM)
    assert res.perm_max_t.shape == (2, MC.N_PERM) and res.perm_max_F.shape == (2, MC.N_PERM)
    np.testing.assert_allclose(res.perm_max_t, mt, rtol=1e-9)
    np.testing.assert_allclose(res.perm_max_F, mF, rtol=1e-9)
    assert np.array_equal(res.p_adj_t, XE.adjusted(np.abs(want["t"]), mt), equal_nan=True)
    assert np.array_equal(res.p_adj_F, XE.adjusted(want["F"], mF), equal_nan=True)
    assert _host_run(lab, MC.PERM[3], Y, Z, use, 0).perm_max_t is None


def test_more_traits_than_a_chunk_holds():
    """T = 17 with chunks of 16 columns: the observed pass and every permutation are cut along the trait axis; nothing changes"""
    key = (MC.N_FIT, 17, 19, 3, 3)
    lab, Y, Z, use = MC.case(*key)
    calls = []

    def stats_fn(Yc, Zc, uc):
        calls.append(Yc.shape[1])
        return admixmap.split_blocks(*XE.float_blocks(lab, 3, Yc, Zc, uc, 0, 19), 3, 3, Yc.shape[1])
    whole = admixmap.run(stats_fn, 19, 3, Y, Z, use, MC.MIN_HAP, 2, MC.SEED)
    assert calls == [17, 34]
    del calls[:]
    cut = admixmap.run(stats_fn, 19, 3, Y, Z, use, MC.MIN_HAP, 2, MC.SEED, chunk_bytes=1)
    assert calls == [16, 1, 16, 1, 16, 1] and max(calls) <= admixmap.columns_per_chunk(19, 3, 3, 1)
    assert all(np.array_equal(getattr(whole, f), getattr(cut, f), equal_nan=True) for f in whole._fields)


def test_two_chromosomes_combine_with_maximum():
    lab, Y, Z, use = MC.case(*MC.PERM)
    A = MC.PERM[3]
    whole = _host_run(lab, A, Y, Z, use, MC.N_PERM)
    one, two = (_host_run(np.ascontiguousarray(part), A, Y, Z, use, MC.N_PERM) for part in (lab[:, :8], lab[:, 8:]))
    assert np.array_equal(np.maximum(one.perm_max_t, two.perm_max_t), whole.perm_max_t)
    assert np.array_equal(np.maximum(one.perm_max_F, two.perm_max_F), whole.perm_max_F)


@pytest.mark.parametrize("n_ind,W", [(1, 1), (5, 4)])
def test_read_msp_round_trip(tmp_path, n_ind, W):
    rng = np.random.RandomState(n_ind)
    lab = rng.randint(0, 3, size=(2 * n_ind, W)).astype(np.int32)
    pops, samples = ["AFR", "EUR", "NAT"], ["s%d" % i for i in range(n_ind)]
    meta = _meta(W)
    postprocess.write_msp(str(tmp_path / "q"), meta, lab, pops, samples)
    got = postprocess.read_msp(str(tmp_path / "q.msp"))
    assert np.array_equal(got.labels, lab) and got.labels.dtype == np.int32 and got.labels.flags.c_contiguous
    assert got.populations == pops and got.samples == samples
    assert got.meta["chm"] == ["22"] * W
    for name in ("spos", "epos", "sgpos", "egpos", "n snps"):
        assert np.array_equal(got.meta[name], meta[name]), name


def test_write_admixmap_format(tmp_path):
    key = MC.PERM
    lab, Y, Z, use = MC.case(*key)
    res = _host_run(lab, key[3], Y, Z, use, MC.N_PERM)
    W = lab.shape[1]
    pops = ["AFR", "EUR", "NAT"]
    meta = _meta(W)
    paths = postprocess.write_admixmap(str(tmp_path / "q"), meta, res, pops, ["height", "bmi"])
    assert [os.path.basename(p) for p in paths] == ["q.admixmap.height.tsv", "q.admixmap.bmi.tsv"]
    lines = open(paths[1]).read().splitlines()
    head = lines[0].split("\t")
    assert head[:6] == ["#chm", "spos", "epos", "sgpos", "egpos", "n snps"]
    assert head[6:13] == ["n", "status", "df1", "df2", "F", "p_joint", "p_adj_F"]
    assert head[13:19] == ["AFR.n_hap", "AFR.beta", "AFR.se", "AFR.t", "AFR.p", "AFR.p_adj"] and len(head) == 13 + 6 * 3
    assert len(lines) == 1 + W
    row = lines[8].split("\t")
    assert row[0] == "22" and int(row[1]) == 701 and int(row[6]) == res.n[7] and int(row[13]) == res.n_hap[7, 0]
    six = lambda v: float(format(float(v), ".6g"))
    assert float(row[10]) == six(res.F[7, 1]) and float(row[14]) == six(res.beta[7, 0, 1]) and float(row[18]) == six(res.p_adj_t[7, 0, 1])
    assert lines[4].split("\t")[10] == "nan"          # window 3: nothing to test
    one = postprocess.write_admixmap(str(tmp_path / "r"), meta, _host_run(lab, key[3], Y[:, :1], Z, use, 0), pops)
    assert [os.path.basename(p) for p in one] == ["r.admixmap.tsv"]
    assert "p_adj_F" not in open(one[0]).readline() and "AFR.p_adj" not in open(one[0]).readline()


def test_front_refusals(tmp_path):
    lab, Y, Z, use = MC.case(*MC.PERM)
    A = MC.PERM[3]
    with pytest.raises(ValueError, match="even"):
        admixmap.admixture_mapping(None, lab[:-1], A, Y, Z, use)
    with pytest.raises(ValueError, match="Y must be"):
        admixmap.admixture_mapping(None, lab, A, Y[:-1], Z, use)
    with pytest.raises(ValueError, match="min_hap"):
        admixmap.admixture_mapping(None, lab, A, Y, Z, use, min_hap=0)
    with pytest.raises(ValueError, match="n_perm"):
        admixmap.admixture_mapping(None, lab, A, Y, Z, use, n_perm=-1)
    # the command line: every error before any work (the model is never touched: None)
    from gnomix_amd import cli
    args = {"query_file": str(tmp_path / "q.vcf"), "chm": "22", "output_basename": str(tmp_path), "phase": False}
    ph = tmp_path / "pheno.tsv"
    ph.write_text("sample\tpheno\ns0\t1.0\n")
    with pytest.raises(ValueError, match="admixture_mapping_output needs"):
        cli.run_inference(args, None, admixture_mapping_output=True)
    with pytest.raises(ValueError, match="phenotype_file: no such file"):
        cli.run_inference(args, None, admixture_mapping_output=True, phenotype_file=str(tmp_path / "absent.tsv"))
    with pytest.raises(ValueError, match="trait_file: no such file"):
        cli.run_inference(args, None, admixture_mapping_output=True, trait_file=str(tmp_path / "absent.tsv"))
    with pytest.raises(ValueError, match="covariate_file: no such file"):
        cli.run_inference(args, None, admixture_mapping_output=True, trait_file=str(ph), covariate_file=str(tmp_path / "absent.tsv"))
    with pytest.raises(ValueError, match="admixture_mapping_perms"):
        cli.run_inference(args, None, admixture_mapping_output=True, phenotype_file=str(ph), admixture_mapping_perms=-1)
    with pytest.raises(ValueError, match="admixture_mapping_min_hap"):
        cli.run_inference(args, None, admixture_mapping_output=True, phenotype_file=str(ph), admixture_mapping_min_hap=0)
    assert sorted(os.listdir(str(tmp_path))) == ["pheno.tsv"]
