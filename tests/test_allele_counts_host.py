"""Ancestry-specific allele counts and dosage, the parts that need no GPU: the numpy restatement (tests/allele_counts_exact.py) on a
hand-worked example, the declarations and bindings, the .afreq.tsv writer and AlleleCounts.freq."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import allele_counts_exact as AE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# four haplotypes, seven SNPs, M = 3, W = 2: SNPs 0..2 are window 0, SNPs 3..6 window 1 (it takes the remainder)
X47 = np.array([[0, 1, 1, 0, 2, 1, 0],
                [1, 1, 0, 0, 1, 1, 7],
                [0, -1, 1, 1, 0, 0, 1],
                [1, 0, 0, 1, 1, 2, 0]], np.int8)
LAB47 = np.array([[0, 1], [1, 1], [0, 0], [1, 0]], np.int32)
OBS47 = np.array([[2, 1, 2, 2, 2, 1, 2], [2, 2, 2, 2, 1, 2, 1]], np.int32)
ALT47 = np.array([[0, 1, 2, 2, 1, 0, 1], [2, 1, 0, 0, 1, 2, 0]], np.int32)
MISS47 = np.array([[0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 1, 0, 1]], np.int32)
DOS47_0 = np.array([[0, 1, 1, 0, 0, 0, 0], [0, 0, 1, 2, 1, 0, 1]], np.uint8)      # ancestry 0
HAP47_0 = np.array([[1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 2, 2, 2, 2]], np.uint8)


def test_the_restatement_on_a_hand_worked_example():
    assert np.array_equal(AE.windows(7, 3, 2), [0, 0, 0, 1, 1, 1, 1])
    obs, alt, miss = AE.allele_counts(X47, LAB47, 3, 2)
    assert np.array_equal(obs, OBS47) and np.array_equal(alt, ALT47) and np.array_equal(miss, MISS47)
    assert obs.dtype == alt.dtype == miss.dtype == np.int32
    dos, hap = AE.dosage(X47, LAB47, 3, 2, 0)
    assert np.array_equal(dos, DOS47_0) and np.array_equal(hap, HAP47_0) and dos.dtype == hap.dtype == np.uint8
    # a label outside [0, A) counts for no ancestry: the row leaves the tables of the window it sits in
    lab = LAB47.copy()
    lab[2, 1] = 2
    obs2, alt2, miss2 = AE.allele_counts(X47, lab, 3, 2)
    assert np.array_equal(obs2[:, :3], OBS47[:, :3]) and np.array_equal(obs2[1], OBS47[1])
    assert np.array_equal(obs2[0, 3:], [1, 1, 0, 1]) and np.array_equal(alt2[0, 3:], [1, 1, 0, 0]) and np.array_equal(miss2[0, 3:], [0, 0, 1, 0])
    # packed rows: codes 2 and 3 are both missing, the codes survive the round trip
    codes = np.where((X47 == 0) | (X47 == 1), X47, 2).astype(np.uint8)
    codes[1, 6] = 3
    P = AE.pack2(codes, ldp=5, fill=0xFF)
    assert P.shape == (4, 5) and np.array_equal(AE.unpack2(P, 7), codes) and (P[:, 2:] == 0xFF).all() and (P[:, 1] >> 6 == 0).all()
    for got, want in zip(AE.allele_counts(AE.unpack2(P, 7), LAB47, 3, 2), (OBS47, ALT47, MISS47)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("N,C,M,W,A", [(10, 37, 5, 7, 3), (6, 16, 1, 16, 4), (8, 50, 7, 3, 2)])
def test_the_sum_identities_of_the_restatement(N, C, M, W, A):
    rng = np.random.RandomState(C)
    X = rng.choice([0, 1, 2, -1, 7], size=(N, C), p=[0.45, 0.4, 0.05, 0.05, 0.05]).astype(np.int8)
    lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
    obs, alt, miss = AE.allele_counts(X, lab, M, A)
    assert (obs + miss).sum(axis=0).tolist() == [N] * C and (alt <= obs).all()
    for a in range(A):
        dos, hap = AE.dosage(X, lab, M, A, a)
        assert np.array_equal(dos.sum(axis=0), alt[a]) and np.array_equal(hap.sum(axis=0), obs[a] + miss[a])
        assert (dos <= hap).all() and hap.max() <= 2


def test_symbols_bindings_and_the_config_default():
    """the five entries are declared, exported and typed as the header states them; the ABI version is unchanged"""
    from gnomix_amd import _lib, cli, multi
    from gnomix_amd.gnomix import HipGnomix
    from gnomix_amd.model import DeviceModel
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gnomix_hip.h")).read(), flags=re.S)
    ctype = {"gnx_ctx*": C.c_void_p, "gnx_model*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "const void*": C.c_void_p,
             "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}
    names = ("gnx_ancestry_allele_counts_dev", "gnx_ancestry_allele_counts", "gnx_ancestry_dosage_dev", "gnx_ancestry_dosage",
             "gnx_ancestry_allele_counts_gt2")
    for name in names:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        types = [re.sub(r"\s*\b\w+$", "", re.sub(r"\s+", " ", p.strip())).replace(" *", "*") for p in m.group(1).split(",")]
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and [ctype[t] for t in types] == list(args), name
        assert getattr(lib, name).argtypes == args
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16      # the ABI only grew
    assert re.search(r"#define\s+GNX_ABI_VERSION\s+16\b", hdr) and re.search(r"#define\s+GNX_ALLELE_MAX_A\s+32\b", hdr)
    assert re.search(r"enum\s*\{\s*GNX_ROWS_INT8\s*=\s*0\s*,\s*GNX_ROWS_PACKED2\s*=\s*1\s*\}", hdr)
    assert (_lib.GNX_ROWS_INT8, _lib.GNX_ROWS_PACKED2, _lib.GNX_ALLELE_MAX_A) == (0, 1, 32)
    assert "gnx_ancestry_allele_counts <- (no counterpart" in open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    for fn in (cli.run_inference, cli._run_and_write):
        assert inspect.signature(fn).parameters["ancestry_allele_freq_output"].default is False
    for owner in (DeviceModel, multi.DeviceGroup):
        assert callable(getattr(owner, "allele_counts_gt2"))
    for name in ("ancestry_allele_counts", "ancestry_dosage", "ancestry_allele_counts_device", "ancestry_dosage_device"):
        assert callable(getattr(DeviceModel, name)), name
    assert callable(HipGnomix.allele_frequencies)
    src = open(os.path.join(ROOT, "gnomix_amd", "cli.py")).read()
    assert src.count('inf.get("ancestry_allele_freq_output")') == 2      # both command-line routes read the key, absent = off


def test_phase_with_the_key_is_refused_before_any_work():
    from gnomix_amd import cli
    with pytest.raises(ValueError, match="allele_frequencies"):     # (no model, no file: nothing is touched before the refusal)
        cli.run_inference({"query_file": "/nonexistent.vcf", "chm": "22", "output_basename": "/nonexistent", "phase": True}, None,
                          ancestry_allele_freq_output=True)


def test_freq_is_nan_where_nothing_was_observed():
    from gnomix_amd import postprocess as pp
    c = pp.AlleleCounts(np.array([[4, 0, 3]], np.int32), np.array([[1, 0, 3]], np.int32), np.array([[0, 4, 1]], np.int32))
    f = c.freq()
    assert f.dtype == np.float64 and f.shape == (1, 3)
    assert f[0, 0] == 0.25 and np.isnan(f[0, 1]) and f[0, 2] == 1.0
    assert c.n_obs is c[0] and c.n_alt is c[1] and c.n_miss is c[2]
    want = pp.AlleleCounts(OBS47, ALT47, MISS47).freq()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(want, ALT47.astype(np.float64) / OBS47.astype(np.float64))


def test_write_afreq_bytes(tmp_path):
    from gnomix_amd import postprocess as pp
    obs = np.array([[2, 0, 3, 7], [1, 5, 0, 3]], np.int32)
    alt = np.array([[1, 0, 3, 2], [0, 5, 0, 1]], np.int32)
    c = pp.AlleleCounts(obs, alt, np.zeros_like(obs))
    prefix = str(tmp_path / "query_results")
    pp.write_afreq(prefix, "22", [101, 250, 251, 9000], 1, 3, c, ["AFR", "EUR"])
    text = open(prefix + ".afreq.tsv").read()
    assert text == (
        "chm\tpos\twindow\tAFR.n_obs\tAFR.n_alt\tAFR.freq\tEUR.n_obs\tEUR.n_alt\tEUR.freq\n"
        "22\t101\t0\t2\t1\t0.500000\t1\t0\t0.000000\n"
        "22\t250\t1\t0\t0\tnan\t5\t5\t1.000000\n"
        "22\t251\t2\t3\t3\t1.000000\t0\t0\tnan\n"
        "22\t9000\t2\t7\t2\t0.285714\t3\t1\t0.333333\n")
    assert text == AE.afreq_text("22", [101, 250, 251, 9000], 1, 3, obs, alt, ["AFR", "EUR"])
    with pytest.raises(ValueError):
        pp.write_afreq(prefix, "22", [101, 250, 251], 1, 3, c, ["AFR", "EUR"])
