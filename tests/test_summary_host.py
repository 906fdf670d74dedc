"""Global ancestry and tract summaries, the parts that need no GPU: the plain-Python restatement (tests/summary_exact.py) against
its exact rational form and its own properties, window_weights, the .Q / .tracts.tsv writers, the new symbols and the config key."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import labels_exact as LE
import summary_exact as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _rows(N, W, A, seed):
    """rows of runs of random lengths with scattered single-window flips, plus a constant and an alternating row"""
    rng = np.random.RandomState(seed + 31 * W + A)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 3 + 1)), 3, axis=1)[:, :W]
    flips = rng.rand(N, W) < 0.2
    lab[flips] = rng.randint(0, A, size=int(flips.sum()))
    lab[0] = A - 1
    lab[1] = np.arange(W) % 2
    return lab.astype(np.int32)


CASES = [(4, 1, 2), (4, 2, 3), (5, 63, 3), (5, 64, 7), (5, 65, 7), (4, 129, 4), (3, 200, 32)]


@pytest.fixture(scope="module")
def cases():
    out = []
    for N, W, A in CASES:
        rng = np.random.RandomState(W)
        lab = _rows(N, W, A, 1)
        w = rng.gamma(0.7, 0.3, size=W) + 1e-9
        w[rng.rand(W) < 0.1] = 0.0                      # windows without length are legal
        if not w.sum():
            w[0] = 0.25
        P = rng.dirichlet(np.ones(A) * 0.3, size=(N, W))
        out.append((lab, w, A, P, SE.summary(lab, w, A, P)))
    return out


def test_the_two_restatements_are_the_same_arithmetic(cases):
    """summary_row (Python floats, the text of the order) and summary (numpy, element by element) agree bit for bit, for float64
    and for float32 probabilities"""
    for lab, w, A, P, got in cases:
        got32 = SE.summary(lab, w, A, P.astype(np.float32))
        for n in range(lab.shape[0]):
            row = SE.summary_row(lab[n], w, A, P[n])
            row32 = SE.summary_row(lab[n], w, A, P[n].astype(np.float32))
            for k in ("hard", "soft", "tract_total", "tract_longest"):
                assert np.array_equal(np.array(row[k]), got[k][n]), (lab.shape, n, k)
            assert np.array_equal(np.array(row32["soft"]), got32["soft"][n])
            assert row["tract_count"] == got["tract_count"][n].tolist()
        assert got["tract_count"].dtype == np.int32 and got["hard"].dtype == np.float64


def test_restatement_is_within_the_derived_bound_of_the_exact_form(cases):
    """every value within relative error 2 (W + 2) 2^-53 of the exact rational: the first-order bound for two W-term sums of
    non-negative float64 terms, W rounded products and one division (derived, not measured)"""
    for lab, w, A, P, got in cases:
        W = lab.shape[1]
        bound = Fraction(2 * (W + 2)) * Fraction(U)
        for n in range(lab.shape[0]):
            ex = SE.summary_fraction(lab[n], w, A, P[n])
            assert ex["tract_count"] == got["tract_count"][n].tolist()
            for k in ("hard", "soft", "tract_total", "tract_longest"):
                for a in range(A):
                    e, g = ex[k][a], Fraction(float(got[k][n, a]))
                    assert abs(g - e) <= bound * abs(e), (lab.shape, n, k, a, float(e), float(g))


@pytest.mark.parametrize("kind", ["snps", "bp"])
def test_integer_weights_make_hard_exact(kind):
    """integer weights below 2^53: both sums are exact, hard is numpy's num / den bit for bit"""
    rng = np.random.RandomState(3)
    for N, W, A in CASES:
        lab = _rows(N, W, A, 2)
        w = (rng.randint(0, 400, size=W) if kind == "snps" else rng.randint(1, 1 << 40, size=W)).astype(np.float64)
        w[0] = max(w[0], 1.0)
        got = SE.summary(lab, w, A)
        wi = w.astype(np.int64)
        num = np.array([[int(wi[lab[n] == a].sum()) for a in range(A)] for n in range(N)], dtype=np.int64)
        assert int(wi.sum()) < 2 ** 53
        assert np.array_equal(got["hard"], num.astype(np.float64) / np.float64(wi.sum()))
        assert np.array_equal(got["tract_total"], num.astype(np.float64)) and got["soft"] is None


def test_properties(cases):
    for lab, w, A, P, got in cases:
        den = SE.denominator(w)
        assert np.all(np.abs(got["hard"].sum(axis=1) - 1.0) <= A * 2.0 ** -52)
        assert np.array_equal(got["tract_total"] / den, got["hard"])
        counts, _, _ = LE.label_runs(lab)
        assert np.array_equal(got["tract_count"].sum(axis=1), counts)
        assert np.all(got["tract_longest"][got["tract_count"] == 0] == 0)      # (longest and total are summed in different orders)
        assert got["tract_count"][0].tolist() == [0] * (A - 1) + [1]                       # the constant row: one tract
        if lab.shape[1] > 1:
            assert got["tract_count"][1, :2].sum() == lab.shape[1]                         # the alternating row: W tracts


def test_a_label_out_of_range_belongs_to_no_class_and_ends_a_run():
    lab = np.array([[0, 0, 5, 0, -1, 1]], np.int32)
    got = SE.summary(lab, np.ones(6), 2)
    assert got["tract_count"].tolist() == [[2, 1]] and got["tract_total"].tolist() == [[3.0, 1.0]] and got["tract_longest"].tolist() == [[2.0, 1.0]]
    assert got["hard"].tolist() == [[0.5, 1.0 / 6.0]]


def _meta_and_msp(tmp_path):
    """a ragged last window: 7 windows of 10 SNPs over 75 model SNPs"""
    from gnomix_amd import postprocess as pp
    model_pos = 1000 + 137 * np.arange(75)
    query_pos = model_pos[::2]
    meta = pp.get_meta_data("22", model_pos, query_pos, 7, 10, np.array([1, 4000, 20000]), np.array([0.0, 1.25, 7.5]))
    lab = np.array([[0, 0, 1, 1, 1, 2, 2], [2, 2, 2, 2, 2, 2, 2], [0, 1, 0, 1, 0, 1, 0], [1, 1, 1, 0, 0, 0, 0]], np.int32)
    prefix = str(tmp_path / "q")
    pp.write_msp(prefix, meta, lab, ["AFR", "EUR", "NAT"], ["s1", "s2"])
    return meta, lab, prefix


def test_window_weights_equal_the_msp_columns(tmp_path):
    from gnomix_amd import postprocess as pp
    meta, lab, prefix = _meta_and_msp(tmp_path)
    rows = [ln.rstrip("\n").split("\t") for ln in open(prefix + ".msp").read().splitlines()[2:]]
    assert len(rows) == 7 and int(rows[-1][5]) != int(rows[0][5])                          # the last window is the ragged one
    spos, epos, sg, eg, ns = (np.array([float(r[c]) for r in rows]) for c in (1, 2, 3, 4, 5))
    for kind, want in (("cM", eg - sg), ("bp", epos - spos), ("snps", ns)):
        got = pp.window_weights(meta, kind)
        assert got.dtype == np.float64 and np.array_equal(got, want), kind
    with pytest.raises(ValueError, match="kind"):
        pp.window_weights(meta, "windows")


def test_writers_on_hand_made_input(tmp_path):
    from gnomix_amd import postprocess as pp
    hard = np.array([[0.5, 0.25, 0.25], [0.0, 0.0, 1.0], [0.123456, 0.876544, 0.0], [1.0 / 3.0, 2.0 / 3.0, 0.0]])
    s = pp.AncestrySummary(hard, None, np.array([[1, 1, 1], [0, 0, 1], [4, 3, 0], [1, 1, 0]], np.int32),
                           np.array([[2.0, 1.0, 1.0], [0.0, 0.0, 4.0], [0.5, 3.5, 0.0], [1.25, 2.75, 0.0]]),
                           np.array([[2.0, 1.0, 1.0], [0.0, 0.0, 4.0], [0.125, 2.000004, 0.0], [1.25, 2.75, 0.0]]), np.ones(4))
    prefix = str(tmp_path / "query_results")
    pp.write_q(prefix, s.hard, ["AFR", "EUR", "NAT"], ["s1", "NA.2"])
    pp.write_tracts(prefix, s, ["AFR", "EUR", "NAT"], ["s1", "NA.2"])
    assert open(prefix + ".Q").read() == (
        "#global ancestry, hard calls, weights: cM\n"
        "#sample\tAFR\tEUR\tNAT\n"
        "s1\t0.25000\t0.12500\t0.62500\n"
        "NA.2\t0.22839\t0.77161\t0.00000\n")
    assert open(prefix + ".tracts.tsv").read() == (
        "sample\thaplotype\tancestry\tn_tracts\ttotal_cM\tlongest_cM\tmean_cM\n"
        "s1\t0\tAFR\t1\t2.00000\t2.00000\t2.00000\n"
        "s1\t0\tEUR\t1\t1.00000\t1.00000\t1.00000\n"
        "s1\t0\tNAT\t1\t1.00000\t1.00000\t1.00000\n"
        "s1\t1\tAFR\t0\t0.00000\t0.00000\t0.00000\n"
        "s1\t1\tEUR\t0\t0.00000\t0.00000\t0.00000\n"
        "s1\t1\tNAT\t1\t4.00000\t4.00000\t4.00000\n"
        "NA.2\t0\tAFR\t4\t0.50000\t0.12500\t0.12500\n"
        "NA.2\t0\tEUR\t3\t3.50000\t2.00000\t1.16667\n"
        "NA.2\t0\tNAT\t0\t0.00000\t0.00000\t0.00000\n"
        "NA.2\t1\tAFR\t1\t1.25000\t1.25000\t1.25000\n"
        "NA.2\t1\tEUR\t1\t2.75000\t2.75000\t2.75000\n"
        "NA.2\t1\tNAT\t0\t0.00000\t0.00000\t0.00000\n")
    with pytest.raises(ValueError):
        pp.write_q(prefix, s.hard[:3], ["AFR", "EUR", "NAT"], ["s1", "NA.2"])


def test_symbols_bindings_and_the_config_default():
    """both entries are declared, exported and typed as the header states them; the ABI version is unchanged; the file path writes the
    two files only when asked to"""
    from gnomix_amd import _lib, cli, multi
    from gnomix_amd.gnomix import HipGnomix
    from gnomix_amd.model import DeviceModel
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gnomix_hip.h")).read(), flags=re.S)
    ctype = {"gnx_ctx*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "const void*": C.c_void_p, "const double*": C.c_void_p,
             "double*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}
    for name in ("gnx_ancestry_summary", "gnx_ancestry_summary_dev"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        types = [re.sub(r"\s*\b\w+$", "", re.sub(r"\s+", " ", p.strip())).replace(" *", "*") for p in m.group(1).split(",")]
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and [ctype[t] for t in types] == list(args), name
        assert getattr(lib, name).argtypes == args
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16      # the ABI only grew
    assert re.search(r"#define\s+GNX_SUMMARY_MAX_A\s+32\b", hdr) and re.search(r"#define\s+GNX_SUMMARY_MAX_W\s+8192\b", hdr)
    assert inspect.signature(cli.run_inference).parameters["global_ancestry_output"].default is False
    assert inspect.signature(cli._run_and_write).parameters["global_ancestry_output"].default is False
    for owner in (DeviceModel, multi.DeviceGroup):
        assert callable(getattr(owner, "ancestry_summary"))
    assert callable(DeviceModel.ancestry_summary_device) and callable(HipGnomix.global_ancestry)
    src = open(os.path.join(ROOT, "gnomix_amd", "cli.py")).read()
    assert src.count('inf.get("global_ancestry_output")') == 2      # both command-line routes read the key, absent = off
