"""CPU tests of the ancestry-partitioned polygenic scores: the restatement (tests/score_exact.py) on a hand-worked case and against
math.fsum within the derived bound, score.read_score_file on every rule, write_sscore's bytes, weights_from_assoc, the ABI symbols and
the command line's refusals."""
import collections
import ctypes
import os

import numpy as np
import pytest

import score_cases as SC
import score_exact as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 2 individuals (4 haplotypes), C = 5, M = 2, W = 2: window 0 = SNPs 0, 1; window 1 = SNPs 2, 3, 4.  A = 2, S = 1.
HW_X = np.array([[1, 0, 1, 1, 0],
                 [0, 0, 1, 2, 1],      # a missing call at SNP 3
                 [1, 1, 0, 0, 1],
                 [1, 0, 0, 1, 1]], np.int8)
HW_LAB = np.array([[0, 1], [0, 0], [1, 1], [0, 1]], np.int32)
HW_EFF = np.array([1, 0, 1, 1, 255], np.uint8)          # SNP 1: the effect allele is REF; SNP 4 is not scored
HW_W = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0], [16.0, 160.0]])[:, :, None]


def test_hand_worked_case():
    """individual 0: row 0 is ancestry 0 in window 0 (ALT at SNP 0: +1; REF at SNP 1: +2) and ancestry 1 in window 1 (ALT at 2 and 3:
    +40 +80); row 1 is ancestry 0 throughout (SNP 0 REF: no; SNP 1 REF: +2; SNP 2 ALT: +4; SNP 3 missing).  individual 1: row 2 is
    ancestry 1 (SNP 0 ALT: +10; SNP 1 ALT: no; SNPs 2, 3 REF: no); row 3 is ancestry 0 in window 0 (+1, +2) and 1 in window 1 (SNP 3: +80)"""
    for f in (SE.scores_literal, SE.scores):
        score, ne, ns, nm, n_bad = f(HW_X, HW_LAB, 2, 2, HW_W, HW_EFF)
        assert n_bad == 0
        assert score[:, :, 0].tolist() == [[1 + 2 + 2 + 4, 40 + 80], [1 + 2, 10 + 80]]
        assert ne.tolist() == [[4, 2], [2, 2]]
        assert ns.tolist() == [[5, 2], [2, 6]]       # called genotypes at scored SNPs under that ancestry
        assert nm.tolist() == [[1, 0], [0, 0]]
    fs, n_terms, mag = SE.score_fsum(HW_X, HW_LAB, 2, 2, HW_W, HW_EFF)
    assert np.array_equal(fs, score) and n_terms.tolist() == ne.tolist()
    # a label out of range counts for no ancestry at that window
    lab = HW_LAB.copy()
    lab[1, 1] = 2
    score, ne, ns, nm, n_bad = SE.scores(HW_X, lab, 2, 2, HW_W, HW_EFF)
    assert n_bad == 1 and score[:, :, 0].tolist() == [[1 + 2 + 2, 120], [3, 90]] and nm.tolist() == [[0, 0], [0, 0]]


SHAPES = [(4, 23, 5, 4, 3, 2), (6, 40, 1, 40, 2, 3), (2, 37, 10, 1, 7, 1), (8, 64, 16, 4, 4, 16)]


@pytest.mark.parametrize("N,C,M,W,A,S", SHAPES)
def test_vectorised_restatement_equals_the_literal_one_bit_for_bit(N, C, M, W, A, S):
    X, lab, w, eff = SC.case(N, C, M, W, A, S)
    lab[0, 0] = A                    # one label out of range
    lit, vec = SE.scores_literal(X, lab, M, A, w, eff), SE.scores(X, lab, M, A, w, eff)
    assert lit[4] == vec[4] == 1
    for a, b in zip(lit[:4], vec[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # the weights make the order visible: summing a window's SNPs in descending order gives other bits somewhere
    rev = SE.scores(X[:, ::-1], lab[:, ::-1], M, A, w[::-1], eff[::-1]) if C == M * W else None
    if rev is not None and C > 8:
        assert not np.array_equal(rev[0], vec[0]) and np.array_equal(rev[1], vec[1])


@pytest.mark.parametrize("N,C,M,W,A,S", SHAPES + [(4, 600, 100, 6, 2, 2)])
def test_restatement_against_fsum_within_the_derived_bound(N, C, M, W, A, S):
    X, lab, w, eff = SC.case(N, C, M, W, A, S, seed=1)
    score, ne = SE.scores(X, lab, M, A, w, eff)[:2]
    fs, n_terms, mag = SE.score_fsum(X, lab, M, A, w, eff)
    assert np.array_equal(n_terms, ne)
    assert (np.abs(score - fs) <= SE.bound(n_terms, mag)).all()


def _score_file(tmp_path, text, name="s.tsv"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_read_score_file_rules(tmp_path):
    from gnomix_amd import score
    pos, ref, alt, pops = [100, 200, 300, 400], ["A", "C", "G", "T"], ["C", "T", "A", "G"], ["AFR", "EUR"]
    head = "chm\tpos\teffect_allele\tprs\tlipid:EUR\tlipid:AFR\n"
    body = ("22\t100\tC\t0.5\t1\t2\n"          # ALT
            "22\t200\tC\t-0.25\t3\t4\n"        # REF
            "21\t300\tA\t9\t9\t9\n"            # another chromosome
            "22\t999\tA\t9\t9\t9\n"            # not in the model
            "22\t400\tA\t9\t9\t9\n")           # neither REF nor ALT
    w, eff, names, rep = score.read_score_file(_score_file(tmp_path, head + body), "22", pos, ref, alt, pops)
    assert names == ["prs", "lipid"] and w.shape == (4, 2, 2) and w.dtype == np.float64 and eff.dtype == np.uint8
    assert eff.tolist() == [1, 0, 255, 255]
    assert w[0].tolist() == [[0.5, 2.0], [0.5, 1.0]] and w[1].tolist() == [[-0.25, 4.0], [-0.25, 3.0]] and not w[2:].any()
    assert rep == {"scored": 2, "other_chm": 1, "not_in_model": 1, "allele_mismatch": 1}
    # a population without a column gets 0
    w, _, names, _ = score.read_score_file(_score_file(tmp_path, "chm\tpos\teffect_allele\tx:EUR\n22\t100\tC\t7\n"), "22", pos, ref, alt, pops)
    assert names == ["x"] and w[0].tolist() == [[0.0], [7.0]]
    bad = {
        "both ways": "chm\tpos\teffect_allele\tx\tx:EUR\n22\t100\tC\t1\t2\n",
        "both ways, reversed": "chm\tpos\teffect_allele\tx:EUR\tx\n22\t100\tC\t1\t2\n",
        "column twice": "chm\tpos\teffect_allele\tx:EUR\tx:EUR\n22\t100\tC\t1\t2\n",
        "unknown population": "chm\tpos\teffect_allele\tx:ASN\n22\t100\tC\t1\n",
        "header": "chr\tpos\teffect_allele\tx\n22\t100\tC\t1\n",
        "no weight column": "chm\tpos\teffect_allele\n22\t100\tC\n",
        "listed twice": "chm\tpos\teffect_allele\tx\n22\t100\tC\t1\n22\t100\tC\t1\n",
        "empty cell": "chm\tpos\teffect_allele\tx\ty\n22\t100\tC\t\t1\n",
        "NA": "chm\tpos\teffect_allele\tx\n22\t100\tC\tNA\n",
        "not finite": "chm\tpos\teffect_allele\tx\n22\t100\tC\tinf\n",
        "not a number": "chm\tpos\teffect_allele\tx\n22\t100\tC\tabc\n",
        "short line": "chm\tpos\teffect_allele\tx\ty\n22\t100\tC\t1\n",
        "empty file": "",
    }
    for what, text in bad.items():
        with pytest.raises(ValueError):
            score.read_score_file(_score_file(tmp_path, text, "bad.tsv"), "22", pos, ref, alt, pops)
            pytest.fail(what)
    # a bad cell on a row of another chromosome is not looked at; one on a position the model lacks is
    ok = "chm\tpos\teffect_allele\tx\n21\t100\tC\tNA\n22\t100\tC\t1\n"
    assert score.read_score_file(_score_file(tmp_path, ok), "22", pos, ref, alt, pops)[3]["other_chm"] == 1
    with pytest.raises(ValueError):
        score.read_score_file(_score_file(tmp_path, "chm\tpos\teffect_allele\tx\n22\t999\tC\tNA\n"), "22", pos, ref, alt, pops)


def test_write_sscore_bytes(tmp_path):
    from gnomix_amd import postprocess as pp
    score = np.array([[[0.1, -2.0], [0.2, 1e-300]], [[1 / 3, 0.0], [2.0 ** -60, 5.0]]])
    ne = np.array([[1, 2], [3, 4]], np.int32)
    res = pp.AncestryScores(score, ne, ne + 10, ne + 20)
    pp.write_sscore(str(tmp_path / "q"), res, ["prs", "lipid"], ["AFR", "EUR"], ["s0", "s1"])
    got = (tmp_path / "q.sscore.tsv").read_text()
    assert got == ("sample\tAFR.n_scored\tAFR.n_effect\tAFR.n_miss\tEUR.n_scored\tEUR.n_effect\tEUR.n_miss\tprs.AFR\tprs.EUR\tprs.total\t"
                   "lipid.AFR\tlipid.EUR\tlipid.total\n"
                   "s0\t11\t1\t21\t12\t2\t22\t0.1\t0.2\t0.30000000000000004\t-2.0\t1e-300\t-2.0\n"
                   "s1\t13\t3\t23\t14\t4\t24\t0.3333333333333333\t8.673617379884035e-19\t0.3333333333333333\t0.0\t5.0\t5.0\n")
    cells = [ln.split("\t") for ln in got.splitlines()[1:]]
    assert float(cells[1][7]) == 1 / 3 and float(cells[1][8]) == 2.0 ** -60          # repr reads back to the same float64
    with pytest.raises(ValueError):
        pp.write_sscore(str(tmp_path / "q"), res, ["prs"], ["AFR", "EUR"], ["s0", "s1"])
    avg = res.avg()
    assert avg.shape == (2, 2, 2) and avg[0, 0, 0] == 0.1 / 11
    none = pp.AncestryScores(score, ne, np.zeros((2, 2), np.int32), ne).avg()
    assert np.isnan(none).all()


def test_score_tables_shapes():
    from gnomix_amd import postprocess as pp
    w1 = np.arange(3.0)
    w, eff = pp.score_tables(w1, None, 3, 2)
    assert w.shape == (3, 2, 1) and w.flags.c_contiguous and w[:, 1, 0].tolist() == [0, 1, 2] and eff.tolist() == [1, 1, 1]
    assert pp.score_tables(np.ones((3, 2)), [1, 0, 255], 3, 2)[0].shape == (3, 2, 1)
    assert pp.score_tables(np.ones((3, 2, 20)), None, 3, 2)[0].shape == (3, 2, 20)
    assert pp.score_chunks(20) == [(0, 16), (16, 20)] and pp.score_chunks(16) == [(0, 16)]
    for bad_w, bad_e in ((np.ones(4), None), (np.ones((3, 3)), None), (np.ones((3, 2, 0)), None), (np.ones(3), [1, 0, 2]), (np.ones(3), [1, 0])):
        with pytest.raises(ValueError):
            pp.score_tables(bad_w, bad_e, 3, 2)


def test_weights_from_assoc():
    from gnomix_amd import assoc, score
    beta = np.array([[0.5, np.nan], [-1.0, 2.0], [np.inf, 3.0]])
    p = np.array([[0.01, 0.5], [0.2, np.nan], [0.001, 0.04]])
    z = np.zeros((3, 2))
    lin = assoc.AncestryAssoc(beta, z, z, p, z, z, z[:, 0], z[:, 0], z[:, 0], z[:, 0])
    assert score.weights_from_assoc(lin).tolist() == [[0.5, 0.0], [-1.0, 2.0], [0.0, 3.0]]
    assert score.weights_from_assoc(lin, p_max=0.05).tolist() == [[0.5, 0.0], [0.0, 0.0], [0.0, 3.0]]
    assert np.isnan(beta[0, 1])          # the result itself is left as it was
    Logit = collections.namedtuple("L", assoc.AncestryAssocLogit._fields)
    logit = Logit(**{f: (beta if f == "beta" else p if f == "p" else None) for f in Logit._fields})
    assert score.weights_from_assoc(logit, p_max=0.2).tolist() == [[0.5, 0.0], [-1.0, 0.0], [0.0, 3.0]]


def test_abi_symbols_are_built_and_declared():
    from gnomix_amd import _lib
    lib = _lib.load()
    for name, n_args in (("gnx_ancestry_score", 21), ("gnx_ancestry_score_dev", 21), ("gnx_ancestry_score_gt2", 15)):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int and len(_lib.SYMBOLS[name][1]) == n_args
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16
    hdr = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    assert "GNX_SCORE_MAX_S 16" in hdr and _lib.GNX_SCORE_MAX_S == 16
    for name in ("ancestry_scores", "ancestry_scores_device", "ancestry_scores_gt2"):
        from gnomix_amd.model import DeviceModel
        assert callable(getattr(DeviceModel, name))
    from gnomix_amd.gnomix import HipGnomix
    assert callable(HipGnomix.ancestry_scores)


def test_run_inference_refuses_the_key_with_phase_or_without_a_file_before_any_work(tmp_path):
    from gnomix_amd import cli
    args = {"query_file": str(tmp_path / "none.vcf"), "chm": "22", "output_basename": str(tmp_path), "phase": True}
    with pytest.raises(ValueError, match="ancestry_score_output with phase=True"):
        cli.run_inference(args, None, ancestry_score_output=True, score_file=str(tmp_path / "s.tsv"))
    with pytest.raises(ValueError, match="score_file"):
        cli.run_inference(dict(args, phase=False), None, ancestry_score_output=True)
    assert os.listdir(str(tmp_path)) == []
