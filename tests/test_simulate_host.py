"""Training mode's host side (gnomix_amd.simulate, cli.training_setup) against tests/golden/G21_sim, which the reference's own
simulator wrote (tests/golden/make_golden_sim.py): splits, chm_info, every split's and generation's X / ancestry / window labels, and
the bytes of the .npy files.  No GPU."""
import hashlib
import os

import numpy as np
import pytest
import yaml

from gnomix_amd import cli
from gnomix_amd import simulate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "G21_sim")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "expected.npz"))


@pytest.fixture(scope="module")
def config():
    with open(os.path.join(G, "config.yaml")) as f:
        return yaml.safe_load(f)


@pytest.fixture(scope="module")
def plan(config):
    return S.plan_splits(os.path.join(G, "panel.vcf.gz"), os.path.join(G, "gmap.tsv"), os.path.join(G, "smap.tsv"), config, chm="22")


def _anc_rows(g, key, C):
    off, st, val = g["anc_off_" + key], g["anc_start_" + key], g["anc_val_" + key]
    out = np.empty((len(off) - 1, C), np.uint8)
    for n in range(len(off) - 1):
        s = st[off[n]:off[n + 1]]
        ends = np.append(s[1:], C)
        for b, e, v in zip(s, ends, val[off[n]:off[n + 1]]):
            out[n, b:e] = v
    return out


def test_genetic_map_reader(tmp_path):
    p = tmp_path / "m.tsv"
    p.write_text("# comment\n22\t100\t0.0\n22\t200\t1.5\nchr7\t50\t0.1\n")
    df = S.read_genetic_map(str(p), "22")
    assert list(df["pos"]) == [100, 200] and list(df["pos_cm"]) == [0.0, 1.5]
    p.write_text("chr22\t100\t0.0\nchr22\t300\t2.5\n")           # "chr" + chm when chm itself is absent
    assert list(S.read_genetic_map(str(p), 22)["pos"]) == [100, 300]
    p.write_text("chm\tpos\tpos_cm\n22\t100\t0.0\n22\t400\t3.0\n")  # a header row: the second attempt reads it as one
    assert list(S.read_genetic_map(str(p), "22")["pos_cm"]) == [0.0, 3.0]
    p.write_text("a\tb\tc\nx\ty\tz\n")
    with pytest.raises(ValueError):
        S.read_genetic_map(str(p), "22")


def test_chm_info_and_window_size_bit_identical(plan, golden, config):
    assert plan.morgans == golden["morgans"]
    assert plan.bp.dtype == golden["bp"].dtype and np.array_equal(plan.bp, golden["bp"])
    assert plan.window_size(config["model"]["window_size_cM"]) == int(golden["M"])


def test_splits_identical_to_the_reference(plan, golden):
    assert list(plan.gens) == ["train1", "train2", "val"]
    for split in plan.gens:
        assert [plan.samples[r] for r in plan.split_rows[split]] == list(golden["split_" + split]), split
        assert plan.gens[split] == list(golden["gens_" + split])


def test_numpy_expansion_equals_the_reference_everywhere(plan, golden):
    M = int(golden["M"])
    X, Y, anc = S.simulate_numpy(plan, M)
    assert len(plan.parts) == 23
    for split, gen, h0, n in plan.parts:
        key = "%s_gen%d" % (split, gen)
        assert tuple(golden["shape_" + key]) == (n, plan.C), key
        assert np.array_equal(np.unpackbits(golden["X_" + key], axis=1)[:, :plan.C], X[h0:h0 + n]), key
        assert np.array_equal(_anc_rows(golden, key, plan.C), anc[h0:h0 + n]), key
        assert np.array_equal(golden["y_" + key], Y[h0:h0 + n]), key


def test_written_files_match_the_references_bytes(plan, golden, tmp_path):
    X, Y, anc = S.simulate_numpy(plan, int(golden["M"]))
    S.write_generated_data(plan, str(tmp_path), X, anc)
    for split, gen, _, _ in plan.parts:
        key = "%s_gen%d" % (split, gen)
        for fn in ("mat_vcf_2d", "mat_map"):
            with open(tmp_path / split / ("gen_%d" % gen) / (fn + ".npy"), "rb") as f:
                assert hashlib.sha256(f.read()).hexdigest() == str(golden["sha_%s_%s" % (key, fn)]), (key, fn)
    for split in plan.gens:
        with open(tmp_path / "sample_maps" / (split + ".map"), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == str(golden["sha_map_" + split])
    # ... and they read back as get_data reads them (metadata.pkl through the restricted unpickler)
    gens = {k: plan.gens[k] for k in plan.gens}
    data, meta = S.read_generated_data(str(tmp_path), gens, 1.0)
    assert meta["M"] == int(golden["M"]) and meta["pop_order"] == plan.pop_order and np.array_equal(meta["snp_pos"], plan.meta["pos_snps"])
    sl = plan.split_slices()
    for (Xs, ys), split in zip(data, ("train1", "train2", "val")):
        assert np.array_equal(Xs, X[sl[split][0]:sl[split][1]]) and np.array_equal(ys, Y[sl[split][0]:sl[split][1]])


def test_window_mode_ties_and_the_long_last_window():
    # C = 23, M = 5: windows [0,5) [5,10) [10,15) and the last [15,23) of M + rem = 8 SNPs
    anc = np.zeros((3, 23), np.uint8)
    anc[0, 0:2], anc[0, 2:4], anc[0, 4] = 2, 1, 0       # 2:2, 1:2, 0:1 -> tie between 1 and 2 -> 1
    anc[1, 15:19], anc[1, 19:23] = 3, 1                  # last window: 4 x 3, 4 x 1 -> 1
    anc[2, 15:20], anc[2, 20:23] = 2, 0                  # 5 x 2 beats 3 x 0 only when the last window is 8 long
    y = S.window_labels(anc, 5)
    assert y.shape == (3, 4)
    assert y[0, 0] == 1 and y[1, 3] == 1 and y[2, 3] == 2


def test_segments_follow_the_reference_rules(plan):
    off, b, s = plan.seg_off, plan.seg_begin, plan.seg_src
    assert off[0] == 0 and np.all(np.diff(off) >= 1) and np.all(b[off[:-1]] == 0)
    for n in range(plan.N):
        assert np.all(np.diff(b[off[n]:off[n + 1]]) > 0)
    assert np.all(plan.anc_of_src[s] < plan.A)
    # generation 0 = the split's founders themselves, maternal then paternal, in sample-map order
    split, gen, h0, n = plan.parts[0]
    assert (split, gen) == ("train1", 0) and n == 2 * len(plan.split_rows["train1"])
    assert list(s[off[h0:h0 + n]]) == [2 * int(plan.vcf_index[r]) + k for r in plan.split_rows["train1"] for k in (0, 1)]


def test_founder_values_other_than_0_1_are_rejected():
    F = np.array([[0, 1, 0, 1], [1, 1, 2, 0]], np.int8)
    with pytest.raises(ValueError, match="founder haplotype 1 holds 2 at SNP 2"):
        S.expand_numpy(F, np.array([0, 2]), np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.zeros(2, np.uint8), 4)


def test_small_panels_and_val_ratio_zero(config):
    smap = ([f"S{i:03d}" for i in range(20)], ["A", "B"] * 10)
    from gnomix_amd import vcfio
    panel = vcfio.read_vcf(os.path.join(G, "panel.vcf.gz"), chm="22")
    p = S.plan_splits(panel, os.path.join(G, "gmap.tsv"), smap, config, chm="22")     # <= 25 founders: no validation split
    assert list(p.gens) == ["train1", "train2"] and "val" not in p.split_slices()
    cfg = S.merge_config(config)
    cfg["simulation"]["splits"]["ratios"]["val"] = 0
    p = S.plan_splits(panel, os.path.join(G, "gmap.tsv"), os.path.join(G, "smap.tsv"), cfg, chm="22")
    assert list(p.gens) == ["train1", "train2"]
    assert p.num_outs == {"train1": 100, "train2": 18}                           # the 800 / 150 floors over 8 generations
    with pytest.raises(ValueError, match="'NOPE'"):
        S.plan_splits(panel, os.path.join(G, "gmap.tsv"), (["S000", "NOPE"], ["A", "B"]), config, chm="22")


def test_cli_training_arguments_and_config(tmp_path, capsys):
    out = str(tmp_path / "out")
    args = ["gnomix.py", "None", out, "22", "False", os.path.join(G, "gmap.tsv"), os.path.join(G, "panel.vcf.gz"), os.path.join(G, "smap.tsv")]
    base, cfg, err = cli.training_setup(args + [os.path.join(G, "config.yaml")])
    assert err is None and base["query_file"] is None and base["phase"] is False and base["chm"] == "22"
    assert cfg["model"]["smooth_size"] == 15 and cfg["model"]["window_size_cM"] == 1.0 and cfg["seed"] == 94305
    # defaults under a partial file
    c = tmp_path / "c.yaml"
    c.write_text("model:\n  inference: fast\n")
    base, cfg, err = cli.training_setup(args + [str(c)])
    assert err is None and cfg["model"]["smooth_size"] == 75 and cfg["simulation"]["r_admixed"] == 1 and cfg["model"]["inference"] == "fast"
    c.write_text("model:\n  inference: best\n")
    assert cli.main(args + [str(c)]) == 2
    assert "best" in capsys.readouterr().out
    assert cli.main(args[:5] + ["/nonexistent.vcf"] + args[6:] + [os.path.join(G, "config.yaml")]) == 2
    assert "not found" in capsys.readouterr().out
    assert not os.path.exists(out)                                                  # nothing written before the inputs check out
    assert cli.main(args + [str(tmp_path / "missing.yaml")]) == 2
    assert "Usage when training a model from scratch" in cli.USAGE
