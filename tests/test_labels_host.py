"""CPU-side tests of the label outputs: the plain-Python restatement of the mode filter against the reference's results (G28), the
native .lai / .bed writers byte for byte against postprocess.msp_to_lai / msp_to_bed (and against the files the reference wrote),
their error returns, the .gnx field and the new prototypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import labels_exact as LE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g28():
    return load_golden("G28_mode_filter.npz")


def test_restatement_equals_the_reference_on_every_case(g28):
    n = int(g28["n_cases"])
    assert n >= 20
    changed = 0
    for k in range(n):
        lab, size, ref = g28["c%d_in" % k], int(g28["c%d_size" % k]), g28["c%d_out" % k]
        got = LE.mode_filter(lab, size)
        assert np.array_equal(got, ref), k
        e = size // 2
        if e:
            assert np.array_equal(got[:, :e], lab[:, :e]) and np.array_equal(got[:, lab.shape[1] - e:], lab[:, lab.shape[1] - e:]), k
        changed += int(not np.array_equal(ref, lab))
    assert changed >= 8   # the fixture is not a list of identities


def test_restatement_of_the_run_list():
    lab = np.array([[1, 1, 1, 1], [0, 1, 0, 1], [2, 2, 0, 0]])
    counts, off, tr = LE.label_runs(lab)
    assert counts.tolist() == [1, 4, 2] and off.tolist() == [0, 1, 5, 7]
    assert tr.tolist() == [[0, 3, 1], [0, 0, 0], [1, 1, 1], [2, 2, 0], [3, 3, 1], [0, 1, 2], [2, 3, 0]]


def _query(n_samples, tmp_path, dotted=True):
    """a small .msp written by the library: W = 5 with a remainder window, one haplotype that is a single run, one that changes
    at every window; -> (meta, labels, positions, samples, pops, msp prefix)"""
    from gnomix_amd import postprocess as pp
    C_, M = 57, 11                                   # W = 5, the last window takes the 2 remaining SNPs
    model_pos = 1000 + 13 * np.arange(C_)
    query_pos = np.concatenate([[400, 990], model_pos[::2] + 1, [5000, 5001]])
    gm_pos, gm_cm = np.array([900, 1300, 1900]), np.array([0.0, 0.71, 2.5])
    meta = pp.get_meta_data("22", model_pos, query_pos, 5, M, gm_pos, gm_cm)
    rng = np.random.RandomState(n_samples)
    labels = rng.randint(0, 3, size=(2 * n_samples, 5)).astype(np.int32)
    labels[0] = 2
    labels[1] = [0, 1, 0, 1, 2]
    labels[-1, 1] = 11                               # a two-digit label
    samples = ["S%d" % i for i in range(n_samples)]
    if dotted:
        samples[1] = "NA.1.x"
    pops = ["P%d" % i for i in range(12)]
    prefix = str(tmp_path / ("q%d" % n_samples))
    pp.write_msp(prefix, meta, labels, pops, samples)
    return meta, labels, query_pos, samples, pops, prefix


@pytest.mark.parametrize("n_samples", [3, 4])
def test_write_lai_equals_msp_to_lai(tmp_path, n_samples):
    from gnomix_amd import postprocess as pp
    meta, labels, pos, samples, pops, prefix = _query(n_samples, tmp_path)
    pp.msp_to_lai(prefix + ".msp", pos, prefix + "_ref.lai")
    for nt in (0, 1, 3):
        pp.write_lai(prefix, meta, labels, pos, samples, populations=pops, n_threads=nt)
        assert open(prefix + ".lai", "rb").read() == open(prefix + "_ref.lai", "rb").read(), nt
    assert len(open(prefix + ".lai").read().splitlines()) == 2 + len(pos)


@pytest.mark.parametrize("n_samples", [3, 4])
@pytest.mark.parametrize("named", [True, False])
def test_write_bed_equals_msp_to_bed(tmp_path, n_samples, named):
    from gnomix_amd import postprocess as pp
    meta, labels, pos, samples, pops, prefix = _query(n_samples, tmp_path)
    ref, got = str(tmp_path / "bed_ref"), str(tmp_path / "bed")
    pp.msp_to_bed(prefix + ".msp", ref, pop_order=pops if named else None)
    _, off, tr = LE.label_runs(labels)
    pp.write_bed_runs(got, meta, off, tr, samples, pop_order=pops if named else None, n_threads=3)
    names = sorted(os.listdir(ref))
    assert names == sorted(os.listdir(got)) and len(names) == 2 * n_samples and "NA_1_x_0.bed" in names
    for n in names:
        assert open(os.path.join(got, n), "rb").read() == open(os.path.join(ref, n), "rb").read(), n
    assert len(open(os.path.join(got, "S0_0.bed")).read().splitlines()) == 2      # the single run
    assert len(open(os.path.join(got, "S0_1.bed")).read().splitlines()) == 6      # a run per window


def test_writers_equal_the_files_the_reference_wrote(tmp_path, g28):
    """the same writers against src/postprocess.py's own msp_to_lai / msp_to_bed output (stored by the fixture generator)"""
    from gnomix_amd import postprocess as pp
    if "w_lai" not in g28.files:
        pytest.skip("the fixture was generated without pandas: the reference's writers did not run")
    meta = {"chm": [str(c) for c in g28["w_chm"]], "spos": g28["w_spos"], "epos": g28["w_epos"], "sgpos": g28["w_sgpos"],
            "egpos": g28["w_egpos"], "n snps": g28["w_nsnps"]}
    labels, samples, pops = g28["w_labels"], [str(s) for s in g28["w_samples"]], [str(p) for p in g28["w_pops"]]
    prefix = str(tmp_path / "q")
    pp.write_msp(prefix, meta, labels, pops, samples)
    assert open(prefix + ".msp", "rb").read() == g28["w_msp"].tobytes()
    pp.write_lai(prefix, meta, labels, g28["w_positions"], samples, populations=pops)
    assert open(prefix + ".lai", "rb").read() == g28["w_lai"].tobytes()
    _, off, tr = LE.label_runs(labels)
    pp.write_bed_runs(str(tmp_path / "bed"), meta, off, tr, samples, pop_order=pops)
    names = [str(n) for n in g28["w_bed_names"]]
    assert sorted(os.listdir(str(tmp_path / "bed"))) == names
    for i, n in enumerate(names):
        assert open(os.path.join(str(tmp_path / "bed"), n), "rb").read() == g28["w_bed_%d" % i].tobytes(), n


def test_writer_error_returns(tmp_path):
    from gnomix_amd import _lib, postprocess as pp
    meta, labels, pos, samples, pops, prefix = _query(3, tmp_path)
    with pytest.raises(_lib.GnxError, match="add up to"):            # the reference's assert sum(n snps) == len(positions)
        pp.write_lai(prefix + "_bad", meta, labels, pos[:-1], samples, populations=pops)
    assert not os.path.exists(prefix + "_bad.lai")
    blocker = tmp_path / "a_file"
    blocker.write_text("x")
    with pytest.raises(_lib.GnxError, match="cannot open"):          # a directory nothing can be created in
        pp.write_lai(str(blocker / "q"), meta, labels, pos, samples, populations=pops)
    _, off, tr = LE.label_runs(labels)
    lib = _lib.load()
    cb, co = pp._blob([s for r in pp._meta_strings(meta) for s in r[:5]])
    fb, fo = pp._blob(["h%d.bed" % i for i in range(labels.shape[0])])
    head = b"chm\n"

    def bed(root, triples, n_anc=0):
        ab, ao = pp._blob(["P%d" % i for i in range(n_anc)])
        return lib.gnx_write_bed(root.encode(), fb, fo.ctypes.data, head, len(head), cb, co.ctypes.data, ab, ao.ctypes.data, n_anc,
                                 off.ctypes.data, triples.ctypes.data, labels.shape[0], 5, 2)
    assert bed(str(blocker / "sub"), tr) == _lib.GNX_EINVAL and b"cannot open" in lib.gnx_io_last_error()
    good = tmp_path / "good"
    good.mkdir()
    assert bed(str(good), tr) == _lib.GNX_OK and len(os.listdir(str(good))) == labels.shape[0]
    far = tr.copy()
    far[0, 1] = 5                                                     # a run that ends past the last window indexes nothing
    assert bed(str(good), far) == _lib.GNX_EINVAL and b"outside" in lib.gnx_io_last_error()
    assert bed(str(good), tr, n_anc=3) == _lib.GNX_EINVAL and b"no name" in lib.gnx_io_last_error()   # label 11 of 3 populations


def test_gnx_keeps_mode_filter_and_old_archives_are_unchanged(tmp_path):
    from gnomix_amd import synth, GnxModelData
    d = synth.synthetic_model(C=337, M=50, A=3, S=5, n_rounds=2, seed=1)
    assert d.mode_filter is None
    d.save(str(tmp_path / "a.gnx"))
    assert "mode_filter" not in np.load(str(tmp_path / "a.gnx")).files     # nothing new in an archive that does not use it
    assert GnxModelData.load(str(tmp_path / "a.gnx")).mode_filter is None
    d.mode_filter = 5
    d.save(str(tmp_path / "b.gnx"))
    e = GnxModelData.load(str(tmp_path / "b.gnx"))
    assert e.mode_filter == 5 and isinstance(e.mode_filter, int)


def test_converter_hands_the_references_mode_filter_on():
    """from_reference_model reads smooth.mode_filter (0 / False / None: off)"""
    import inspect
    from gnomix_amd import convert
    src = inspect.getsource(convert.from_reference_model)
    assert "mode_filter" in src
    from gnomix_amd.gnomix import HipGnomix
    assert "mode_filter" in inspect.signature(HipGnomix.__init__).parameters


def test_new_prototypes_and_bindings():
    """the four device entries and the two writers are declared, exported and typed as the headers state them"""
    from gnomix_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read() + open(os.path.join(ROOT, "include", "gnomix_io.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    ctype = {"gnx_ctx*": C.c_void_p, "const char*": (C.c_char_p, C.c_void_p), "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p,
             "const int64_t*": C.c_void_p, "int64_t*": (C.c_void_p, C.POINTER(C.c_int64)), "int64_t": C.c_int64, "int32_t": C.c_int32,
             "int": C.c_int}
    for name in ("gnx_mode_filter", "gnx_mode_filter_dev", "gnx_label_runs", "gnx_label_runs_dev", "gnx_write_lai", "gnx_write_bed"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == len(types), name
        for t, a in zip(types, args):
            want = ctype[t]
            assert a in (want if isinstance(want, tuple) else (want,)), (name, t, a)
        assert getattr(lib, name).argtypes == args
    assert lib.gnx_abi_version() == _lib.GNX_ABI_VERSION == 16      # the ABI only grew
    assert re.search(r"#define\s+GNX_MODE_FILTER_MAX_A\s+32\b", hdr) and re.search(r"#define\s+GNX_MODE_FILTER_LDS_ROW\s+16384\b", hdr)
