"""gnx_mode_filter[_dev] and gnx_label_runs[_dev] (csrc/labels/k_labels.hip) on the MI355X against the plain-Python restatement
(tests/labels_exact.py) and the reference's own results (G28), at every size where the kernels change path, and mode_filter through
HipSmoother / HipGnomix and the file path.  The restatement is slow Python: its results are computed once per input and shared."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_golden
import labels_exact as LE

pytestmark = pytest.mark.gpu

TILE = 256            # threads of a k_mode_filter workgroup = output positions it takes per step
LDS_ROW = 16384       # GNX_MODE_FILTER_LDS_ROW: a longer row is read from global memory
_want = {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _labels(N, W, A, seed=0):
    """rows of runs with scattered single-window flips (what a smoother's argmax looks like), drawn once per shape"""
    rng = np.random.RandomState(seed + 7 * N + W + 1000 * A)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 4 + 1)), 4, axis=1)[:, :W]
    flips = rng.rand(N, W) < 0.25
    lab[flips] = rng.randint(0, A, size=int(flips.sum()))
    return np.ascontiguousarray(lab, dtype=np.int32)


def _expected(N, W, A, size):
    key = (N, W, A, size)
    if key not in _want:
        lab = _labels(N, W, A)
        _want[key] = (lab, LE.mode_filter(lab, size))
    return _want[key]


def _filter_dev(ctx, lab, A, size, pad=0):
    """gnx_mode_filter_dev on a CUDA tensor whose rows lie `pad` elements further apart than W"""
    import torch
    from gnomix_amd import resident
    N, W = lab.shape
    buf = torch.full((N, W + pad), -7, dtype=torch.int32, device="cuda")
    buf[:, :W] = torch.from_numpy(lab).cuda()
    out = torch.full((N, W + 2 * pad), -9, dtype=torch.int32, device="cuda")
    with resident.torch_stream(ctx):
        rc = ctx.lib.gnx_mode_filter_dev(ctx.h, buf.data_ptr(), W + pad, out.data_ptr(), W + 2 * pad, N, W, A, size)
        torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, W:] == -9).all()            # nothing is written between the rows
    return rc, o[:, :W]


# W = 1; W = 2 ends and 2 ends + 1 (sizes 3, 5 and the even 4); W = 7 size 3; one more than a workgroup's 256 positions; N = 1 and N
# that no rows-per-workgroup count divides; A = 2 and A = 32; a row one label longer than the LDS tile (the global-memory path)
SHAPES = [(3, 1, 3, 3), (3, 2, 3, 3), (3, 3, 3, 3), (5, 4, 4, 5), (5, 5, 4, 5), (5, 4, 4, 4), (5, 5, 4, 4), (4, 7, 4, 3), (1, 7, 3, 3),
          (1, TILE + 1, 5, 5), (7, TILE + 1, 5, 5), (1031, 61, 7, 5), (67, 317, 2, 5), (67, 317, 32, 7), (13, 317, 5, 6),
          (2, LDS_ROW, 3, 5), (3, LDS_ROW + 1, 3, 5), (1, LDS_ROW + 1, 32, 4), (4, 40, 3, 1), (4, 40, 3, 0), (4, 40, 3, 40), (4, 40, 3, 41),
          (4, 40, 3, 1 << 40)]


@pytest.mark.parametrize("N,W,A,size", SHAPES)
def test_mode_filter_equals_the_restatement(ctx, N, W, A, size):
    from gnomix_amd import postprocess as pp
    lab, want = _expected(N, W, A, size)
    if size in (3, 5) and W > 2 * (size // 2) + 8:
        assert not np.array_equal(want, lab)                 # the case filters something
    if size // 2 == 0 or 2 * (size // 2) >= W:
        assert np.array_equal(want, lab)
    got = pp.mode_filter(ctx, lab, A, size)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for pad in (0, 5):
        rc, dev = _filter_dev(ctx, lab, A, size, pad)
        assert rc == 0 and np.array_equal(dev, want), pad


def test_mode_filter_equals_the_reference_on_g28(ctx):
    from gnomix_amd import postprocess as pp
    g = load_golden("G28_mode_filter.npz")
    for k in range(int(g["n_cases"])):
        lab, size, A = g["c%d_in" % k], int(g["c%d_size" % k]), int(g["c%d_A" % k])
        assert np.array_equal(pp.mode_filter(ctx, lab, A, size), g["c%d_out" % k]), k
        rc, dev = _filter_dev(ctx, np.ascontiguousarray(lab), A, size, pad=3)
        assert rc == 0 and np.array_equal(dev, g["c%d_out" % k]), k


@pytest.mark.parametrize("W", [40, LDS_ROW + 1])
def test_mode_filter_reports_labels_out_of_range(ctx, W):
    """well-formed memory, malformed values: a label that is no class is compared, never used as an index"""
    from gnomix_amd import _lib
    lab = _labels(3, W, 4).copy()
    lab[1, 17], lab[2, 3] = 4, -1
    out = np.empty_like(lab)
    rc = ctx.lib.gnx_mode_filter(ctx.h, lab.ctypes.data, out.ctypes.data, 3, W, 4, 5)
    assert rc == _lib.GNX_EINVAL and b"outside [0, 4)" in ctx.lib.gnx_last_error(ctx.h)
    assert out[1, 17] == 4 and out[2, 3] == -1 and np.array_equal(out[0], LE.mode_filter(lab[:1], 5)[0])
    rc, _ = _filter_dev(ctx, lab, 4, 5)
    assert rc == _lib.GNX_EINVAL
    assert ctx.lib.gnx_mode_filter(ctx.h, lab.ctypes.data, out.ctypes.data, 3, W, 4, -3) == _lib.GNX_EINVAL      # before the launch
    assert ctx.lib.gnx_mode_filter(ctx.h, lab.ctypes.data, out.ctypes.data, 3, W, 33, 3) == _lib.GNX_EUNSUPPORTED


# ---------------------------------------------------------------- through the plugin interface ----------------------------------
@pytest.fixture(scope="module")
def model(ga):
    """a logistic base with a tree smoother, isotonic maps that reorder the classes, inputs and the unfiltered labels of every form"""
    from gnomix_amd import synth
    d = synth.synthetic_model(C=3037, M=50, A=4, S=11, n_rounds=4, seed=5)
    xs = np.linspace(0.0, 1.0, 6)
    d.calib_off = (np.arange(d.A + 1) * 6).astype(np.int32)
    d.calib_x = np.tile(xs, d.A)
    d.calib_y = np.concatenate([np.clip(xs ** (0.4 + 0.7 * a), 0, 1) for a in range(d.A)])
    X = synth.synthetic_X(26, d.C, seed=3)
    g0 = ga.HipGnomix(d, device=0)
    B = g0.base.predict_proba(X)
    plain = {}
    for cal in (False, True):
        g0.smooth.calibrate = cal
        plain[cal] = (g0.smooth.predict(B), g0.predict(X))
    g0.smooth.calibrate = False
    assert not np.array_equal(plain[False][0], plain[True][0])       # the calibrator moves labels: both routes are worth checking
    return d, X, B, plain


@pytest.mark.parametrize("cal", [False, True])
@pytest.mark.parametrize("k", [3, 5, 0])
def test_predict_applies_the_filter_after_the_argmax(ga, model, k, cal):
    import torch
    d, X, B, plain = model
    g = ga.HipGnomix(d, device=0, calibrate=cal, mode_filter=k)
    assert g.smooth.mode_filter == k and bool(g.smooth.calibrate) == cal
    want_s, want_g = LE.mode_filter(plain[cal][0], k), LE.mode_filter(plain[cal][1], k)
    if k:
        assert not np.array_equal(want_s, plain[cal][0])             # the filter changes these labels
    got = g.smooth.predict(B)
    assert got.dtype == np.int64 and np.array_equal(got, want_s)
    got = g.predict(X)
    assert got.dtype == np.int64 and np.array_equal(got, want_g)
    got = g.smooth.predict(torch.from_numpy(B).cuda())
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want_s)
    got = g.predict(torch.from_numpy(X).cuda())
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want_g)
    p = g.smooth.predict_proba(B)                                    # untouched by the filter
    g.smooth.mode_filter = 0
    assert np.array_equal(p, g.smooth.predict_proba(B)) and np.array_equal(g.smooth.predict(B), plain[cal][0])


def test_model_data_and_none_switch_the_filter(ga, model):
    import dataclasses
    d, X, B, plain = model
    d5 = dataclasses.replace(d, mode_filter=5)
    assert ga.HipGnomix(d5, device=0).smooth.mode_filter == 5
    for off in (0, False):
        g = ga.HipGnomix(d5, device=0, mode_filter=off)
        assert not g.smooth.mode_filter and np.array_equal(g.predict(X), plain[False][1])
    g = ga.HipGnomix(d, device=0)
    g.smooth.mode_filter = None
    assert np.array_equal(g.smooth.predict(B), plain[False][0])


def test_phase_refuses_a_filter(ga, model):
    d, X, B, _ = model
    g = ga.HipGnomix(d, device=0, mode_filter=3)
    with pytest.raises(NotImplementedError, match="mode_filter"):
        g.phase(X[:4])


def test_file_path_filters_the_msp_and_leaves_the_fb(ga, model, tmp_path):
    """a .gnx that stores mode_filter, read back and run on a query file: the .msp holds the filtered labels, the .fb is unchanged;
    .lai and .bed (from the labels in memory) equal what msp_to_lai / msp_to_bed make of that .msp"""
    import dataclasses
    from gnomix_amd import synth, vcfio, cli, postprocess as pp
    d, X, _, plain = model
    d = dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                            population_order=["P%d" % a for a in range(d.A)], gen_map_pos=np.array([1, 50_000, 200_000]),
                            gen_map_cm=np.array([0.0, 1.5, 9.25]))
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    outs = {}
    for k in (0, 5):
        path = str(tmp_path / ("m%d.gnx" % k))
        dataclasses.replace(d, mode_filter=k or None).save(path)
        g = ga.HipGnomix.load(path, device=0)
        assert (g.smooth.mode_filter or 0) == k
        od = tmp_path / ("out%d" % k)
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": False}, g, snp_level=True,
                          bed_file_output=True, verbose=False)
        outs[k] = od
        if k:
            with pytest.raises(NotImplementedError, match="mode_filter"):
                cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od / "ph"), "phase": True}, g, verbose=False)
    assert (outs[0] / "query_results.fb").read_bytes() == (outs[5] / "query_results.fb").read_bytes()
    vcf = vcfio.read_vcf(q, chm="22")
    meta = pp.get_meta_data("22", d.snp_pos, vcf["variants/POS"], d.W, d.M, d.gen_map_pos, d.gen_map_cm)
    for k in (0, 5):
        pp.write_msp(str(tmp_path / ("want%d" % k)), meta, LE.mode_filter(plain[False][1], k), d.population_order, vcf["samples"])
        msp = outs[k] / "query_results.msp"
        assert msp.read_bytes() == (tmp_path / ("want%d.msp" % k)).read_bytes(), k
        pp.msp_to_lai(str(msp), vcf["variants/POS"], str(tmp_path / "ref.lai"))
        assert (outs[k] / "query_results.lai").read_bytes() == (tmp_path / "ref.lai").read_bytes(), k
        ref_bed = tmp_path / ("ref_bed%d" % k)
        pp.msp_to_bed(str(msp), str(ref_bed), pop_order=d.population_order)
        names = sorted(os.listdir(str(ref_bed)))
        assert names == sorted(os.listdir(str(outs[k] / "query_results_bed"))) and len(names) == X.shape[0]
        for n in names:
            assert (outs[k] / "query_results_bed" / n).read_bytes() == (ref_bed / n).read_bytes(), (k, n)
    assert (outs[0] / "query_results.msp").read_bytes() != (outs[5] / "query_results.msp").read_bytes()


# ---------------------------------------------------------------- the run list -------------------------------------------------
def _run_inputs(name):
    if name == "equal":
        return np.full((5, 70), 3, np.int32)
    if name == "alternating":
        return np.ascontiguousarray(np.tile(np.arange(131) % 2, (3, 1)) + np.arange(3)[:, None], dtype=np.int32)
    if name == "one_row":
        return _labels(1, 317, 5)
    if name == "one_window":
        return _labels(9, 1, 5)
    return _labels(1031, 317, 7)


@pytest.mark.parametrize("name", ["equal", "alternating", "random", "one_row", "one_window"])
def test_label_runs_equal_the_restatement(ctx, name):
    import torch
    from gnomix_amd import postprocess as pp, resident
    lab = _run_inputs(name)
    if name not in _want:
        _want[name] = LE.label_runs(lab)
    counts, off, tr = _want[name]
    N, W = lab.shape
    if name == "equal":
        assert counts.tolist() == [1] * N
    if name == "alternating":
        assert counts.tolist() == [W] * N
    got = pp.label_runs(ctx, lab)                     # (the first buffer holds 8 runs a row: "alternating" and "random" need the retry)
    assert np.array_equal(got[0], counts) and np.array_equal(got[1], off) and np.array_equal(got[2], tr)
    # device pointers, rows 3 elements further apart than W
    t = torch.full((N, W + 3), -5, dtype=torch.int32, device="cuda")
    t[:, :W] = torch.from_numpy(lab).cuda()
    d_counts = torch.zeros(N, dtype=torch.int64, device="cuda")
    d_off = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_tr = torch.full((len(tr) + 2, 3), -1, dtype=torch.int32, device="cuda")
    total = C.c_int64(-1)
    with resident.torch_stream(ctx):
        ctx.check(ctx.lib.gnx_label_runs_dev(ctx.h, t.data_ptr(), W + 3, N, W, d_counts.data_ptr(), d_off.data_ptr(), d_tr.data_ptr(),
                                             len(tr) + 2, C.byref(total)))
        torch.cuda.synchronize()
    assert total.value == len(tr) and np.array_equal(d_counts.cpu().numpy(), counts) and np.array_equal(d_off.cpu().numpy(), off)
    assert np.array_equal(d_tr.cpu().numpy()[:len(tr)], tr) and (d_tr.cpu().numpy()[len(tr):] == -1).all()


def test_label_runs_refuse_a_buffer_one_triple_too_small(ctx):
    from gnomix_amd import _lib
    lab = _run_inputs("alternating")
    counts, off, tr = LE.label_runs(lab)
    N, W = lab.shape
    c, o, total = np.zeros(N, np.int64), np.zeros(N + 1, np.int64), C.c_int64(0)
    buf = np.full((len(tr) - 1, 3), -1, np.int32)
    rc = ctx.lib.gnx_label_runs(ctx.h, lab.ctypes.data, W, N, W, c.ctypes.data, o.ctypes.data, buf.ctypes.data, len(tr) - 1, C.byref(total))
    assert rc == _lib.GNX_EINVAL and b"room for" in ctx.lib.gnx_last_error(ctx.h)
    assert total.value == len(tr) and np.array_equal(c, counts) and np.array_equal(o, off) and (buf == -1).all()
    buf = np.full((len(tr), 3), -1, np.int32)
    rc = ctx.lib.gnx_label_runs(ctx.h, lab.ctypes.data, W, N, W, c.ctypes.data, o.ctypes.data, buf.ctypes.data, len(tr), C.byref(total))
    assert rc == 0 and np.array_equal(buf, tr)
