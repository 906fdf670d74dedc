"""gnx_ancestry_summary[_dev] (csrc/summary/k_ancestry_summary.hip) on the MI355X against the restatement in the kernel's summation
order (tests/summary_exact.py), bit for bit, and the summaries through DeviceModel, HipGnomix.global_ancestry and the file path.

Shapes.  Lane c of a wave owns the windows [c L, (c + 1) L) with L = ceil(W / 64): W = 1, 2 (most lanes own nothing), 63, 64, 65
(L steps from 1 to 2: half the lanes own nothing), 129 (L = 3, the last chunk ragged), 1000 (L = 16, ragged).  Four rows per workgroup:
N = 2 (a workgroup with idle waves), 6 (a ragged second workgroup), 130.  The kernel has ONE path: no size switches to another one.
The restatement's results are computed once per input and shared."""
import ctypes as C
import os

import numpy as np
import pytest

import summary_exact as SE

pytestmark = pytest.mark.gpu

WS = [1, 2, 63, 64, 65, 129, 1000]
AS = [2, 3, 7, 32]
NS = [2, 6, 130]
KEYS = ("hard", "soft", "tract_count", "tract_total", "tract_longest")
_inputs, _want = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _case(N, W, A):
    """labels (N, W): row 0 constant, row 1 alternating, row 2 one run over every lane-chunk border but the first window, row 3 runs
    that start one window before every chunk border, the rest argmax of Dirichlet rows drawn in blocks; weights (cM-like, a few
    zeros); probabilities (N, W, A) Dirichlet"""
    key = (N, W, A)
    if key not in _inputs:
        rng = np.random.RandomState(N + 131 * W + 7 * A)
        P = rng.dirichlet(np.ones(A) * 0.4, size=(N, W))
        blocks = np.repeat(rng.dirichlet(np.ones(A) * 0.3, size=(N, W // 5 + 1)), 5, axis=1)[:, :W]
        lab = np.argmax(blocks + 0.35 * P, axis=2).astype(np.int32)
        L = (W + 63) // 64
        lab[0] = A - 1
        lab[1] = np.arange(W) % 2
        if N > 2:
            lab[2] = 1
            lab[2, 0] = 0
        if N > 3:
            lab[3] = ((np.arange(W) + 1) // L) % A
        w = rng.gamma(0.7, 0.3, size=W) + 1e-9
        w[rng.rand(W) < 0.1] = 0.0
        w[0] = 0.125
        _inputs[key] = (np.ascontiguousarray(lab), w, P)
    return _inputs[key]


def _expected(N, W, A, f32):
    key = (N, W, A, f32)
    if key not in _want:
        lab, w, P = _case(N, W, A)
        _want[key] = SE.summary(lab, w, A, P.astype(np.float32) if f32 else P)
    return _want[key]


def _same(got, want, soft=True):
    for k in KEYS:
        g = getattr(got, k)
        if k == "soft" and not soft:
            assert g is None
            continue
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        assert np.array_equal(g, want[k]), (k, np.argwhere(g != want[k])[:4].tolist())


def _device_call(ctx, lab, w, A, P=None, pad=3):
    """gnx_ancestry_summary_dev on CUDA tensors, the labels' rows `pad` elements further apart than W -> (rc, AncestrySummary)"""
    import torch
    from gnomix_amd import resident
    from gnomix_amd.postprocess import AncestrySummary
    N, W = lab.shape
    buf = torch.full((N, W + pad), -7, dtype=torch.int32, device="cuda")
    buf[:, :W] = torch.from_numpy(lab).cuda()
    Pt = torch.from_numpy(np.ascontiguousarray(P)).cuda() if P is not None else None
    new = lambda dt, v: torch.full((N, A), v, dtype=dt, device="cuda")
    hard, total, longest, count = new(torch.float64, -3.0), new(torch.float64, -3.0), new(torch.float64, -3.0), new(torch.int32, -3)
    soft = new(torch.float64, -3.0) if P is not None else None
    wv = np.ascontiguousarray(w, dtype=np.float64) if w is not None else None
    with resident.torch_stream(ctx):
        rc = ctx.lib.gnx_ancestry_summary_dev(ctx.h, buf.data_ptr(), W + pad, Pt.data_ptr() if Pt is not None else None,
                                              int(P is not None and P.dtype == np.float64), wv.ctypes.data if wv is not None else None,
                                              N, W, A, hard.data_ptr(), soft.data_ptr() if soft is not None else None, count.data_ptr(),
                                              total.data_ptr(), longest.data_ptr())
        torch.cuda.synchronize()
    return rc, AncestrySummary(hard, soft, count, total, longest, wv)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("W", WS)
def test_summary_equals_the_restatement_bit_for_bit(ctx, N, W, A):
    from gnomix_amd import postprocess as pp
    lab, w, P = _case(N, W, A)
    want64, want32 = _expected(N, W, A, False), _expected(N, W, A, True)
    assert want64["tract_count"][0].tolist() == [0] * (A - 1) + [1]                    # the constant row: one tract
    if W > 1:
        assert want64["tract_count"][1, :2].sum() == W                                 # the alternating row: W tracts
    host64 = pp.ancestry_summary(ctx, lab, A, w, P)                                    # host pointers, float64 probabilities
    _same(host64, want64)
    host32 = pp.ancestry_summary(ctx, lab, A, w, P.astype(np.float32))
    _same(host32, want32)
    _same(pp.ancestry_summary(ctx, lab, A, w), want64, soft=False)                     # labels only
    for Pd, want in ((P, want64), (P.astype(np.float32), want32)):                     # device pointers, strided rows
        rc, dev = _device_call(ctx, lab, w, A, Pd)
        assert rc == 0
        _same(dev, want)
    rc, again = _device_call(ctx, lab, w, A, P, pad=0)                                 # a second call: the same bits
    assert rc == 0
    _same(again, want64)


def test_no_weights_means_every_window_counts_the_same(ctx):
    from gnomix_amd import postprocess as pp
    lab, _, P = _case(6, 129, 3)
    want = SE.summary(lab, np.ones(129), 3, P)
    _same(pp.ancestry_summary(ctx, lab, 3, None, P), want)
    rc, dev = _device_call(ctx, lab, None, 3, P)
    assert rc == 0
    _same(dev, want)
    assert np.array_equal(want["tract_total"], np.stack([(lab == a).sum(axis=1) for a in range(3)], axis=1).astype(np.float64))


def _host_call(ctx, lab, ld, P, f64, w, N, W, A, outs, soft=True):
    hard, sft, cnt, tot, lng = outs
    return ctx.lib.gnx_ancestry_summary(ctx.h, lab.ctypes.data, ld, P.ctypes.data if P is not None else None, f64,
                                        w.ctypes.data if w is not None else None, N, W, A, hard.ctypes.data,
                                        sft.ctypes.data if soft else None, cnt.ctypes.data, tot.ctypes.data, lng.ctypes.data)


def test_argument_errors_write_nothing_and_the_context_goes_on(ctx):
    from gnomix_amd import _lib, postprocess as pp
    N, W, A = 6, 65, 3
    lab, w, P = _case(N, W, A)
    big = np.zeros((2, 8193), np.int32)

    def fresh(n=N, a=A):
        return [np.full((n, a), -3.0), np.full((n, a), -3.0), np.full((n, a), -3, np.int32), np.full((n, a), -3.0), np.full((n, a), -3.0)]

    def bad_w(i, v):
        x = w.copy()
        x[i] = v
        return x
    einval = {
        "N < 0": dict(N=-1), "W < 1": dict(W=0), "A < 1": dict(A=0), "ld < W": dict(ld=W - 1),
        "negative weight": dict(w=bad_w(7, -1e-300)), "infinite weight": dict(w=bad_w(64, np.inf)), "nan weight": dict(w=bad_w(0, np.nan)),
        "zero sum": dict(w=np.zeros(W)), "soft without proba": dict(P=None), "proba without soft": dict(soft=False),
    }
    for what, kw in einval.items():
        outs = fresh()
        a = dict(lab=lab, ld=W, P=P, f64=1, w=w, N=N, W=W, A=A, soft=True)
        a.update(kw)
        rc = _host_call(ctx, a["lab"], a["ld"], a["P"], a["f64"], a["w"], a["N"], a["W"], a["A"], outs, a["soft"])
        assert rc == _lib.GNX_EINVAL, what
        assert b"ancestry_summary" in ctx.lib.gnx_last_error(ctx.h), what
        assert all((o == -3).all() for o in outs), what
    # beyond the LDS plan: one class more than a staged label is compared with, one window more than a wave stages
    for what, (l, Wx, Ax) in {"A": (lab, W, 33), "W": (big, 8193, 3)}.items():
        outs = fresh(l.shape[0], Ax)
        rc = _host_call(ctx, l, Wx, None, 0, None, l.shape[0], Wx, Ax, outs, soft=False)
        assert rc == _lib.GNX_EUNSUPPORTED and len(ctx.lib.gnx_last_error(ctx.h)) > 20, what
        assert all((o == -3).all() for o in outs), what
    # the device form checks the same before it launches
    import torch
    from gnomix_amd import resident
    t = torch.from_numpy(lab).cuda()
    o = torch.full((N, A), -3.0, dtype=torch.float64, device="cuda")
    with resident.torch_stream(ctx):
        for kw in (dict(W=0), dict(A=33), dict(ld=W - 1)):
            a = dict(W=W, A=A, ld=W)
            a.update(kw)
            rc = ctx.lib.gnx_ancestry_summary_dev(ctx.h, t.data_ptr(), a["ld"], None, 0, None, N, a["W"], a["A"], o.data_ptr(), None, None, None, None)
            assert rc == (_lib.GNX_EUNSUPPORTED if "A" in kw else _lib.GNX_EINVAL), kw
        torch.cuda.synchronize()
    assert (o.cpu().numpy() == -3).all()
    outs = fresh()
    assert _host_call(ctx, lab, W, None, 0, w, 0, W, A, outs, soft=False) == 0 and all((x == -3).all() for x in outs)   # N == 0: nothing to do
    _same(pp.ancestry_summary(ctx, lab, A, w, P), _expected(N, W, A, False))                                            # the context still works
    _same(pp.ancestry_summary(ctx, big[:, :8192] + 1, 3, None), SE.summary(big[:, :8192] + 1, np.ones(8192), 3), soft=False)  # the longest row taken


def test_a_label_out_of_range_is_reported_after_the_launch(ctx):
    """well-formed memory, malformed values: such a label is compared, never used as an index; it counts for no class"""
    from gnomix_amd import _lib
    N, W, A = 6, 129, 3
    lab, w, P = _case(N, W, A)
    lab = lab.copy()
    lab[1, 17], lab[4, 128] = A, -1
    want = SE.summary(lab, w, A, P)
    clean = _expected(N, W, A, False)
    outs = [np.full((N, A), -3.0), np.full((N, A), -3.0), np.full((N, A), -3, np.int32), np.full((N, A), -3.0), np.full((N, A), -3.0)]
    rc = _host_call(ctx, lab, W, P, 1, w, N, W, A, outs)
    assert rc == _lib.GNX_EINVAL and b"outside [0, 3)" in ctx.lib.gnx_last_error(ctx.h)
    for k, o in zip(KEYS, outs):
        assert np.array_equal(o, want[k]), k
        assert np.array_equal(o[[0, 2, 3, 5]], clean[k][[0, 2, 3, 5]]), k          # the other rows are what they were
    rc, dev = _device_call(ctx, lab, w, A, P)
    assert rc == _lib.GNX_EINVAL
    _same(dev, want)


# ---------------------------------------------------------------- through the model ---------------------------------------------
@pytest.fixture(scope="module")
def model(ga):
    """a logistic base with a tree smoother and isotonic maps that reorder the classes (as tests/test_gpu_labels.py builds it)"""
    from gnomix_amd import synth
    d = synth.synthetic_model(C=3037, M=50, A=4, S=11, n_rounds=4, seed=5)
    xs = np.linspace(0.0, 1.0, 6)
    d.calib_off = (np.arange(d.A + 1) * 6).astype(np.int32)
    d.calib_x = np.tile(xs, d.A)
    d.calib_y = np.concatenate([np.clip(xs ** (0.4 + 0.7 * a), 0, 1) for a in range(d.A)])
    X = synth.synthetic_X(26, d.C, seed=3)
    return d, X


def _pairs(rows):
    return (rows[0::2] + rows[1::2]) / 2


@pytest.mark.parametrize("cal,mf", [(False, 0), (False, 5), (True, 0), (True, 5)])
def test_global_ancestry_follows_predict_and_predict_proba(ga, model, cal, mf):
    import torch
    d, X = model
    g = ga.HipGnomix(d, device=0, calibrate=cal, mode_filter=mf)
    lab, P = g.predict(X), g.predict_proba(X)
    if mf:
        assert not np.array_equal(lab, ga.HipGnomix(d, device=0, calibrate=cal, mode_filter=0).predict(X))     # the filter moves labels
    w = np.random.RandomState(4).gamma(0.7, 0.3, size=d.W)
    Xt = torch.from_numpy(X).cuda()
    for weights in (None, w):
        want = SE.summary(lab, np.ones(d.W) if weights is None else weights, d.A, P)
        hard, soft = g.global_ancestry(X, weights), g.global_ancestry(X, weights, soft=True)
        assert hard.shape == (X.shape[0] // 2, d.A) and hard.dtype == np.float64
        assert np.array_equal(hard, _pairs(want["hard"])) and np.array_equal(soft, _pairs(want["soft"]))
        hard_t, soft_t = g.global_ancestry(Xt, weights), g.global_ancestry(Xt, weights, soft=True)
        assert hard_t.is_cuda and soft_t.is_cuda and hard_t.dtype == torch.float64
        assert np.array_equal(hard_t.cpu().numpy(), _pairs(want["hard"])) and np.array_equal(soft_t.cpu().numpy(), _pairs(want["soft"]))
    s = g.dev.ancestry_summary(lab, w, P)
    st = g.dev.ancestry_summary_device(torch.from_numpy(lab).to(torch.int32).cuda(), w, torch.from_numpy(P).cuda())
    for k in KEYS:
        assert np.array_equal(getattr(s, k), getattr(st, k).cpu().numpy()), k
    with pytest.raises(ValueError, match="two"):
        g.global_ancestry(X[:3])


# ---------------------------------------------------------------- the file path ------------------------------------------------
def _read_msp(path):
    lines = open(path).read().splitlines()
    rows = [ln.split("\t") for ln in lines[2:]]
    lab = np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T
    cm = np.array([float(r[4]) for r in rows]) - np.array([float(r[3]) for r in rows])
    return np.ascontiguousarray(lab), cm


def _expected_files(msp, pops, samples):
    """the two files' text from the restatement run on the labels and the cM columns parsed back from the .msp"""
    lab, cm = _read_msp(msp)
    s = SE.summary(lab, cm, len(pops))
    q = _pairs(s["hard"])
    qt = "#global ancestry, hard calls, weights: cM\n#sample\t" + "\t".join(pops) + "\n"
    tt = "sample\thaplotype\tancestry\tn_tracts\ttotal_cM\tlongest_cM\tmean_cM\n"
    for i, name in enumerate(samples):
        qt += name + "\t" + "\t".join("%.5f" % v for v in q[i]) + "\n"
        for h in (0, 1):
            for a, pop in enumerate(pops):
                n, t, l = int(s["tract_count"][2 * i + h, a]), float(s["tract_total"][2 * i + h, a]), float(s["tract_longest"][2 * i + h, a])
                tt += "%s\t%d\t%s\t%d\t%.5f\t%.5f\t%.5f\n" % (name, h, pop, n, t, l, t / n if n else 0.0)
    return qt, tt


def test_file_path_writes_q_and_tracts_only_when_asked(ga, model, tmp_path):
    import dataclasses
    from gnomix_amd import synth, vcfio, cli
    from gnomix_amd.multi import DeviceGroup
    d, X = model
    pops = ["P%d" % a for a in range(d.A)]
    d = dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                            population_order=pops, gen_map_pos=np.array([1, 50_000, 200_000]), gen_map_cm=np.array([0.0, 1.5, 9.25]))
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    samples = [str(s) for s in vcfio.read_vcf(q, chm="22")["samples"]]
    g = ga.HipGnomix(d, device=0)

    def run(name, phase=False, devices=None, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, devices=devices, **kw)
        return od
    off, on = run("off"), run("on", global_ancestry_output=True)
    assert sorted(os.listdir(str(off))) == ["query_results.fb", "query_results.msp"]                  # the files it holds today
    assert sorted(os.listdir(str(on))) == ["query_results.Q", "query_results.fb", "query_results.msp", "query_results.tracts.tsv"]
    for f in ("query_results.fb", "query_results.msp"):
        assert (off / f).read_bytes() == (on / f).read_bytes()
    qt, tt = _expected_files(str(on / "query_results.msp"), pops, samples)
    assert (on / "query_results.Q").read_text() == qt and (on / "query_results.tracts.tsv").read_text() == tt
    assert len(qt.splitlines()) == 2 + len(samples) and len(tt.splitlines()) == 1 + 2 * len(samples) * d.A
    # phasing: the files follow Gnofix's labels
    ph = run("phased", phase=True, global_ancestry_output=True)
    assert (ph / "query_results.msp").read_bytes() != (on / "query_results.msp").read_bytes()
    qp, tp = _expected_files(str(ph / "query_results.msp"), pops, samples)
    assert (ph / "query_results.Q").read_text() == qp and (ph / "query_results.tracts.tsv").read_text() == tp and tp != tt
    # two contexts on one GPU: the same bytes
    with DeviceGroup(d, [0, 0], first=g.dev) as grp:
        assert len(grp.models) == 2
        two = run("two", devices=grp, global_ancestry_output=True)
    for f in sorted(os.listdir(str(on))):
        assert (two / f).read_bytes() == (on / f).read_bytes(), f
