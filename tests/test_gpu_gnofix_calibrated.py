"""Calibrated models on the GPU: Gnofix with the calibrate switch on (k_gnofix_opts' calibrated labelling mode) against the
REFERENCE's gnofix() run with its own calibrated Smoother (tests/golden/G26_gnofix_calibrated.npz, exact), the packed-row and file
forms against the int8 form, the dispatch with calibration off, the refusal that remains, and HipGnomix.train(calibrate=True) for
the CRF and CNN smoothers."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
FIXTURE = "G26_gnofix_calibrated.npz"


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _data(ga, g, name, calibrator=True):
    W, A, S, Cn = (int(g[name + k]) for k in ("_W", "_A", "_S", "_C"))
    t = name + "_t_"
    d = ga.GnxModelData(C=Cn, M=Cn // W, A=A, S=S, context=0, smooth_kind="xgb", tree_off=g[t + "tree_off"], left=g[t + "left"],
                        right=g[t + "right"], feat=g[t + "feat"], cond=g[t + "cond"], tree_class=g[t + "tree_class"],
                        base_score=float(g[t + "base_score"]))
    if calibrator:
        d.calib_off, d.calib_x, d.calib_y, d.calib_is_f32 = g[name + "_calib_off"], g[name + "_calib_x"], g[name + "_calib_y"], True
    return d


@pytest.fixture(scope="module")
def models(ga):
    """per geometry: the fixture and ONE calibrated device model (calibrate switch on)"""
    g = load_golden(FIXTURE)
    out = {}
    for n in g["geoms"]:
        dev = ga.DeviceModel(_data(ga, g, str(n)))
        dev.set_calibrate(True)
        out[str(n)] = dev
    return g, out


def _cases():
    g = load_golden(FIXTURE)
    return [(str(n), k) for n in g["geoms"] for k in range(len(g[str(n) + "_cases"]))]


def _ex(dev, X, B, opt):
    """gnx_gnofix_ex itself, the default option set included (DeviceModel.gnofix would take gnx_gnofix for it)"""
    from gnomix_amd import _lib
    o = _lib.gnofix_opts(**opt)
    X1 = X.copy()
    Y, nsw = np.full((X.shape[0], dev.W), -7, np.int32), np.full((X.shape[0] // 2,), -7, np.int32)
    dev.ctx.check(dev.lib.gnx_gnofix_ex(dev.h, X1.ctypes.data, X1.shape[1], B.ctypes.data, X1.shape[0] // 2, C.byref(o), Y.ctypes.data,
                                        nsw.ctypes.data))
    return X1, Y, nsw


@pytest.mark.parametrize("form", ["ex", "phase", "dev"])
@pytest.mark.parametrize("name,k", _cases())
def test_G26_equals_the_references_calibrated_gnofix(ga, models, name, k, form):
    """X, Y and the switch counts of every option set equal gnofix() with Smoother(calibrate=True, calibrator=fitted).  On the parent
    of this feature every one of these calls is GNX_EUNSUPPORTED."""
    import torch
    g, devs = models
    dev = devs[name]
    opt = json.loads(str(g[name + "_cases"][k]))
    X, B = g[name + "_X"], np.ascontiguousarray(g[name + "_B"])
    if form == "ex":
        Xo, Y, nsw = _ex(dev, X, B, opt)
    elif form == "phase":
        hip = ga.HipGnomix(_data(ga, g, name), calibrate=True)
        Xo, Y = hip.phase(X, B=B, **opt)
        nsw = None
    else:
        Xt, Bt = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(B).cuda()
        Yt, nt = dev.gnofix_device(Xt, Bt, **opt)
        Xo, Y, nsw = Xt.cpu().numpy(), Yt.cpu().numpy(), nt.cpu().numpy()
    assert np.array_equal(Xo, g["%s_%d_oX" % (name, k)])
    assert np.array_equal(Y, g["%s_%d_oY" % (name, k)])
    if nsw is not None:
        assert np.array_equal(nsw, g["%s_%d_nhist" % (name, k)] - 2)


def test_default_entry_points_take_the_calibrated_route(models):
    """gnx_gnofix and gnx_gnofix_dev (no options) on a calibrated model: the same reference results as gnx_gnofix_ex's defaults"""
    import torch
    g, devs = models
    for name, dev in devs.items():
        X, B = g[name + "_X"], np.ascontiguousarray(g[name + "_B"])
        max_it = json.loads(str(g[name + "_cases"][0]))["max_it"]
        Xo, Y, nsw = dev.gnofix(X, B, max_it=max_it)
        assert np.array_equal(Xo, g[name + "_0_oX"]) and np.array_equal(Y, g[name + "_0_oY"]) and np.array_equal(nsw, g[name + "_0_nhist"] - 2)
        Xt, Bt = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(B).cuda()
        Yt, nt = dev.gnofix_device(Xt, Bt, max_it=max_it)
        assert np.array_equal(Xt.cpu().numpy(), Xo) and np.array_equal(Yt.cpu().numpy(), Y) and np.array_equal(nt.cpu().numpy(), nsw)


def test_initial_labels_are_the_calibrated_ones(ga, models):
    """max_it = 0 returns the initial labels: HipSmoother.predict(B) with calibration on = the reference's Smoother.predict, and
    they differ from the raw arg-max"""
    g, devs = models
    for name, dev in devs.items():
        X, B = g[name + "_X"], np.ascontiguousarray(g[name + "_B"])
        sm = ga.HipSmoother(dev, calibrate=True)
        lab = sm.predict(B)
        assert np.array_equal(lab, g[name + "_Y0"]) and (lab != g[name + "_Y0raw"]).any()
        Xo, Y, nsw = dev.gnofix(X, B, max_it=0)
        assert np.array_equal(Y, lab) and np.array_equal(Xo, X) and not nsw.any()
        Xo, Y, nsw = _ex(dev, X, B, dict(max_it=0, prob_comp="prod"))
        assert np.array_equal(Y, lab) and np.array_equal(Xo, X) and not nsw.any()


def test_candidates_are_compared_by_raw_probabilities(models):
    """gnofix.py:157 asks smoother.model (never calibrated).  The fixture holds, for the defaults, the run of a smoother whose
    CANDIDATE probabilities are calibrated too; on the witness individuals it ends differently, and the kernel sides with the
    reference there"""
    g, devs = models
    dev = devs["a3"]
    wit = g["a3_raw_witness"]
    assert len(wit) > 0
    X, B = g["a3_X"], np.ascontiguousarray(g["a3_B"])
    Xo, Y, nsw = _ex(dev, X, B, json.loads(str(g["a3_cases"][0])))
    for i in wit:
        rows = slice(2 * i, 2 * i + 2)
        assert np.array_equal(Xo[rows], g["a3_0_oX"][rows]) and np.array_equal(Y[rows], g["a3_0_oY"][rows]) and nsw[i] == g["a3_0_nhist"][i] - 2
        assert not (np.array_equal(Xo[rows], g["a3_0_cX"][rows]) and np.array_equal(Y[rows], g["a3_0_cY"][rows]) and
                    nsw[i] == g["a3_0_cnhist"][i] - 2)


def test_packed_rows_equal_the_int8_form(models):
    import torch
    g, devs = models
    for name, dev in devs.items():
        X, B = g[name + "_X"], np.ascontiguousarray(g[name + "_B"])
        max_it = json.loads(str(g[name + "_cases"][0]))["max_it"]
        Xt, Bt = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(B).cuda()
        Pt = dev.pack_device(Xt)
        Yp, npk = dev.gnofix_packed_device(Pt, Bt, max_it=max_it)
        Y, ns = dev.gnofix_device(Xt, Bt, max_it=max_it)
        assert torch.equal(Yp, Y) and torch.equal(npk, ns) and torch.equal(Pt, dev.pack_device(Xt))
        assert np.array_equal(Y.cpu().numpy(), g[name + "_0_oY"])


def _trained_like_model(ga, calibrated):
    """a whole model (logistic base + tree smoother) with a calibrator fitted on the smoother's own probabilities and skewed labels"""
    from gnomix_amd import synth, calibrate
    d = synth.synthetic_model(C=2037, M=50, A=3, S=9, n_rounds=4, seed=5)
    X = synth.synthetic_X(24, d.C, seed=2)
    dev = ga.DeviceModel(d)
    p, lab = dev.infer(synth.synthetic_X(60, d.C, seed=3))
    assert p.dtype == np.float32
    rng = np.random.RandomState(0)
    y = lab.reshape(-1).copy()
    y[rng.rand(y.size) < 0.3] = 0
    y[:d.A] = np.arange(d.A)                      # every class occurs
    dev.close()
    if calibrated:
        for k, v in calibrate.fit_calibrator(p.reshape(-1, d.A), y, d.A).items():
            setattr(d, k, v)
    return d, X


def test_phase_gt2_equals_the_int8_route_on_a_calibrated_model(ga):
    """the file path (gnx_phase_gt2): base, calibrated Gnofix, then calibrated probabilities of the re-phased haplotypes"""
    from gnomix_amd import vcfio
    d, X = _trained_like_model(ga, True)
    dev = ga.DeviceModel(d)
    dev.set_calibrate(True)
    _, B = dev.base_predict(X)
    Xp, Y, nsw = dev.gnofix(X, B)
    p_ref, _ = dev.infer(Xp)
    assert p_ref.dtype == np.float64
    raw = ga.DeviceModel(d)                       # the same maps, switch off: another route and, here, another result
    Xr, Yr, nr = raw.gnofix(X, B)
    assert not (np.array_equal(Yr, Y) and np.array_equal(Xr, Xp))
    cols = np.arange(0, d.C, 7, dtype=np.int32)
    Go, pr, lab, ns2 = dev.phase_gt2(vcfio.pack_gt2(X), X.shape[0], np.arange(d.C, dtype=np.int32), out_cols=cols)
    assert np.array_equal(lab, Y) and np.array_equal(ns2, nsw) and np.array_equal(pr, p_ref)
    back = np.stack([(Go[:, h // 4] >> (2 * (h % 4))) & 3 for h in range(X.shape[0])], axis=0).astype(np.int8)
    assert np.array_equal(back, Xp[:, cols])


def test_calibration_off_is_the_old_dispatch(ga, models):
    """a model that CARRIES maps but has the switch off, and one without maps: gnx_gnofix_ex's defaults equal gnx_gnofix bit for bit
    (same library: this guards the dispatch), and differ from the calibrated run"""
    g, devs = models
    name = "a3"
    X, B = g[name + "_X"], np.ascontiguousarray(g[name + "_B"])
    off = ga.DeviceModel(_data(ga, g, name))
    plain = ga.DeviceModel(_data(ga, g, name, calibrator=False))
    X0, Y0, n0 = plain.gnofix(X, B, max_it=6)
    for dev in (off, plain):
        X1, Y1, n1 = dev.gnofix(X, B, max_it=6)
        X2, Y2, n2 = _ex(dev, X, B, dict(max_it=6))
        for a, b in ((X1, X0), (Y1, Y0), (n1, n0), (X2, X0), (Y2, Y0), (n2, n0)):
            assert np.array_equal(a, b)
    assert not np.array_equal(Y0, g[name + "_0_oY"])
    off.set_calibrate(True)                       # the switch alone changes the route
    X3, Y3, n3 = off.gnofix(X, B, max_it=6)
    assert np.array_equal(Y3, g[name + "_0_oY"]) and np.array_equal(X3, g[name + "_0_oX"])


def test_what_is_still_refused(ga, models, monkeypatch):
    from gnomix_amd import _lib
    g, devs = models
    X, B = g["a3_X"], np.ascontiguousarray(g["a3_B"])
    W, A = int(g["a3_W"]), int(g["a3_A"])
    # a CRF smoother cannot re-phase (src/model.py:194), calibrated or not
    rng = np.random.RandomState(1)
    crf = ga.GnxModelData(C=int(g["a3_C"]), M=int(g["a3_C"]) // W, A=A, S=5, context=0, smooth_kind="crf",
                          crf_state=rng.standard_normal((A, A)), crf_trans=rng.standard_normal((A, A)))
    crf.calib_off, crf.calib_x, crf.calib_y, crf.calib_is_f32 = g["a3_calib_off"], g["a3_calib_x"], g["a3_calib_y"], True
    hip = ga.HipGnomix(crf, calibrate=True)
    with pytest.raises(AssertionError, match="does not currently support re-phasing"):
        hip.phase(X, B=B)
    with pytest.raises(_lib.GnxError, match="Type of Smoother does not currently support re-phasing"):
        hip.dev.gnofix(X, B)
    # a calibrated model on the float32 Gnofix kernel: refused, and the message names the reason
    monkeypatch.setenv("GNX_GNOFIX_IMPL", "f32")
    ctx = _lib.Context(0)
    try:
        dev = ga.DeviceModel(_data(ga, g, "a3"), ctx=ctx)
        dev.set_calibrate(True)
        with pytest.raises(_lib.GnxError, match="rank-quantised copy") as e:
            dev.gnofix(X, B)
        assert e.value.code == _lib.GNX_EUNSUPPORTED
        dev.set_calibrate(False)
        assert dev.gnofix(X, B, max_it=2)[1].shape == (X.shape[0], W)      # the model still runs uncalibrated
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["crf", "cnn"])
def test_train_with_calibration_fast_and_large_modes(ga, kind):
    """HipGnomix.train(calibrate=True) for the CRF (float64 fit) and CNN (float32 fit) smoothers, at the geometry of
    tests/test_train_crf.py's end-to-end test: maps are fitted and loaded, calibrated output = the maps on the raw output, rows sum
    to one, and the model survives save / load"""
    import os
    import tempfile
    from gnomix_amd.train import cnn_init
    A, M, W, S = 3, 40, 30, 7
    Cn = M * W + 13
    rng = np.random.RandomState(4)
    freq = np.clip(rng.uniform(0.2, 0.8, size=(1, Cn)) + rng.normal(0, 0.13, size=(A, Cn)), 0.02, 0.98)

    def haplotypes(n, seed):
        r = np.random.RandomState(seed)
        y = np.zeros((n, W), np.int32)
        for i in range(n):
            cuts = np.sort(r.choice(np.arange(3, W - 3), size=2, replace=False))
            a = r.randint(A)
            for lo, hi in zip([0, *cuts], [*cuts, W]):
                y[i, lo:hi] = a
                a = (a + 1 + r.randint(A - 1)) % A
        ysnp = np.concatenate([np.repeat(y, M, axis=1), np.repeat(y[:, -1:], Cn - M * W, axis=1)], axis=1)
        X = (r.uniform(size=(n, Cn)) < freq[ysnp, np.arange(Cn)[None, :]]).astype(np.int8)
        return X, y

    t1, t2, v = haplotypes(120, 1), haplotypes(80, 2), haplotypes(40, 3)
    d = ga.GnxModelData(C=Cn, M=M, A=A, S=S, context=M // 2, smooth_kind=kind)
    d.base_kind, d.lr_coef, d.lr_intercept = "logistic", np.zeros((W, A, M + 2 * (M // 2) + Cn - M * W)), np.zeros((W, A))
    if kind == "crf":
        d.crf_state, d.crf_trans = np.zeros((A, A)), np.zeros((A, A))
        kw = {}
    else:
        d.cnn_weight, d.cnn_bias = cnn_init(A, S, seed=0)
        kw = dict(max_ep=30, seed=1)
    np.random.seed(0)                              # train_calibrator samples with numpy's global generator, as the reference
    g = ga.HipGnomix(d, calibrate=True)
    g.train((t1, t2, v), evaluate=False, **kw)
    data = g.dev.data
    assert data.calib_off is not None and len(data.calib_off) == A + 1 and g.smooth.calibrator
    assert data.calib_is_f32 is (kind == "cnn")
    assert g.smooth.calibrate and g.dev.calibrated
    pc = g.predict_proba(v[0])
    assert pc.dtype == np.float64
    g.smooth.calibrate = False
    raw = g.predict_proba(v[0])
    g.smooth.calibrate = True
    assert raw.dtype == (np.float64 if kind == "crf" else np.float32)
    want = g.dev.calibrate_rows(raw.reshape(-1, A)).reshape(raw.shape)
    assert np.array_equal(pc, want) and not np.array_equal(pc, raw.astype(np.float64))
    assert np.abs(pc.sum(-1) - 1.0).max() < 1e-12
    with tempfile.TemporaryDirectory() as td:
        g2 = ga.HipGnomix.load(g.save(os.path.join(td, "calibrated.gnx")), calibrate=True)
        assert np.array_equal(g2.predict_proba(v[0][:10]), pc[:10])
