"""The LDA base on the GPU: the Gram kernel of the fit (k_lda_gram) against int64 numpy, exactly; the fit (train_lda_base) against
tests/lda_exact.py, bit for bit (the integers and the host function are the same); the inference kernel (k_lda_softmax) against numpy
float64 within a bound derived from the summation; training end to end, the 2-bit entry, Gnofix, the reference's own LDABase
(tests/golden/G25_lda_base.npz), and the C ABI's refusals.

The bound on B, per row:  |dd| <= (width + 2) 2^-53 (sum_p |c_p x_p| + |b|)  for a float64 sum in any order (lda_exact.decision_bound),
|dp| <= 2 max_a |dd_a| + 4 * 2^-53.  The Gram kernel takes 64 haplotypes per MFMA step and 64 x 64 macro-tiles of [X | one-hot];
the inference kernel 256 query rows per block and 16 positions per X chunk."""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_golden
import lda_exact as LE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
C6, M6, CX6 = LE.SIXTH["C"], LE.SIXTH["M"], LE.SIXTH["cx"]
FIXTURE_TOL = 1.6e-10      # tests/test_lda_host.py, DECISION_TOL


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _xy(rng, N, A, C=C6, M=M6):
    return rng.randint(0, 3, (N, C)).astype(np.int8), rng.randint(0, A, (N, C // M)).astype(np.int32)


def _equal(got, ref):
    for a, b, name in zip(got, ref, "GSn"):
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), name


@pytest.mark.parametrize("N", (1, 63, 64, 65, 130))
def test_gram_equals_int64_numpy_exactly(ctx, N):
    from gnomix_amd.train import lda_gram
    rng = np.random.RandomState(N)
    X, y = _xy(rng, N, 3)
    X[0], X[-1] = np.arange(C6) % 3, (np.arange(C6) // 2) % 3      # asymmetric rows: a reflected or shifted column shows
    got = lda_gram(X, y, M6, CX6, 3, 0, 8, ctx=ctx)                 # widths 48 and 59: 59 + 3 one-hot columns end inside the tile
    ref = LE.numpy_gram(X, y, C6, M6, CX6, 3)
    _equal(got, ref)
    assert got[0].shape == (8, 59, 59) and not got[0][0, 48:].any() and not got[0][0, :, 48:].any() and got[0][7, 58, 58] > 0
    assert np.array_equal(got[0], got[0].transpose(0, 2, 1)) and got[2].sum() == 8 * N


def test_gram_seven_classes_a_window_range_device_pointers_and_a_row_pitch(ctx):
    import torch
    from gnomix_amd.train import lda_gram
    A, N, ldx = 7, 130, C6 + 13
    rng = np.random.RandomState(7)
    X, y = _xy(rng, N, A)
    # 59 + 7 = 66 columns: the one-hot columns spill into the second macro-tile together with the data; w0 = 5 .. the last window
    ref = LE.numpy_gram(X, y, C6, M6, CX6, A, 5, 8)
    _equal(lda_gram(X, y, M6, CX6, A, 5, 8, ctx=ctx), ref)
    _equal(lda_gram(X, y, M6, CX6, A, 2, 3, ctx=ctx), LE.numpy_gram(X, y, C6, M6, CX6, A, 2, 3))
    Xp = np.full((N, ldx), 3, np.int8)
    Xp[:, :C6] = X
    dX, dy = torch.from_numpy(Xp).cuda(), torch.from_numpy(y).cuda()
    G = torch.full((3, 59, 59), -1, dtype=torch.int32, device="cuda")
    S = torch.full((3, A, 59), -1, dtype=torch.int32, device="cuda")
    n = torch.full((3, A), -1, dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    ctx.check(ctx.lib.gnx_train_lda_gram_dev(ctx.h, dX.data_ptr(), N, ldx, dy.data_ptr(), C6, M6, CX6, A, 5, 8, G.data_ptr(), S.data_ptr(),
                                             n.data_ptr()))
    torch.cuda.synchronize()
    _equal((G.cpu().numpy(), S.cpu().numpy(), n.cpu().numpy()), ref)
    # the host form with the same pitch
    Gh, Sh, nh = np.zeros((3, 59, 59), np.int32), np.zeros((3, A, 59), np.int32), np.zeros((3, A), np.int32)
    Xp[:, C6:] = 0
    ctx.check(ctx.lib.gnx_train_lda_gram(ctx.h, Xp.ctypes.data, N, ldx, y.ctypes.data, C6, M6, CX6, A, 5, 8, Gh.ctypes.data, Sh.ctypes.data,
                                         nh.ctypes.data))
    _equal((Gh, Sh, nh), ref)


def test_gram_refusals_are_decided_on_the_arguments(ctx):
    from gnomix_amd import _lib
    X, y = _xy(np.random.RandomState(0), 4, 3)
    G, S, n = np.zeros((8, 59, 59), np.int32), np.zeros((8, 3, 59), np.int32), np.zeros((8, 3), np.int32)

    def call(fn, N=4, A=3, w0=0, w1=8, yy=y):
        return fn(ctx.h, X.ctypes.data, N, C6, yy.ctypes.data, C6, M6, CX6, A, w0, w1, G.ctypes.data, S.ctypes.data, n.ctypes.data)

    for fn in (ctx.lib.gnx_train_lda_gram, ctx.lib.gnx_train_lda_gram_dev):     # (refused before any pointer is followed)
        assert call(fn, N=1 << 29) == _lib.GNX_EINVAL and "4 N" in ctx.lib.gnx_last_error(ctx.h).decode()
        assert call(fn, w0=5, w1=9) == _lib.GNX_EINVAL and call(fn, w0=3, w1=3) == _lib.GNX_EINVAL and call(fn, A=1) == _lib.GNX_EINVAL
    bad = y.copy()
    bad[2, 6] = 3
    assert call(ctx.lib.gnx_train_lda_gram, yy=bad) == _lib.GNX_EINVAL and "label" in ctx.lib.gnx_last_error(ctx.h).decode()
    bad[2, 6] = -1
    assert call(ctx.lib.gnx_train_lda_gram, yy=bad) == _lib.GNX_EINVAL
    assert call(ctx.lib.gnx_train_lda_gram, yy=bad, w0=0, w1=6) == _lib.GNX_OK       # the bad label lies outside the range
    assert call(ctx.lib.gnx_train_lda_gram) == _lib.GNX_OK


@pytest.mark.parametrize("A", (3, 2))
def test_fit_is_bit_identical_to_the_restatement(ctx, A):
    from gnomix_amd.train import train_lda_base, untrained_model
    (C, M, cx, _), X, y, Xq = LE.sixth_panel(A)
    coef, icpt, infos = LE.fit(X, y, C, M, cx, A)
    for per_call in (None, 3):
        d = untrained_model(C, M, A, 5, cx, "default", base="lda_svd")
        info = train_lda_base(d, X, y, ctx=ctx, windows_per_call=per_call)
        assert d.base_kind == "lda" and np.array_equal(d.lda_coef, coef) and np.array_equal(d.lda_intercept, icpt)
        assert np.array_equal(info["ranks"], [(i["rank"], i["rank2"]) for i in infos])
    yb = y.copy()
    yb[yb[:, 4] == A - 1, 4] = 0
    with pytest.raises(ValueError, match="window 4: class %d has no row" % (A - 1)):
        train_lda_base(untrained_model(C, M, A, 5, cx, "default", base="lda_svd"), X, yb, ctx=ctx)


def _lda_model(rng, A, C=C6, M=M6, cx=CX6):
    from gnomix_amd.train import untrained_model
    d = untrained_model(C, M, A, 3, cx, "default", base="lda_svd", seed=1)
    for w in range(d.W):
        width = d.window_width(w)
        d.lda_coef[w, :, :width] = rng.normal(size=(d.lda_coef.shape[1], width)) * 10.0 ** rng.uniform(-2, 3, size=(d.lda_coef.shape[1], 1))
        d.lda_intercept[w] = rng.normal(size=d.lda_coef.shape[1]) * 10.0 ** rng.uniform(-1, 3)
    return d


def _check(dev, d, Xq, what, extra=0.0):
    """the device's B against numpy float64 within the derived bound -> b64"""
    C, M, cx, A = d.C, d.M, d.context, d.A
    ref = LE.predict(Xq, d.lda_coef, d.lda_intercept, C, M, cx, A)
    bound = 2 * LE.decision_bound(Xq, d.lda_coef, d.lda_intercept, C, M, cx) + 4 * 2.0 ** -53 + extra
    b32, b64 = dev.base_predict(Xq, want_f32=True, want_f64=True)
    err = np.abs(b64 - ref).max(-1)
    print(what, "cells %d, max |B - numpy| %.3e, worst err / bound %.3f" % (err.size, err.max(), (err / bound).max()))
    assert b64.shape == ref.shape and np.all(err <= bound)
    assert np.array_equal(b32, b64.astype(np.float32))
    assert np.all(np.abs(b64.sum(-1) - 1.0) <= 4 * 2.0 ** -52)
    top = np.sort(ref, axis=-1)
    clear = top[..., -1] - top[..., -2] > 2 * bound
    print(what, "rows whose top-two gap is inside twice the bound: %d of %d" % ((~clear).sum(), clear.size))
    assert (~clear).sum() <= 0.01 * clear.size
    assert np.array_equal(b64.argmax(-1)[clear], ref.argmax(-1)[clear])
    return b64


@pytest.mark.parametrize("A", (2, 3, 7, 12))
@pytest.mark.parametrize("N", (1, 17, 257))
def test_inference_from_given_coefficients_equals_numpy_within_the_derived_bound(ctx, N, A):
    from gnomix_amd import DeviceModel
    rng = np.random.RandomState(100 * A + N)
    d = _lda_model(rng, A)
    Xq = rng.randint(0, 3, (N, C6)).astype(np.int8)
    Xq[0] = np.arange(C6) % 3
    B = _check(DeviceModel(d, ctx=ctx), d, Xq, "N %d A %d" % (N, A))
    if N == 257:
        assert (B.max(-1) == 1.0).any() and (B.max(-1) < 1.0).any()    # saturated rows and rows that are not


def test_packed_entry_device_pointers_and_the_references_base_G25(ctx):
    import torch
    from gnomix_amd import DeviceModel
    from gnomix_amd.convert import lda_from_sklearn
    from gnomix_amd.train import untrained_model
    for A in (3, 2):
        g = load_golden("G25_lda_base.npz")
        pre = "A%d_" % A
        d = untrained_model(C6, M6, A, 3, CX6, "default", base="lda_svd", seed=1)
        for w in range(d.W):
            c, b = lda_from_sklearn(type("Bag", (), dict(coef_=g["%sw%d_coef_" % (pre, w)], intercept_=g["%sw%d_intercept_" % (pre, w)],
                                                         classes_=np.arange(A)))(), d.window_width(w), A)
            d.lda_coef[w, :, :c.shape[1]], d.lda_intercept[w] = c, b
        dev = DeviceModel(d, ctx=ctx)
        Xq = g[pre + "Xq"]
        B = _check(dev, d, Xq, "G25 A %d" % A)
        bound = 2 * LE.decision_bound(Xq, d.lda_coef, d.lda_intercept, C6, M6, CX6) + 4 * 2.0 ** -53 + FIXTURE_TOL
        err = np.abs(B - g[pre + "B"]).max(-1)
        print("G25 A %d max |B - reference| %.3e" % (A, err.max()))
        assert np.all(err <= bound)
        P = torch.from_numpy(np.ascontiguousarray(dev.pack_x(Xq))).cuda()
        assert np.array_equal(dev.base_predict_packed_device(P, f64=True).cpu().numpy(), B)
        assert np.array_equal(dev.base_predict_device(torch.from_numpy(Xq).cuda(), f64=True).cpu().numpy(), B)
        p, l = dev.infer(Xq)
        p2, l2 = dev.infer_packed(dev.pack_x(Xq))
        assert np.array_equal(p, p2) and np.array_equal(l, l2)


def test_load_refusals_return_the_stated_codes(ctx):
    from gnomix_amd import DeviceModel, _lib
    rng = np.random.RandomState(3)
    d = _lda_model(rng, 3)
    desc, keep = d.to_desc()
    h = ctypes.c_void_p()
    assert ctx.lib.gnx_model_load(ctx.h, ctypes.byref(desc), ctypes.byref(h)) == _lib.GNX_EINVAL and not h.value
    assert "gnx_model_load_lda" in ctx.lib.gnx_last_error(ctx.h).decode()
    for where, value in (("coef", np.nan), ("coef", np.inf), ("icpt", -np.inf)):
        bad = _lda_model(rng, 3)
        if where == "coef":
            bad.lda_coef[5, 2, 40] = value
        else:
            bad.lda_intercept[5, 1] = value
        with pytest.raises(_lib.GnxError, match="window 5") as e:
            DeviceModel(bad, ctx=ctx)
        assert e.value.code == _lib.GNX_EINVAL
    lda, keep2 = d.lda_windows()
    lda[7].width = 48
    assert ctx.lib.gnx_model_load_lda(ctx.h, ctypes.byref(desc), lda, ctypes.byref(h)) == _lib.GNX_EINVAL
    desc.base_kind = _lib.BASE_NB
    assert ctx.lib.gnx_model_load_lda(ctx.h, ctypes.byref(desc), lda, ctypes.byref(h)) == _lib.GNX_EINVAL
    with pytest.raises(_lib.GnxError) as e:
        DeviceModel(_lda_model(rng, 17), ctx=ctx)
    assert e.value.code == _lib.GNX_EUNSUPPORTED


def test_trains_end_to_end_and_answers_like_the_parts_composed_by_hand(ctx, tmp_path):
    from gnomix_amd import HipGnomix, GnxModelData
    from gnomix_amd.train import untrained_model
    (C, M, cx, A), data = LE.e2e_data(seed=7)
    model = HipGnomix(untrained_model(C, M, A, 3, cx, "default", base="lda_svd", seed=1), ctx=ctx)
    model.train(data=data, retrain_base=True, evaluate=True)
    print("accuracies", model.accuracies)
    d = model.dev.data
    assert d.base_kind == "lda" and d.smooth_kind == "xgb" and model.accuracies["base_val_acc"] > 100.0 / A
    X_q = data[2][0]
    _check(model.dev, d, X_q, "trained")
    p, lab = model.predict_proba(X_q), model.predict(X_q)
    b32, _ = model.dev.base_predict(X_q, want_f32=True, want_f64=False)
    p_hand, lab_hand = model.dev.smooth_predict(b32)
    assert np.array_equal(lab, lab_hand) and np.array_equal(p, p_hand)
    _, lab_packed = model.dev.infer_packed(model.dev.pack_x(X_q))
    assert np.array_equal(lab_packed, lab)
    Xp, Yp = model.phase(X_q)
    assert Xp.shape == X_q.shape and np.array_equal(np.sort(Xp.reshape(-1, 2, C), axis=1), np.sort(X_q.reshape(-1, 2, C), axis=1))
    path = str(tmp_path / "lda.gnx")
    model.save(path)
    again = HipGnomix(GnxModelData.load(path), ctx=ctx)
    assert np.array_equal(again.predict_proba(X_q), p) and np.array_equal(again.predict(X_q), lab)
