"""The three Naive-Bayes bases on the GPU: the table kernel (k_nb_table) against tests/nb_exact.py — a sequential float64 sum in
position order — at every tile edge, class count and window geometry, against the reference's own bases (tests/golden/G23_nb.npz)
and live scikit-learn; the counting kernel of the fit (k_nb_count) against numpy, exactly; training end to end, the command line, and
the C ABI's refusals.

The bar on B is nb_exact.tolerance: 1e-12 (the project's bar for base probabilities) wherever the restated max |jll| <= 512, else
8 ulp(max |jll|), the spacing scikit-learn's own jll - logsumexp carries.  Labels must be equal wherever the restatement's top-two
gap exceeds that bar.  The kernel takes 256 query rows per block and 16 positions per X chunk."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from conftest import load_golden
import nb_exact as NE
from nb_exact import KINDS, golden_windows, numpy_counts, degenerate_panel, sk_estimator, e2e_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BLOCK_ROWS, CHUNK = 256, 16


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _model(C, M, A, cx, wins, kind="gaussian"):
    from gnomix_amd.train import untrained_model
    d = untrained_model(C, M, A, 1, cx, "default", base="nb_" + kind)
    for w, (t, b) in enumerate(wins):
        d.nb_table[w, :len(t)], d.nb_bias[w] = t, b
    if d.W < 2:
        d.smooth_kind = None        # (the tree smoother needs more windows than its size; these tests run the base pass)
    return d


def _random_windows(rng, C, M, A, cx, scale=1.0, absent=()):
    W = C // M
    wins = []
    for w in range(W):
        width = M + 2 * cx + (C - M * W if w == W - 1 else 0)
        t, b = scale * rng.normal(size=(width, 4, A)), rng.normal(size=A)
        for (aw, ac) in absent:
            if aw == w:
                t[:, :, ac], b[ac] = 0.0, -np.inf
        wins.append((t, b))
    return wins


def _check(dev, Xq, wins, C, M, cx, A, what):
    ref, J = NE.predict(Xq, wins, C, M, cx, A)
    tol = NE.tolerance(J)
    b32, b64 = dev.base_predict(Xq, want_f32=True, want_f64=True)
    err = np.abs(b64 - ref).max(-1)
    print(what, "cells %d, max |B - restatement| %.3e (bar min %.1e max %.1e), worst err / bar %.3f" %
          (err.size, err.max(), tol.min(), tol.max(), (err / tol).max()))
    assert b64.dtype == np.float64 and b32.dtype == np.float32 and np.isfinite(b64).all()
    assert np.all(err <= tol)
    assert np.array_equal(b32, b64.astype(np.float32))
    top = np.sort(ref, -1)
    clear = top[..., -1] - top[..., -2] > tol
    assert np.array_equal(b64.argmax(-1)[clear], ref.argmax(-1)[clear])
    s = b64.sum(-1)
    assert np.all(np.abs(s - 1.0) <= 4 * np.spacing(1.0))
    return b64


@pytest.mark.parametrize("N", (1, 15, 16, 17, BLOCK_ROWS + 1))
def test_row_counts_around_the_tile_and_block_sizes(ctx, N):
    from gnomix_amd import DeviceModel
    C, M, cx, A = 83, 20, 3, 4
    rng = np.random.RandomState(N)
    wins = _random_windows(rng, C, M, A, cx)
    _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), rng.randint(0, 3, (N, C)).astype(np.int8), wins, C, M, cx, A, "N = %d" % N)


@pytest.mark.parametrize("A", (2, 3, 7, 12, 16))
def test_class_counts_up_to_one_column_tile(ctx, A):
    from gnomix_amd import DeviceModel
    C, M, cx = 83, 20, 3
    rng = np.random.RandomState(100 + A)
    wins = _random_windows(rng, C, M, A, cx)
    _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), rng.randint(0, 3, (33, C)).astype(np.int8), wins, C, M, cx, A, "A = %d" % A)


# the narrowest model the loader takes is M = 2, ctx = 0, C = 5 (widths 2 and 3): C % M == 0 is refused, so M = 1 cannot be loaded
GEOMETRIES = [("narrowest", 5, 2, 0), ("one window", 23, 20, 0), ("one window with context", 23, 20, 4),
              ("chunk - 1", 2 * (CHUNK - 1) + 1, CHUNK - 1, 0), ("chunk", 2 * CHUNK + 1, CHUNK, 0), ("chunk + 1", 2 * (CHUNK + 1) + 1, CHUNK + 1, 0),
              ("chunk with context", 3 * 12 + 5, 12, 2), ("two chunks + 1, context", 4 * 25 + 7, 25, 4), ("context wider than a window", 5 * 6 + 2, 6, 9),
              # a one-position tail (nv = 1): after a full chunk on the contiguous path (interior windows) and on the gathered path (edges)
              ("chunk + 1 with context", 4 * 13 + 3, 13, 2)]


@pytest.mark.parametrize("name,C,M,cx", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_window_geometries_first_and_last_windows_and_remainders(ctx, name, C, M, cx):
    from gnomix_amd import DeviceModel
    A = 3
    rng = np.random.RandomState(len(name) + C)
    wins = _random_windows(rng, C, M, A, cx)
    Xq = rng.randint(0, 3, (37, C)).astype(np.int8)
    Xq[0], Xq[1] = np.arange(C) % 3, (np.arange(C) // 2) % 3     # asymmetric rows: a reflected or shifted column shows
    B = _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), Xq, wins, C, M, cx, A, name)
    assert B.shape == (37, C // M, A)


def test_codes_2_and_3_the_2bit_entry_absent_classes_and_large_sums(ctx):
    import torch
    from gnomix_amd import DeviceModel
    C, M, cx, A = 331, 60, 11, 5
    rng = np.random.RandomState(4)
    wins = _random_windows(rng, C, M, A, cx, absent=((0, 1), (2, 0), (2, 4), (4, 3)))
    Xq = rng.randint(0, 4, (70, C)).astype(np.int8)
    Xq[0], Xq[1] = 3, 2
    dev = DeviceModel(_model(C, M, A, cx, wins), ctx=ctx)
    B = _check(dev, Xq, wins, C, M, cx, A, "codes 0..3, absent classes")
    for (w, c) in ((0, 1), (2, 0), (2, 4), (4, 3)):
        assert not B[:, w, c].any()
    assert (B[:, 1] > 0).all()
    P = torch.from_numpy(np.ascontiguousarray(dev.pack_x(Xq))).cuda()
    assert np.array_equal(dev.base_predict_packed_device(P, f64=True).cpu().numpy(), B)
    assert np.array_equal(dev.base_predict_packed_device(P, f64=False).cpu().numpy(), B.astype(np.float32))
    assert np.array_equal(dev.base_predict_device(torch.from_numpy(Xq).cuda(), f64=True).cpu().numpy(), B)
    p, l = dev.infer(Xq)
    p2, l2 = dev.infer_packed(dev.pack_x(Xq))
    assert np.array_equal(p, p2) and np.array_equal(l, l2)
    # sums far above 512: the bar becomes 8 ulp(max |jll|)
    wins = _random_windows(rng, C, M, A, cx, scale=300.0)
    ref, J = NE.predict(Xq, wins, C, M, cx, A)
    assert np.abs(J).max() > 2048
    _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), Xq, wins, C, M, cx, A, "large sums")


@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_references_bases_G23(ctx, kind):
    from gnomix_amd import DeviceModel
    g = load_golden("G23_nb.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    wins = golden_windows(g, kind)
    B = _check(DeviceModel(_model(C, M, A, cx, wins, kind), ctx=ctx), g["Xq"], wins, C, M, cx, A, "G23 " + kind)
    err = np.abs(B - g[kind + "_B"]).max()
    print("G23", kind, "max |B - reference| %.3e" % err)
    assert err <= 1e-12 and np.array_equal(B.argmax(-1), g[kind + "_B"].argmax(-1))


@pytest.mark.parametrize("n_fit", (131, 240))
def test_counts_equal_numpy_exactly(ctx, n_fit):
    from gnomix_amd.train import nb_counts
    C, M, A, cx = 300 + 7, 100, 5, 30            # ldw = 167: more than one count block per window is not needed below 256
    rng = np.random.RandomState(n_fit)
    X, y = rng.randint(0, 3, (n_fit, C)).astype(np.int8), rng.randint(0, A, (n_fit, C // M)).astype(np.int32)
    y[:, 1][y[:, 1] == 2] = 0                    # a class without rows in a window
    got = nb_counts(X, y, M, cx, A, ctx=ctx)
    for a, b in zip(got, numpy_counts(X, y, C, M, cx, A)):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    C, M, cx = 2 * 300 + 5, 300, 0               # widths 300 and 305: two count blocks per window
    X, y = rng.randint(0, 3, (n_fit, C)).astype(np.int8), rng.randint(0, A, (n_fit, 2)).astype(np.int32)
    for a, b in zip(nb_counts(X, y, M, cx, A, ctx=ctx), numpy_counts(X, y, C, M, cx, A)):
        assert np.array_equal(a, b)


def _sklearn_B(kind, X, y, Xq, C, M, cx, A):
    W = C // M
    B = np.zeros((len(Xq), W, A))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for w in range(W):
            cols = NE.window_columns(C, M, cx, w)
            sk = sk_estimator(kind).fit(X[:, cols].astype(np.float64), y[:, w])
            B[:, w][:, sk.classes_] = sk.predict_proba(Xq[:, cols].astype(np.float64))
    return B


@pytest.mark.parametrize("kind", KINDS)
def test_device_trained_tables_on_the_degenerate_panel_equal_live_scikit_learn(ctx, kind):
    from gnomix_amd import DeviceModel
    from gnomix_amd.train import train_nb_base, untrained_model
    C, M, A, cx, X, y, Xq = degenerate_panel()
    d = untrained_model(C, M, A, 1, cx, "default", base="nb_" + kind)
    info = train_nb_base(d, X, y, kind, ctx=ctx)
    for a, b in zip((info["n1"], info["n2"], info["class_count"]), numpy_counts(X, y, C, M, cx, A)):
        assert np.array_equal(a, b)
    wins = [(d.nb_table[w, :d.window_width(w)], d.nb_bias[w]) for w in range(d.W)]
    B = _check(DeviceModel(d, ctx=ctx), Xq, wins, C, M, cx, A, "degenerate " + kind)
    ref = _sklearn_B(kind, X, y, Xq, C, M, cx, A)
    _, J = NE.predict(Xq, wins, C, M, cx, A)
    err = np.abs(B - ref).max(-1)
    print("degenerate", kind, "max |B - scikit-learn| %.3e" % err.max())
    assert np.all(err <= NE.tolerance(J))


@pytest.mark.parametrize("kind", KINDS)
def test_hipgnomix_trains_the_base_and_answers_like_live_scikit_learn(ctx, kind):
    from gnomix_amd import HipGnomix
    from gnomix_amd.train import untrained_model
    g = load_golden("G23_nb.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    X, y = g["Xt"][:211], g["yt"][:211]            # a fit-row count that is not a multiple of anything
    model = HipGnomix(untrained_model(C, M, A, 5, cx, "default", base="nb_" + kind, seed=1), ctx=ctx)
    model.base.train(X, y)
    d = model.dev.data
    assert d.base_kind == "nb" and d.nb_kind == kind
    B = np.asarray(model.base.predict_proba(g["Xq"]), dtype=np.float64)
    wins = [(d.nb_table[w, :d.window_width(w)], d.nb_bias[w]) for w in range(d.W)]
    _, J = NE.predict(g["Xq"], wins, C, M, cx, A)
    ref = _sklearn_B(kind, X, y, g["Xq"], C, M, cx, A)
    err = np.abs(B - ref).max(-1)
    print("trained", kind, "max |B - scikit-learn| %.3e" % err.max())
    assert B.dtype == np.float64 and np.all(err <= NE.tolerance(J))


def test_trains_end_to_end_saves_loads_and_serves_the_command_line(ctx, tmp_path):
    import subprocess
    import sys
    from gnomix_amd import HipGnomix, GnxModelData, synth, vcfio
    from gnomix_amd.train import untrained_model
    (C, M, cx, A), data = e2e_data(seed=7)
    d = untrained_model(C, M, A, 5, cx, "default", base="nb_bernoulli", seed=1,
                        meta=dict(snp_pos=1000 + 37 * np.arange(C), snp_ref=np.array(["A"] * C), snp_alt=np.array(["C"] * C),
                                  pop_order=["p%d" % a for a in range(A)]))
    d.gen_map_pos, d.gen_map_cm = np.array([1, 400_000]), np.array([0.0, 1.3])
    model = HipGnomix(d, ctx=ctx)
    model.train(data=data, retrain_base=True, evaluate=True)
    print("accuracies", model.accuracies)
    assert model.accuracies["base_val_acc"] > 100.0 / A and "smooth_train_acc" in model.accuracies
    assert model.dev.data.base_kind == "nb" and model.dev.data.nb_kind == "bernoulli"
    X_q = data[2][0][:40]
    p, lab = model.predict_proba(X_q), model.predict(X_q)
    Xp, Yp = model.phase(X_q)
    assert np.isfinite(p).all()
    path = str(tmp_path / "nb.gnx")
    model.save(path)
    again = HipGnomix(GnxModelData.load(path), ctx=ctx)
    assert np.array_equal(again.predict_proba(X_q), p) and np.array_equal(again.predict(X_q), lab)
    Xp2, Yp2 = again.phase(X_q)
    assert np.array_equal(Xp, Xp2) and np.array_equal(Yp, Yp2)
    dd = model.dev.data
    vcf = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X_q), len(X_q) // 2, dd.snp_pos, dd.snp_ref, dd.snp_alt, chrom="22")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gnomix.py"), vcf, str(tmp_path / "out"), "22", "False", path],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    msp = [ln.split("\t") for ln in open(tmp_path / "out" / "query_results.msp").read().splitlines()[2:]]
    assert len(msp) == C // M and (tmp_path / "out" / "query_results.fb").exists()
    assert np.array_equal(np.array([[int(v) for v in row[6:]] for row in msp]).T, lab)


def test_the_c_abi_refuses_what_the_header_says(ctx):
    from gnomix_amd import DeviceModel, _lib
    C, M, cx, A = 131, 30, 4, 3
    rng = np.random.RandomState(2)

    def refused(d, code, says):
        with pytest.raises(_lib.GnxError) as e:
            DeviceModel(d, ctx=ctx)
        assert e.value.code == code and says in str(e.value), str(e.value)

    good = lambda: _model(C, M, A, cx, _random_windows(rng, C, M, A, cx))   # noqa: E731
    DeviceModel(good(), ctx=ctx)
    for bad in (np.nan, np.inf, -np.inf):
        d = good()
        d.nb_table[2, 5, 1, 2] = bad
        refused(d, _lib.GNX_EINVAL, "window 2")
    for bad in (np.nan, np.inf):
        d = good()
        d.nb_bias[1, 0] = bad
        refused(d, _lib.GNX_EINVAL, "bias")
    d = good()
    d.nb_bias[3] = -np.inf
    refused(d, _lib.GNX_EINVAL, "no class")
    d = good()
    desc, keep = d.to_desc()
    nb, keep2 = d.nb_windows()
    h = ctypes.c_void_p()
    nb[1].width += 1
    assert ctx.lib.gnx_model_load_nb(ctx.h, ctypes.byref(desc), nb, ctypes.byref(h)) == _lib.GNX_EINVAL and not h.value
    assert b"width" in ctx.lib.gnx_last_error(ctx.h)
    nb[1].width -= 1
    # gnx_model_load does not take the kind and names the entry that does
    assert ctx.lib.gnx_model_load(ctx.h, ctypes.byref(desc), ctypes.byref(h)) == _lib.GNX_EINVAL and not h.value
    assert b"gnx_model_load_nb" in ctx.lib.gnx_last_error(ctx.h)
    desc.base_kind = _lib.BASE_LOGISTIC
    assert ctx.lib.gnx_model_load_nb(ctx.h, ctypes.byref(desc), nb, ctypes.byref(h)) == _lib.GNX_EINVAL and not h.value
    desc.base_kind = _lib.BASE_NB
    assert ctx.lib.gnx_model_load_nb(ctx.h, ctypes.byref(desc), None, ctypes.byref(h)) == _lib.GNX_EINVAL and not h.value
    # more than one column tile
    A17 = 17
    refused(_model(C, M, A17, cx, _random_windows(rng, C, M, A17, cx)), _lib.GNX_EUNSUPPORTED, "16")
    # the counting entry: labels and codes outside their ranges
    X, y = rng.randint(0, 3, (9, C)).astype(np.int8), rng.randint(0, A, (9, C // M)).astype(np.int32)
    from gnomix_amd.train import nb_counts
    for bx, by in ((np.where(X == 2, 3, X), y), (X, y + 1), (X, y - 1)):
        with pytest.raises(_lib.GnxError) as e:
            nb_counts(bx, by, M, cx, A, ctx=ctx)
        assert e.value.code == _lib.GNX_EINVAL
    # nothing was half-loaded: the context still serves a good model
    wins = _random_windows(rng, C, M, A, cx)
    _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), rng.randint(0, 3, (5, C)).astype(np.int8), wins, C, M, cx, A, "after refusals")
