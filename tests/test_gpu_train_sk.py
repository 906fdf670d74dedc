"""The plain and the polynomial string-kernel SVC bases (StringKernelBase, PolynomialStringKernelBase) trained on the MI355X:
the Gram pass checked entry for entry against the oracle's kernels (gnx_svc_gram), both fits pinned to the reference's own
(tests/golden/G27_sk_train.npz), the polynomial fit compared with sklearn on random geometries, HipGnomix.train end to end with
the seeds the reference's sequential fits draw, and the rejections of the C entries."""
import ctypes as C_
import zlib

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
P = 1.2


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300) + 1e-300)


def _run_values(C, M, cx):
    from gnomix_amd.convert import poly_run_values
    return poly_run_values(M + 2 * cx + C % M, P)["run_value"]


# name, C, M, ctx: window widths M + 2 ctx, the last one C % M more
GRAM_GEOMETRIES = [
    ("width31_partial_word", 62, 31, 0),
    ("width64_exact_words", 128, 64, 0),
    ("width200_one_leaf", 200, 100, 50),          # ~100 contigs between random rows: the <= 128 leaf and its m % 8 tail
    ("width333_recursion_wider_last", 495, 233, 50),  # ~167 / ~181 contigs: one split; the all-mismatch pair (334 / 363): two
]


def _gram_rows(name, C, N=48):
    rng = np.random.RandomState(zlib.crc32(name.encode()) % 1000)
    X = rng.randint(0, 2, size=(N, C)).astype(np.int8)
    X[rng.random_sample(X.shape) < 0.03] = 2      # rows with code 2 (a third symbol)
    X[1] = X[0]                                   # two equal rows: one contig
    X[3] = rng.randint(0, 2, size=C)
    X[2] = 1 - X[3]                               # every SNP differs: width + 1 zero-length contigs
    X[5] = 2                                      # a row of missing calls only
    return X


@pytest.mark.parametrize("name,C,M,cx", GRAM_GEOMETRIES, ids=[g[0] for g in GRAM_GEOMETRIES])
def test_gram_matrices_equal_the_oracles_kernels_entry_for_entry(ctx, oracle, name, C, M, cx):
    from gnomix_amd.train import svc_gram, window_columns
    X = _gram_rows(name, C)
    W, rv = C // M, _run_values(C, M, cx)
    Gp = svc_gram(X, M, cx, kernel="poly_kernel", p=P, ctx=ctx)
    Gs = svc_gram(X, M, cx, kernel="string_kernel", ctx=ctx)
    Gc = svc_gram(X, M, cx, kernel="CovRSK", ctx=ctx)
    assert Gp.shape == Gs.shape == Gc.shape == (W, len(X), len(X)) and Gp.dtype == np.float32
    for w in range(W):
        Xw = X[:, window_columns(C, M, cx, w)]
        width = Xw.shape[1]
        assert width == M + 2 * cx + (C % M if w == W - 1 else 0)
        Kp = oracle.poly_kernel(Xw, Xw, rv, P)
        bad = np.argwhere(Gp[w] != Kp)
        assert len(bad) == 0, (name, w, bad[:5], Gp[w][tuple(bad[0])], Kp[tuple(bad[0])])
        assert np.array_equal(Gp[w], Gp[w].T)
        assert (np.diag(Gp[w]) == int(width ** P / P)).all()
        assert Gp[w][0, 1] == Gp[w][0, 0] and Gp[w][2, 3] == int((width + 1) * rv[0] / P) == 0
        assert np.array_equal(Gs[w], oracle.string_kernel(Xw, Xw)), (name, w)
        assert np.array_equal(Gs[w], Gs[w].T) and (np.diag(Gs[w]) == width * (width + 1) // 2).all()
        assert np.array_equal(Gc[w], oracle.covrsk(Xw, Xw)), (name, w)
    # a sub-range answers the same matrices
    assert np.array_equal(svc_gram(X, M, cx, kernel="poly_kernel", p=P, w0=W - 1, w1=W, ctx=ctx)[0], Gp[W - 1])


def test_gram_of_the_fixture_equals_the_references_own_matrix(ctx):
    from gnomix_amd.train import svc_gram
    g = load_golden("G27_sk_train.npz")
    G = svc_gram(g["Xt"], int(g["M"]), int(g["ctx"]), kernel="poly_kernel", p=float(g["poly_p"]), w0=0, w1=1, ctx=ctx)
    assert np.array_equal(G[0], g["pk_K0"])


@pytest.mark.parametrize("kernel,pre,base_name", [("string_kernel", "sk_", "string_kernel"), ("poly_kernel", "pk_", "poly_string_kernel")])
def test_G27_reference_fit_is_reproduced(ctx, kernel, pre, base_name):
    """fails before the polynomial trainer exists with GNX_EUNSUPPORTED (poly) / an unknown base name (both)"""
    from gnomix_amd import DeviceModel
    from gnomix_amd.base import HipBase
    from gnomix_amd.train import train_svc_arrays, train_svc_base, untrained_model
    g = load_golden("G27_sk_train.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    res, info = train_svc_arrays(g["Xt"], g["yt"], M, cx, A, g["seeds"], kernel=kernel, ctx=ctx)
    assert info["n_guarded"] == 0
    for w in range(C // M):
        n = int(res["n_sv"][w])
        assert np.array_equal(res["support"][w, :n], g["%sw%d_support" % (pre, w)]), w
        assert np.array_equal(res["n_support"][w], g["%sw%d_n_support" % (pre, w)]), w
        assert np.max(np.abs(res["dual_coef"][w, :, :n] - g["%sw%d_dual" % (pre, w)])) <= 1e-12, w
        assert np.max(np.abs(res["intercept"][w] - g["%sw%d_intercept" % (pre, w)])) <= 1e-12, w
        assert _close(res["prob_a"][w], g["%sw%d_probA" % (pre, w)], 1e-10) and _close(res["prob_b"][w], g["%sw%d_probB" % (pre, w)], 1e-10), w
    d = untrained_model(C, M, A, 1, cx, "default", base=base_name)
    train_svc_base(d, g["Xt"], g["yt"], ctx=ctx, seeds=g["seeds"], kernel=kernel)
    B = HipBase(DeviceModel(d, ctx=ctx)).predict_proba(g["Xq"])
    err = np.max(np.abs(B - g[pre + "B"]))
    print(kernel, "predict_proba vs the reference: max |diff| = %.3g" % err)
    assert err <= 1e-12 and np.array_equal(np.argmax(B, -1), np.argmax(g[pre + "B"], -1))


def _sk_fit(K, yw, k):
    """sklearn's fit on a precomputed Gram; RandomState(k) makes it draw the seed RandomState(k).randint(2**31 - 1)"""
    from sklearn.svm import SVC
    return SVC(kernel="precomputed", probability=True, random_state=np.random.RandomState(k)).fit(K.astype(np.float64), yw)


def _labels(rng, N, W, A, counts=None):
    y = np.empty((N, W), np.int32)
    for w in range(W):
        col = np.concatenate([np.arange(A), rng.randint(0, A, N - A)]) if counts is None else np.repeat(np.arange(A), counts)
        y[:, w] = rng.permutation(col)
    return y


GEOMETRIES = [
    # name, N, C, M, ctx, A, how the rows / labels are drawn
    ("A2_partial_words", 40, 203, 40, 7, 2, "plain"),
    ("A3_duplicated_rows", 45, 260, 50, 9, 3, "dup"),
    ("A7_imbalanced", 70, 150, 30, 5, 7, "imbalanced"),
]


@pytest.mark.parametrize("name,N,C,M,cx,A,how", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_poly_fit_against_sklearn_on_random_geometries(ctx, oracle, name, N, C, M, cx, A, how):
    from gnomix_amd.train import train_svc_arrays, window_columns, SVC_SEED_HIGH
    rng = np.random.RandomState(zlib.crc32(name.encode()) % 1000)
    W = C // M
    X = (rng.random_sample((N, C)) < rng.uniform(0.2, 0.8, C)).astype(np.int8)
    X[rng.random_sample(X.shape) < 0.02] = 2
    if how == "dup":
        X[N // 2:] = X[:N - N // 2]           # every row twice: tied kernel rows
    counts = {"imbalanced": [40, 3, 4, 6, 2, 10, 5]}.get(how)
    y = _labels(rng, N, W, A, counts)
    ks = [100 + w for w in range(W)]
    seeds = np.array([np.random.RandomState(k).randint(SVC_SEED_HIGH) for k in ks], np.uint32)
    res, info = train_svc_arrays(X, y, M, cx, A, seeds, kernel="poly_kernel", p=P, ctx=ctx)
    assert info["n_guarded"] == 0
    rv = _run_values(C, M, cx)
    for w in range(W):
        Xw = X[:, window_columns(C, M, cx, w)]
        sk = _sk_fit(oracle.poly_kernel(Xw, Xw, rv, P), y[:, w], ks[w])
        n = int(res["n_sv"][w])
        assert np.array_equal(res["support"][w, :n], sk.support_), (name, w)
        assert np.array_equal(res["n_support"][w], sk._n_support), (name, w)
        assert np.max(np.abs(res["dual_coef"][w, :, :n] - sk._dual_coef_)) <= 1e-12, (name, w)
        assert np.max(np.abs(res["intercept"][w] - sk._intercept_)) <= 1e-12, (name, w)
        assert _close(res["prob_a"][w], sk._probA, 1e-10) and _close(res["prob_b"][w], sk._probB, 1e-10), (name, w)


def _e2e_data(seed, C=190, M=45, cx=5, A=3):
    W = C // M
    rng = np.random.RandomState(seed)
    f = rng.uniform(0.05, 0.95, (A, C))

    def split(n):
        y = np.empty((n, W), np.int32)
        for i in range(n):
            cut = rng.randint(0, W + 1)
            y[i, :cut], y[i, cut:] = rng.randint(A), rng.randint(A)
        y[:2 * A] = np.tile(np.arange(A), 2)[:, None]
        anc = np.repeat(y, M, axis=1)
        anc = np.concatenate([anc, np.repeat(anc[:, -1:], C - W * M, axis=1)], axis=1)
        X = (rng.uniform(size=(n, C)) < f[anc, np.arange(C)[None, :]]).astype(np.int8)
        X[rng.uniform(size=X.shape) < 0.01] = 2
        return X, y

    return (C, M, cx, A), (split(60), split(40), split(30))


@pytest.mark.parametrize("base_name,tag", [("string_kernel", "string_kernel"), ("poly_string_kernel", "poly_kernel")])
def test_trains_end_to_end_with_the_references_seeds_and_keeps_its_kind(ctx, tmp_path, base_name, tag):
    from gnomix_amd import HipGnomix, GnxModelData
    from gnomix_amd.train import untrained_model, svc_window_kernel, train_svc_arrays, SVC_SEED_HIGH
    (C, M, cx, A), data = _e2e_data(seed=11)
    W, k = C // M, 4242
    model = HipGnomix(untrained_model(C, M, A, 5, cx, "fast", base=base_name, seed=1), ctx=ctx)
    np.random.seed(k)
    model.train(data=data, retrain_base=False, evaluate=True)
    info = model.base.train_info
    first = np.random.RandomState(k).randint(SVC_SEED_HIGH, size=W).astype(np.uint32)
    assert info["n_guarded"] == 0 and np.array_equal(info["seeds"], first)
    assert "smooth_train_acc" in model.accuracies and model.accuracies["base_train_acc"] > 100.0 / A
    dd = model.dev.data
    assert dd.base_kind == "covrsk" and all(svc_window_kernel(s) == tag for s in dd.svc)
    # the base is the fit train_svc_arrays makes with those seeds
    res, _ = train_svc_arrays(data[0][0], data[0][1], M, cx, A, first, kernel=tag, ctx=ctx)
    for w in range(W):
        assert np.array_equal(dd.svc[w]["dual_coef"], res["dual_coef"][w, :, :int(res["n_sv"][w])]), w
    X_q = data[2][0]
    p, lab = model.predict_proba(X_q), model.predict(X_q)
    assert np.isfinite(p).all()
    path = str(tmp_path / (base_name + ".gnx"))
    model.save(path)
    again = HipGnomix(GnxModelData.load(path), ctx=ctx)
    assert all(svc_window_kernel(s) == tag for s in again.dev.data.svc)
    assert np.array_equal(again.predict_proba(X_q), p) and np.array_equal(again.predict(X_q), lab)
    # a second fit of the loaded, tagged model keeps its kind and parameters, draws W seeds and leaves the generator there
    before = [dict(s) for s in again.dev.data.svc]
    np.random.seed(k + 1)
    again.train_base(np.concatenate([s[0] for s in data]), np.concatenate([s[1] for s in data]))
    ref = np.random.RandomState(k + 1)
    assert np.array_equal(again.base.train_info["seeds"], ref.randint(SVC_SEED_HIGH, size=W).astype(np.uint32))
    st, st_ref = np.random.get_state(), ref.get_state()
    assert np.array_equal(st[1], st_ref[1]) and st[2] == st_ref[2]           # no CovRSK re-seeding (np.random.seed(37) + draws)
    for w, (a, b) in enumerate(zip(again.dev.data.svc, before)):
        assert svc_window_kernel(a) == tag
        if tag == "poly_kernel":
            assert float(a["poly_p"]) == float(b["poly_p"]) == P and np.array_equal(a["run_value"], b["run_value"]) and "ms" not in a
        else:
            assert np.array_equal(a["ms"], b["ms"]) and np.array_equal(a["ms"], np.arange(1, again.data.window_width(w) + 1))
    assert np.isfinite(again.predict_proba(X_q)).all()
    # HipGnomix.train's retrain step leaves the generator alone too: W seeds per fit, nothing else drawn
    np.random.seed(k + 2)
    again.train(data=data, retrain_base=True, evaluate=False)
    ref = np.random.RandomState(k + 2)
    ref.randint(SVC_SEED_HIGH, size=W)
    assert np.array_equal(again.base.train_info["seeds"], ref.randint(SVC_SEED_HIGH, size=W).astype(np.uint32))
    assert all(svc_window_kernel(s) == tag for s in again.dev.data.svc)


def test_rejections_write_nothing(ctx):
    from gnomix_amd import _lib
    from gnomix_amd.convert import poly_run_values

    def call(X, y, C, M, cx, A, p=P, rv="table", n_rv=None, kind=1, entry="poly"):
        N, W, Pn = X.shape[0], C // M, A * (A - 1) // 2
        outs = [np.full(W, -7, np.int32), np.full((W, A), -7, np.int32), np.full((W, N), -7, np.int32),
                np.full((W, A - 1, N), -7.0), np.full((W, Pn), -7.0), np.full((W, Pn), -7.0), np.full((W, Pn), -7.0)]
        seeds = np.zeros(W, np.uint32)
        info = _lib.SvcTrainInfo()
        prm = _lib.SvcParams(kind, 0, 1.0, 0.0)
        table = poly_run_values(M + 2 * cx + C % M, P)["run_value"] if isinstance(rv, str) else rv
        n_rv = (0 if table is None else len(table)) if n_rv is None else n_rv
        if entry == "poly":
            rc = ctx.lib.gnx_train_svc_poly(ctx.h, X.ctypes.data, N, C, y.ctypes.data, C, M, cx, A, C_.byref(prm), p,
                                            None if table is None else table.ctypes.data, n_rv, seeds.ctypes.data,
                                            *(o.ctypes.data for o in outs), C_.byref(info))
        else:
            rc = ctx.lib.gnx_train_svc2(ctx.h, X.ctypes.data, N, C, y.ctypes.data, C, M, cx, A, C_.byref(prm), seeds.ctypes.data,
                                        *(o.ctypes.data for o in outs), C_.byref(info))
        if rc != _lib.GNX_OK:
            assert all((o == -7).all() for o in outs), "a refused call wrote its outputs"
        return rc, ctx.lib.gnx_last_error(ctx.h).decode()

    rng = np.random.RandomState(0)
    X = rng.randint(0, 2, size=(30, 130)).astype(np.int8)
    y = np.ascontiguousarray(np.tile(np.arange(3), 10)[:, None].repeat(2, axis=1).astype(np.int32))
    # a window wider than the LDS-derived bound: 8 191 SNPs (8 192 run values of 8 bytes = 64 KiB)
    Xw = rng.randint(0, 2, size=(30, 16384)).astype(np.int8)
    rc, msg = call(Xw, y, 16384, 8192, 0, 3)
    assert rc == _lib.GNX_EINVAL and "8191" in msg and "LDS" in msg
    rc, msg = call(Xw[:, :16382], y, 16382, 8191, 0, 3)          # the bound itself is accepted by that check: the fit runs
    assert rc == _lib.GNX_OK, msg
    for bad_p in (0.0, -1.2, float("nan")):
        rc, msg = call(X, y, 130, 60, 5, 3, p=bad_p)
        assert rc == _lib.GNX_EINVAL and "poly_p" in msg
    rc, msg = call(X, y, 130, 60, 5, 3, rv=None)
    assert rc == _lib.GNX_EINVAL and "run_value" in msg
    rc, msg = call(X, y, 130, 60, 5, 3, n_rv=80)                 # the last window is 80 SNPs wide: 81 values needed
    assert rc == _lib.GNX_EINVAL and "81" in msg
    missing = y.copy()
    missing[missing[:, 1] == 2, 1] = 0
    rc, msg = call(X, missing, 130, 60, 5, 3)
    assert rc == _lib.GNX_EINVAL and "class 2" in msg
    rc, msg = call(X, y, 130, 60, 5, 3, kind=2)                  # the poly entry takes the poly kind only
    assert rc == _lib.GNX_EINVAL
    rc, msg = call(X, y, 130, 60, 5, 3, entry="svc2")
    assert rc == _lib.GNX_EUNSUPPORTED and "gnx_train_svc_poly" in msg
    rc, msg = call(X, y, 130, 60, 5, 3)
    assert rc == _lib.GNX_OK, msg
    # gnx_svc_gram holds the same bounds
    G = np.full((1, 30, 30), -7, np.float32)
    rv = poly_run_values(8192, P)["run_value"]
    rc = ctx.lib.gnx_svc_gram(ctx.h, Xw.ctypes.data, 30, 16384, 16384, 8192, 0, 1, P, rv.ctypes.data, len(rv), 0, 1, G.ctypes.data)
    assert rc == _lib.GNX_EINVAL and "8191" in ctx.lib.gnx_last_error(ctx.h).decode() and (G == -7).all()
    rc = ctx.lib.gnx_svc_gram(ctx.h, X.ctypes.data, 30, 130, 130, 60, 5, 3, P, None, 0, 0, 1, G.ctypes.data)
    assert rc == _lib.GNX_EINVAL and (G == -7).all()             # the RBF kind has no string-kernel Gram
