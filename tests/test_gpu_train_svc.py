"""gnx_train_svc on the MI355X: the CovRSK SVC base (mode "best") fitted on the device equals sklearn's libsvm on the same Gram
matrix and seed.  Pinned to the reference's own fit (G2), compared with sklearn on random geometries, rejections, and
HipGnomix.train end to end on simulated data (tests/golden/G21_sim)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import yaml

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21 = os.path.join(ROOT, "tests", "golden", "G21_sim")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _g2_training_set(g):
    """the reference's training haplotypes (60 x 537) from its fitted windows' __Xfit (overlapping windows of the padded rows) and
    their labels from support_ / n_support (every row is a support vector in G2)"""
    C, M, A, ctx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    W = C // M
    Xp = np.full((60, C + 2 * ctx), -1, np.int16)
    y = np.full((60, W), -1, np.int32)
    for w in range(W):
        xf = g["w%d_Xfit" % w]
        Xp[:, w * M:w * M + xf.shape[1]] = xf
        y[g["w%d_support" % w], w] = np.repeat(np.arange(A), g["w%d_nsv" % w])
    X = Xp[:, ctx:ctx + C]
    assert (X >= 0).all() and (y >= 0).all()
    return X.astype(np.int8), y


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300) + 1e-300)


def test_G2_reference_fit_is_reproduced(ctx):
    from gnomix_amd import DeviceModel
    from gnomix_amd.base import HipBase
    from gnomix_amd.train import untrained_model
    g = load_golden("G2_covrsk.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    X, y = _g2_training_set(g)
    base = HipBase(DeviceModel(untrained_model(C, M, A, 5, cx, "best"), ctx=ctx))
    np.random.seed(11)
    base.train(X, y)
    info = base.train_info
    assert info["n_guarded"] == 0
    d = base.dev.data
    for w in range(C // M):
        s = d.svc[w]
        assert np.array_equal(info["support"][w], g["w%d_support" % w]), w
        assert np.array_equal(s["n_support"], g["w%d_nsv" % w]), w
        assert np.max(np.abs(s["dual_coef"] - g["w%d_dual" % w])) <= 1e-12, w
        assert np.max(np.abs(s["intercept"] - g["w%d_intercept" % w])) <= 1e-12, w
        assert _close(s["prob_a"], g["w%d_probA" % w], 1e-10) and _close(s["prob_b"], g["w%d_probB" % w], 1e-10), w
        assert np.array_equal(s["xfit"], g["w%d_Xfit" % w][info["support"][w]])
    B = base.predict_proba(g["X"])
    assert np.max(np.abs(B - g["B"])) <= 1e-12
    assert np.array_equal(np.argmax(B, -1), np.argmax(g["B"], -1))
    ref = np.random.RandomState(37)
    ref.rand(136)                    # the last window is 137 SNPs wide
    st, st_ref = np.random.get_state(), ref.get_state()
    assert np.array_equal(st[1], st_ref[1]) and st[2] == st_ref[2]


def _sk_fit(K, yw, k):
    """sklearn's fit on a precomputed Gram; RandomState(k) makes it draw the seed RandomState(k).randint(2**31 - 1)"""
    from sklearn.svm import SVC
    return SVC(kernel="precomputed", probability=True, random_state=np.random.RandomState(k)).fit(K.astype(np.float64), yw)


def _labels(rng, N, W, A, counts=None):
    y = np.empty((N, W), np.int32)
    for w in range(W):
        if counts is None:
            col = np.concatenate([np.arange(A), rng.randint(0, A, N - A)])
        else:
            col = np.repeat(np.arange(A), counts)
        y[:, w] = rng.permutation(col)
    return y


GEOMETRIES = [
    # name, N, C, M, ctx, A, kernel, how the rows / labels are drawn
    ("A2_partial_words", 40, 203, 40, 7, 2, "CovRSK", "plain"),
    ("A3_duplicated_rows", 45, 260, 50, 9, 3, "CovRSK", "dup"),
    ("A7_imbalanced", 70, 150, 30, 5, 7, "CovRSK", "imbalanced"),
    ("A12", 96, 99, 40, 3, 12, "CovRSK", "plain"),
    ("plain_string_kernel", 42, 203, 40, 7, 3, "string_kernel", "plain"),
    ("l_over_2000", 2200, 45, 40, 0, 2, "CovRSK", "plain"),
]


@pytest.mark.parametrize("name,N,C,M,cx,A,kernel,how", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_against_sklearn_on_random_geometries(ctx, oracle, name, N, C, M, cx, A, kernel, how):
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
    res, info = train_svc_arrays(X, y, M, cx, A, seeds, kernel=kernel, ctx=ctx)
    assert info["n_guarded"] == 0
    for w in range(W):
        Xw = X[:, window_columns(C, M, cx, w)]
        K = oracle.covrsk(Xw, Xw) if kernel == "CovRSK" else oracle.string_kernel(Xw, Xw)
        sk = _sk_fit(K, y[:, w], ks[w])
        n = int(res["n_sv"][w])
        assert np.array_equal(res["support"][w, :n], sk.support_), (name, w)
        assert np.array_equal(res["n_support"][w], sk._n_support), (name, w)
        assert np.max(np.abs(res["dual_coef"][w, :, :n] - sk._dual_coef_)) <= 1e-12, (name, w)
        assert np.max(np.abs(res["intercept"][w] - sk._intercept_)) <= 1e-12, (name, w)
        assert _close(res["prob_a"][w], sk._probA, 1e-10) and _close(res["prob_b"][w], sk._probB, 1e-10), (name, w)
    if name == "l_over_2000":
        assert info["smo_iterations"] > 6 * 1000   # enough iterations per solve for shrinking to run


def test_rejections_write_nothing(ctx):
    from gnomix_amd import _lib
    import ctypes as C_

    def call(X, y, C, M, cx, A, kind):
        N = X.shape[0]
        W = C // M
        P = A * (A - 1) // 2
        outs = [np.full(W, -7, np.int32), np.full((W, A), -7, np.int32), np.full((W, N), -7, np.int32),
                np.full((W, A - 1, N), -7.0), np.full((W, P), -7.0), np.full((W, P), -7.0), np.full((W, P), -7.0)]
        seeds = np.zeros(W, np.uint32)
        info = _lib.SvcTrainInfo()
        rc = ctx.lib.gnx_train_svc(ctx.h, X.ctypes.data, N, C, y.ctypes.data, C, M, cx, A, kind, seeds.ctypes.data,
                                   *(o.ctypes.data for o in outs), C_.byref(info))
        if rc != _lib.GNX_OK:
            assert all((o == -7).all() for o in outs), "a refused call wrote its outputs"
        return rc

    rng = np.random.RandomState(0)
    X = rng.randint(0, 2, size=(30, 130)).astype(np.int8)
    y = np.tile(np.arange(3), 10)[:, None].repeat(2, axis=1).astype(np.int32)
    missing = y.copy()
    missing[missing[:, 1] == 2, 1] = 0
    assert call(X, missing, 130, 60, 5, 3, 0) == _lib.GNX_EINVAL
    assert "class 2" in ctx.lib.gnx_last_error(ctx.h).decode()
    bad = y.copy()
    bad[3, 0] = 3
    assert call(X, bad, 130, 60, 5, 3, 0) == _lib.GNX_EINVAL
    assert call(X, y, 130, 60, 5, 3, 1) == _lib.GNX_EUNSUPPORTED
    Xw = rng.randint(0, 2, size=(30, 12000)).astype(np.int8)
    yw = np.tile(np.arange(3), 10)[:, None].repeat(2, axis=1).astype(np.int32)
    assert call(Xw, yw, 12000, 6000, 0, 3, 2) == _lib.GNX_EINVAL           # plain kernel, 6 000 SNPs: g = 18 M >= 2^24
    assert "2^24" in ctx.lib.gnx_last_error(ctx.h).decode()
    assert call(X, y, 130, 60, 5, 3, 0) == _lib.GNX_OK


@pytest.fixture(scope="module")
def sim_data(ctx):
    from gnomix_amd import simulate as S
    with open(os.path.join(G21, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    plan = S.plan_splits(os.path.join(G21, "panel.vcf.gz"), os.path.join(G21, "gmap.tsv"), os.path.join(G21, "smap.tsv"), cfg, chm="22")
    M = plan.window_size(cfg["model"]["window_size_cM"])
    context = int(M * cfg["model"]["context_ratio"])
    meta = {"snp_pos": plan.meta["pos_snps"], "snp_ref": plan.meta["ref_snps"], "snp_alt": plan.meta["alt_snps"], "pop_order": plan.pop_order}
    return plan, plan.materialise(ctx, M=M), M, context, meta, cfg


def test_best_model_trains_end_to_end(ctx, sim_data, tmp_path):
    from gnomix_amd import HipGnomix, GnxModelData
    from gnomix_amd.train import untrained_model
    plan, data, M, context, meta, cfg = sim_data
    from gnomix_amd import simulate as S
    d = untrained_model(plan.C, M, plan.A, int(cfg["model"]["smooth_size"]), context, "best", seed=cfg["seed"], meta=meta)
    gmap = S.read_genetic_map(os.path.join(G21, "gmap.tsv"), "22")
    d.gen_map_pos, d.gen_map_cm = gmap["pos"].to_numpy(np.int64), gmap["pos_cm"].to_numpy(np.float64)
    model = HipGnomix(d, ctx=ctx)
    np.random.seed(cfg["seed"])
    model.train(data=data, retrain_base=True, evaluate=True)
    assert set(model.Confusion_Matrices) >= {"train"} and "smooth_train_acc" in model.accuracies
    X_q = data[0][0][:40]
    p = model.predict_proba(X_q)
    assert np.isfinite(p).all() and model.dev.data.base_kind == "covrsk"
    path = str(tmp_path / "best.gnx")
    model.save(path)
    again = HipGnomix(GnxModelData.load(path), ctx=ctx)
    assert np.array_equal(again.predict_proba(X_q), p) and np.array_equal(again.predict(X_q), model.predict(X_q))
    # the command line infers with it (the query: the panel itself)
    q = os.path.join(G21, "panel.vcf.gz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gnomix.py"), q, str(tmp_path / "out"), "22", "False", path],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out" / "query_results.msp").exists() and (tmp_path / "out" / "query_results.fb").exists()


def test_compacted_xfit_predicts_like_the_full_training_rows(ctx, sim_data):
    """train_svc_base keeps only the support rows per window; a model holding every training row (support = raw indices) is the
    same classifier"""
    from gnomix_amd import DeviceModel
    from gnomix_amd.train import untrained_model, train_svc_base, window_columns
    plan, data, M, context, meta, cfg = sim_data
    X, y = data[0]
    d = untrained_model(plan.C, M, plan.A, 5, context, "best")
    info = train_svc_base(d, X, y, ctx=ctx, seeds=np.arange(d.W, dtype=np.uint32) + 5)
    full = untrained_model(plan.C, M, plan.A, 5, context, "best")
    full.svc = [dict(s, xfit=np.ascontiguousarray(X[:, window_columns(plan.C, M, context, w)]), support=info["support"][w])
                for w, s in enumerate(d.svc)]
    Xq = data[1][0][:64]
    _, b_small = DeviceModel(d, ctx=ctx).base_predict(Xq)
    _, b_full = DeviceModel(full, ctx=ctx).base_predict(Xq)
    assert np.array_equal(b_small, b_full)
