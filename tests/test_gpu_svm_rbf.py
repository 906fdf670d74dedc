"""The RBF SVC base (SVMBase: SVC(C=100, gamma=0.001, probability=True)) on the MI355X: inference (k_rbf_dec: squared distances on
the int8 matrix cores, kernel values from the host-built exp table) against the reference's own fit (G21) and live sklearn fits,
the trainer (gnx_train_svc2 with GNX_SVC_KERNEL_RBF) against sklearn on the same seed and against G21, HipGnomix.train end to end,
refusals.  Bars: B within 1e-12 of predict_proba (README "Parity"); support_ / n_support_ identical, _dual_coef_ / _intercept_
within 1e-12, _probA / _probB within 1e-10 (relative), n_guarded == 0."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import yaml

from conftest import load_golden
import svm_rbf_exact as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "tests", "golden", "G21_sim")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300) + 1e-300)


def _model(C, M, A, cx, svc):
    from gnomix_amd.train import untrained_model
    d = untrained_model(C, M, A, 1, cx, "default", base="svm")
    d.svc = svc
    return d


def _panel(rng, N, C, A, W, miss=0.02, counts=None):
    y = np.empty((N, W), np.int32)
    for w in range(W):
        col = np.concatenate([np.arange(A), rng.randint(0, A, N - A)]) if counts is None else np.repeat(np.arange(A), counts)
        y[:, w] = rng.permutation(col)
    f = rng.uniform(0.1, 0.9, (A, C))
    X = np.empty((N, C), np.int8)
    M = C // W
    for w in range(W):
        c0, c1 = w * M, (C if w == W - 1 else (w + 1) * M)
        X[:, c0:c1] = rng.uniform(size=(N, c1 - c0)) < f[y[:, w]][:, c0:c1]
    X[rng.uniform(size=X.shape) < miss] = 2
    return X, y


def test_inference_equals_the_references_SVMBase_G21(ctx):
    from gnomix_amd import DeviceModel
    g = load_golden("G21_svm_rbf.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    dev = DeviceModel(_model(C, M, A, cx, E.golden_windows(g)), ctx=ctx)
    _, B = dev.base_predict(g["Xq"])
    err = np.max(np.abs(B - g["B"]))
    print("G21 inference: max |B - predict_proba| = %.3g" % err)
    assert err <= 1e-12 and np.array_equal(np.argmax(B, -1), np.argmax(g["B"], -1))


INFER = [
    # name, N train, N query, C, M, ctx, A
    ("A2_one_snp_context", 50, 70, 203, 40, 1, 2),        # widths 42 / 45
    ("A3_width_not_16", 60, 33, 263, 50, 9, 3),           # 68 / 81
    ("A7_wide", 140, 129, 1990, 900, 450, 7),             # 1800 / 1990: row pitch 2048, the widest that keeps the 64-query tile at A = 7
    ("A12", 120, 65, 99, 40, 3, 12),                      # 46 / 65
    ("A7_tile32", 140, 97, 2381, 1150, 575, 7),           # 2300 / 2381: row pitch 2304 / 2432 -> k_rbf_dec<32> (chr22's tile at M = 1000)
    ("A2_tile16", 30, 41, 4937, 2450, 1225, 2),           # 4900 / 4937: row pitch 4928 / 4992 -> k_rbf_dec<16>
]
# the query tile the loader picks (k_base_rbf.hip: the largest of 64 / 32 / 16 whose LDS working set fits 160 KB), restated so that
# the cases above provably reach every instantiation
TILE = {"A2_one_snp_context": 64, "A3_width_not_16": 64, "A7_wide": 64, "A12": 64, "A7_tile32": 32, "A2_tile16": 16}


def _query_tile(C, M, cx, A):
    P, kp = A * (A - 1) // 2, (M + 2 * cx + C % M + 63) // 64 * 64
    for qb in (64, 32, 16):
        if (P * qb * 8 + 15) // 16 * 16 + qb * 264 + qb * (kp + 16) <= 160 * 1024:
            return qb
    return 0


@pytest.mark.parametrize("name,Nt,Nq,C,M,cx,A", INFER, ids=[g[0] for g in INFER])
def test_inference_against_live_sklearn(ctx, name, Nt, Nq, C, M, cx, A):
    import torch
    from sklearn.svm import SVC
    from gnomix_amd import DeviceModel
    from gnomix_amd.convert import svc_window_from_sklearn
    from gnomix_amd.train import window_columns
    rng = np.random.RandomState(zlib.crc32(name.encode()) % 1000)
    W = C // M
    assert _query_tile(C, M, cx, A) == TILE[name]
    X, y = _panel(rng, Nt, C, A, W)
    Xq, _ = _panel(rng, Nq, C, A, W, miss=0.05)
    fits = [SVC(C=100., gamma=0.001, probability=True, random_state=np.random.RandomState(w)).fit(X[:, window_columns(C, M, cx, w)], y[:, w])
            for w in range(W)]
    d = _model(C, M, A, cx, [svc_window_from_sklearn(m, len(window_columns(C, M, cx, w))) for w, m in enumerate(fits)])
    dev = DeviceModel(d, ctx=ctx)
    _, B = dev.base_predict(Xq)
    ref = np.stack([m.predict_proba(Xq[:, window_columns(C, M, cx, w)]) for w, m in enumerate(fits)], axis=1)
    err = np.max(np.abs(B - ref))
    print(name, "max |B - predict_proba| = %.3g" % err)
    assert err <= 1e-12 and np.array_equal(np.argmax(B, -1), np.argmax(ref, -1))
    # the 2-bit entry: bit-identical
    P = torch.from_numpy(np.ascontiguousarray(dev.pack_x(Xq))).cuda()
    Bp = dev.base_predict_packed_device(P, f64=True).cpu().numpy()
    assert np.array_equal(Bp, B)
    p, l = dev.infer(Xq)
    p2, l2 = dev.infer_packed(dev.pack_x(Xq))
    assert np.array_equal(p, p2) and np.array_equal(l, l2)


def test_single_support_vector_per_class_and_query_code_3(ctx):
    """a window whose classes hold one support vector each; packed rows may hold code 3: it is HANDLED as the number 3 (the header's
    contract), identically by both entries, and equals the restatement"""
    import torch
    from gnomix_amd import DeviceModel
    rng = np.random.RandomState(3)
    C, M, cx, A = 131, 60, 7, 3
    P = A * (A - 1) // 2
    svc = []
    for w in range(C // M):
        width = M + 2 * cx + (C % M if w == C // M - 1 else 0)
        n_sup = np.ones(A, np.int32) if w == 0 else np.array([3, 1, 2], np.int32)
        n = int(n_sup.sum())
        svc.append(dict(xfit=rng.randint(0, 3, (n, width)).astype(np.int8), support=np.arange(n, dtype=np.int32),
                        dual_coef=rng.uniform(-100, 100, (A - 1, n)), intercept=rng.normal(size=P), prob_a=-rng.uniform(0.5, 3, P),
                        prob_b=rng.normal(0, 0.3, P), n_support=n_sup, kernel=np.array("rbf"), gamma=np.float64(0.003)))
    dev = DeviceModel(_model(C, M, A, cx, svc), ctx=ctx)
    Xq = rng.randint(0, 4, (70, C)).astype(np.int8)
    _, B = dev.base_predict(Xq)
    ref = E.predict_proba(svc, Xq, C, M, cx)
    err = np.max(np.abs(B - ref))
    print("one vector per class / code 3: max |B - restatement| = %.3g" % err)
    assert err <= 1e-12 and np.array_equal(np.argmax(B, -1), np.argmax(ref, -1))
    Pk = torch.from_numpy(np.ascontiguousarray(dev.pack_x(Xq))).cuda()
    assert np.array_equal(dev.base_predict_packed_device(Pk, f64=True).cpu().numpy(), B)


TRAIN = [
    # name, N, C, M, ctx, A, how
    ("A2_partial", 40, 203, 40, 7, 2, "plain"),
    ("A3_tied_rows", 46, 260, 50, 9, 3, "dup"),
    ("A7_fold_without_positives", 70, 150, 30, 5, 7, "imbalanced"),
    ("A12", 96, 99, 40, 3, 12, "plain"),
    ("l_over_2000", 2200, 45, 40, 0, 2, "plain"),
]


@pytest.mark.parametrize("name,N,C,M,cx,A,how", TRAIN, ids=[g[0] for g in TRAIN])
def test_training_against_sklearn_on_the_same_seed(ctx, name, N, C, M, cx, A, how):
    from sklearn.svm import SVC
    from gnomix_amd.train import train_svc_arrays, window_columns, SVC_SEED_HIGH
    rng = np.random.RandomState(zlib.crc32(name.encode()) % 1000)
    W = C // M
    counts = [40, 3, 4, 6, 1, 10, 6] if how == "imbalanced" else None
    X, y = _panel(rng, N, C, A, W, counts=counts)
    if how == "dup":
        X[N // 2:] = X[:N - N // 2]           # every row twice: tied kernel rows
    ks = [100 + w for w in range(W)]
    seeds = np.array([np.random.RandomState(k).randint(SVC_SEED_HIGH) for k in ks], np.uint32)
    if how == "imbalanced":
        # the name is true: under these seeds' fold permutations (libsvm's own, gnx_svc_fold_permutation) some fold's training part
        # holds no row of one of the pair's classes (the one-row class guarantees it; counted over every window and pair)
        from gnomix_amd.train import svc_fold_permutation
        empty = 0
        for w in range(W):
            n_of = np.bincount(y[:, w], minlength=A)
            for i in range(A):
                for j in range(i + 1, A):
                    l, perm = int(n_of[i] + n_of[j]), svc_fold_permutation(seeds[w], int(n_of[i] + n_of[j]))
                    for f in range(5):
                        b, e = f * l // 5, (f + 1) * l // 5
                        rest = np.concatenate([perm[:b], perm[e:]])
                        empty += int((rest < n_of[i]).sum() == 0 or (rest >= n_of[i]).sum() == 0)
        print(name, "folds whose training part lacks a class:", empty)
        assert empty >= W
    res, info = train_svc_arrays(X, y, M, cx, A, seeds, kernel="rbf", gamma=0.001, C=100.0, ctx=ctx)
    print(name, {k: info[k] for k in ("smo_iterations", "n_solves", "n_guarded", "gram_ms", "smo_ms", "platt_ms")})
    assert info["n_guarded"] == 0
    for w in range(W):
        Xw = X[:, window_columns(C, M, cx, w)]
        sk = SVC(C=100., gamma=0.001, probability=True, random_state=np.random.RandomState(ks[w])).fit(Xw, y[:, w])
        n = int(res["n_sv"][w])
        assert np.array_equal(res["support"][w, :n], sk.support_), (name, w)
        assert np.array_equal(res["n_support"][w], sk._n_support), (name, w)
        print(name, w, "dual %.3g icpt %.3g" % (np.max(np.abs(res["dual_coef"][w, :, :n] - sk._dual_coef_)),
                                                np.max(np.abs(res["intercept"][w] - sk._intercept_))))
        assert np.max(np.abs(res["dual_coef"][w, :, :n] - sk._dual_coef_)) <= 1e-12, (name, w)
        assert np.max(np.abs(res["intercept"][w] - sk._intercept_)) <= 1e-12, (name, w)
        assert _close(res["prob_a"][w], sk._probA, 1e-10) and _close(res["prob_b"][w], sk._probB, 1e-10), (name, w)
    if name == "l_over_2000":
        assert info["smo_iterations"] > 6 * 1000   # enough iterations per solve for shrinking to run


def test_training_reproduces_the_references_fit_G21(ctx):
    from gnomix_amd import DeviceModel
    from gnomix_amd.base import HipBase
    from gnomix_amd.train import untrained_model
    g = load_golden("G21_svm_rbf.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    base = HipBase(DeviceModel(untrained_model(C, M, A, 1, cx, "default", base="svm"), ctx=ctx))
    np.random.seed(int(g["np_seed"]))
    base.train(g["Xt"], g["yt"])
    info = base.train_info
    assert info["n_guarded"] == 0 and np.array_equal(info["seeds"], g["seeds"])
    d = base.dev.data
    for w in range(C // M):
        s = d.svc[w]
        assert np.array_equal(info["support"][w], g["w%d_support" % w]), w
        assert np.array_equal(s["n_support"], g["w%d_n_support" % w]), w
        assert np.max(np.abs(s["dual_coef"] - g["w%d_dual" % w])) <= 1e-12, w
        assert np.max(np.abs(s["intercept"] - g["w%d_intercept" % w])) <= 1e-12, w
        assert _close(s["prob_a"], g["w%d_probA" % w], 1e-10) and _close(s["prob_b"], g["w%d_probB" % w], 1e-10), w
        assert float(s["gamma"]) == float(g["w%d_gamma" % w])
    B = base.predict_proba(g["Xq"])
    assert np.max(np.abs(B - g["B"])) <= 1e-12 and np.array_equal(np.argmax(B, -1), np.argmax(g["B"], -1))


@pytest.fixture(scope="module")
def sim_data(ctx):
    from gnomix_amd import simulate as S
    with open(os.path.join(SIM, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    plan = S.plan_splits(os.path.join(SIM, "panel.vcf.gz"), os.path.join(SIM, "gmap.tsv"), os.path.join(SIM, "smap.tsv"), cfg, chm="22")
    M = plan.window_size(cfg["model"]["window_size_cM"])
    context = int(M * cfg["model"]["context_ratio"])
    meta = {"snp_pos": plan.meta["pos_snps"], "snp_ref": plan.meta["ref_snps"], "snp_alt": plan.meta["alt_snps"], "pop_order": plan.pop_order}
    return plan, plan.materialise(ctx, M=M), M, context, meta, cfg


def test_svm_base_trains_end_to_end(ctx, sim_data, tmp_path):
    from gnomix_amd import HipGnomix, GnxModelData
    from gnomix_amd import simulate as S
    from gnomix_amd.model import svc_window_is_rbf
    from gnomix_amd.train import untrained_model
    plan, data, M, context, meta, cfg = sim_data
    d = untrained_model(plan.C, M, plan.A, int(cfg["model"]["smooth_size"]), context, "default", seed=cfg["seed"], meta=meta, base="svm")
    gmap = S.read_genetic_map(os.path.join(SIM, "gmap.tsv"), "22")
    d.gen_map_pos, d.gen_map_cm = gmap["pos"].to_numpy(np.int64), gmap["pos_cm"].to_numpy(np.float64)
    model = HipGnomix(d, ctx=ctx)
    np.random.seed(cfg["seed"])
    model.train(data=data, retrain_base=True, evaluate=True)
    assert model.base.train_info["n_guarded"] == 0
    assert set(model.Confusion_Matrices) >= {"train"} and "smooth_train_acc" in model.accuracies
    assert model.dev.data.base_kind == "covrsk" and all(svc_window_is_rbf(s) for s in model.dev.data.svc)
    X_q = data[0][0][:40]
    p, lab = model.predict_proba(X_q), model.predict(X_q)
    Xp, Yp = model.phase(X_q)
    assert np.isfinite(p).all()
    path = str(tmp_path / "svm.gnx")
    model.save(path)
    again = HipGnomix(GnxModelData.load(path), ctx=ctx)
    assert np.array_equal(again.predict_proba(X_q), p) and np.array_equal(again.predict(X_q), lab)
    Xp2, Yp2 = again.phase(X_q)
    assert np.array_equal(Xp, Xp2) and np.array_equal(Yp, Yp2)
    q = os.path.join(SIM, "panel.vcf.gz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gnomix.py"), q, str(tmp_path / "out"), "22", "False", path],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out" / "query_results.msp").exists() and (tmp_path / "out" / "query_results.fb").exists()


def test_refusals(ctx):
    import ctypes as C_
    from gnomix_amd import DeviceModel, _lib
    g = load_golden("G21_svm_rbf.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    good = E.golden_windows(g)
    DeviceModel(_model(C, M, A, cx, good), ctx=ctx)   # GNX_SVC_KERNEL_RBF loads
    for bad in (0.0, -0.001, float("nan"), float("inf")):
        svc = [dict(s) for s in good]
        svc[2]["gamma"] = np.float64(bad)
        with pytest.raises(_lib.GnxError) as e:
            DeviceModel(_model(C, M, A, cx, svc), ctx=ctx)
        assert e.value.code == _lib.GNX_EINVAL and "gamma" in str(e.value)
    svc = [dict(s) for s in good]
    svc[1]["xfit"] = svc[1]["xfit"].copy()
    svc[1]["xfit"][0, 5] = 3
    with pytest.raises(_lib.GnxError) as e:
        DeviceModel(_model(C, M, A, cx, svc), ctx=ctx)
    assert e.value.code == _lib.GNX_EINVAL and "0..2" in str(e.value)
    svc = [dict(s) for s in good]
    svc[3] = dict(svc[3], ms=np.array([1, 4], np.int32))
    del svc[3]["kernel"]
    with pytest.raises(_lib.GnxError) as e:   # every window of a model has the same kernel
        DeviceModel(_model(C, M, A, cx, svc), ctx=ctx)
    assert e.value.code == _lib.GNX_EINVAL
    # the trainer: gamma / C out of range, and the old entry (no gamma) refuses the RBF kind; nothing is written
    X, y = np.ascontiguousarray(g["Xt"]), np.ascontiguousarray(g["yt"])
    N, W, P = X.shape[0], C // M, A * (A - 1) // 2

    def call(entry, arg):
        outs = [np.full(W, -7, np.int32), np.full((W, A), -7, np.int32), np.full((W, N), -7, np.int32),
                np.full((W, A - 1, N), -7.0), np.full((W, P), -7.0), np.full((W, P), -7.0), np.full((W, P), -7.0)]
        info = _lib.SvcTrainInfo()
        rc = getattr(ctx.lib, entry)(ctx.h, X.ctypes.data, N, C, y.ctypes.data, C, M, cx, A, arg, g["seeds"].ctypes.data,
                                     *(o.ctypes.data for o in outs), C_.byref(info))
        assert all((o == -7).all() for o in outs), "a refused call wrote its outputs"
        return rc

    for gamma, cost in ((0.0, 100.0), (-1.0, 100.0), (float("nan"), 100.0), (0.001, 0.0), (0.001, float("inf"))):
        assert call("gnx_train_svc2", C_.byref(_lib.SvcParams(_lib.SVC_KERNEL_RBF, 0, cost, gamma))) == _lib.GNX_EINVAL
    assert call("gnx_train_svc", _lib.SVC_KERNEL_RBF) == _lib.GNX_EINVAL
    assert "gnx_train_svc2" in ctx.lib.gnx_last_error(ctx.h).decode()
