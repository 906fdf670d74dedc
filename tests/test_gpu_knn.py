"""The 1-nearest-neighbour base (KNNBase) on the MI355X: k_knn_argmin (csrc/knn/k_base_knn.hip) against tests/knn_exact.py — integer
distances, ties to the lowest fit-row index — with EXACT equality on every cell, against the reference's own KNNBase output (G22)
on every cell whose nearest label is unambiguous, and against a live KNeighborsClassifier by membership in its tied set; the edge
shapes of the kernel's tiling, the 2-bit entry points, training / save / load / command line end to end, and the C ABI's refusals."""
import os

import numpy as np
import pytest

from conftest import load_golden
import knn_exact as KE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _model(C, M, A, cx, wins):
    from gnomix_amd.train import untrained_model
    d = untrained_model(C, M, A, 1, cx, "default", base="knn")
    d.knn_X = d.knn_y = None
    d.knn = [dict(xfit=np.ascontiguousarray(x, dtype=np.int8), y=np.ascontiguousarray(y, dtype=np.int32)) for x, y in wins]
    return d


def _check(dev, Xq, wins, C, M, cx, A, what):
    """both outputs of the base pass equal the restatement exactly, on every cell -> (B float64, restatement's chosen rows)"""
    ref, idx, amb = KE.predict(Xq, wins, C, M, cx, A)
    b32, b64 = dev.base_predict(Xq, want_f32=True, want_f64=True)
    print(what, "cells %d, differing f64 %d f32 %d, label-ambiguous %d" % (ref[..., 0].size, int((b64 != ref).any(-1).sum()),
                                                                          int((b32 != ref).any(-1).sum()), int(amb.sum())))
    assert b64.dtype == np.float64 and b32.dtype == np.float32
    assert np.array_equal(b64, ref) and np.array_equal(b32, ref.astype(np.float32))
    return b64, idx, amb


def test_equals_the_restatement_everywhere_and_the_references_KNNBase_G22_where_unambiguous(ctx):
    from gnomix_amd import DeviceModel
    g = load_golden("G22_knn.npz")
    C, M, A, cx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    wins = [(g["w%d_fit_X" % w], g["w%d_y" % w]) for w in range(C // M)]
    dev = DeviceModel(_model(C, M, A, cx, wins), ctx=ctx)
    B, idx, amb = _check(dev, g["Xq"], wins, C, M, cx, A, "G22")
    assert np.array_equal(amb, g["ambiguous"])
    assert (~amb).mean() >= 0.98                       # at least 98 % of the cells are compared with the reference
    assert np.array_equal(B[~amb], g["B"][~amb])
    # the shared form (what training stores) cuts the same windows
    from gnomix_amd.train import untrained_model, train_knn_base
    d = untrained_model(C, M, A, 1, cx, "default", base="knn")
    train_knn_base(d, g["Xt"], g["yt"])
    assert np.array_equal(DeviceModel(d, ctx=ctx).base_predict(g["Xq"])[1], B)


def _queries(rng, N, C, fitX):
    """random rows with 5 % missing, some of the fit rows themselves (distance 0), an all-missing row, an all-zero row (|x|^2 = 0:
    padded fit rows would tie at 0 unless masked) and an all-one row"""
    Xq = rng.randint(0, 2, (N, C)).astype(np.int8)
    Xq[rng.uniform(size=Xq.shape) < 0.05] = 2
    k = min(5, len(fitX))
    Xq[3:3 + k] = fitX[rng.choice(len(fitX), k, replace=False)]
    Xq[0], Xq[1], Xq[2] = 2, 0, 1
    Xq[N - 1] = 0                                      # the last row of the last, partial query tile too
    return Xq


@pytest.mark.parametrize("n_fit", [1, 63, 64, 65, 127, 128, 129, 130, 257])
def test_fit_row_counts_around_the_tile_sizes(ctx, n_fit):
    """padded rows (n_fit up to the next multiple of 128) never win; rows on both sides of the 16-, 32-, 64- and 128-row boundaries
    are found.  C = 203, M = 40, ctx = 7: widths 54 / 57 (no multiple of 64), the last window with its remainder, the first and
    last windows reflect-padded; 70 queries = one full 64-query tile and a partial one"""
    from gnomix_amd import DeviceModel
    C, M, cx, A = 203, 40, 7, 3
    rng = np.random.RandomState(n_fit)
    X = rng.randint(0, 3, (n_fit, C)).astype(np.int8)
    if n_fit > 1:
        X[-1] = 0                                      # the last real row is all zeros: the all-zero query must find IT, not a padded row
    y = rng.randint(0, A, (n_fit, C // M))
    wins = KE.shared_windows(X, y, C, M, cx)
    Xq = _queries(rng, 70, C, X)
    B, idx, amb = _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), Xq, wins, C, M, cx, A, "n_fit=%d" % n_fit)
    assert idx.max() < n_fit and (n_fit == 1 or (idx[1] == np.array([np.flatnonzero(~xf.any(1))[0] for xf, _ in wins])).all())


def test_two_classes_a_class_missing_from_a_window_and_other_row_counts_per_window(ctx):
    from gnomix_amd import DeviceModel
    rng = np.random.RandomState(5)
    for A in (2, 5):
        C, M, cx = 131, 30, 4
        W = C // M
        wins = []
        for w in range(W):
            width = M + 2 * cx + (C % M if w == W - 1 else 0)
            n = [7, 130, 64, 33][w]
            yw = rng.randint(0, A, n)
            if w == 1:
                yw[yw == A - 1] = 0                    # window 1 has no row of the last class: a zero column
            wins.append((rng.randint(0, 3, (n, width)).astype(np.int8), yw))
        Xq = _queries(rng, 37, C, np.zeros((1, C), np.int8))
        B, idx, amb = _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), Xq, wins, C, M, cx, A, "A=%d" % A)
        assert not B[:, 1, A - 1].any() and np.all(B.sum(-1) == 1.0)


TILES = [
    # name, C, M, ctx -> widths (M + 2 ctx, + rem), the widest row pitch, the query tile
    ("tile64_limit", 2490, 1200, 600, 64),     # 2400 / 2490 -> pitch 2496: the widest that keeps 64 queries
    ("tile32_first", 2550, 1230, 615, 32),     # 2460 / 2550 -> 2560
    ("tile32_limit", 5050, 2480, 1240, 32),    # 4960 / 5050 -> 5056
    ("tile16_first", 5100, 2500, 1250, 16),    # 5000 / 5100 -> 5120
    ("tile16_widest", 8192, 4000, 2000, 16),   # 8000 / 8192 = GNX_RBF_MAX_WIDTH
]


def _query_tile(C, M, cx):
    """the query tile the loader picks (k_base_knn.hip: the largest of 64 / 32 / 16 whose LDS working set — 36 bytes per query and
    the query tile at a pitch of 16 bytes more than the widest row — fits 160 KB), restated so that the cases provably reach every
    instantiation and both sides of each threshold"""
    kp = (M + 2 * cx + C % M + 63) // 64 * 64
    return next((qb for qb in (64, 32, 16) if qb * 36 + qb * (kp + 16) <= 160 * 1024), 0)


@pytest.mark.parametrize("name,C,M,cx,tile", TILES, ids=[t[0] for t in TILES])
def test_every_query_tile_size(ctx, name, C, M, cx, tile):
    from gnomix_amd import DeviceModel
    assert _query_tile(C, M, cx) == tile
    A = 4
    rng = np.random.RandomState(len(name) + C)
    X = rng.randint(0, 3, (70, C)).astype(np.int8)
    y = rng.randint(0, A, (70, C // M))
    wins = KE.shared_windows(X, y, C, M, cx)
    Xq = _queries(rng, 37, C, X)                       # 37 queries: a partial tile at every size
    _check(DeviceModel(_model(C, M, A, cx, wins), ctx=ctx), Xq, wins, C, M, cx, A, name)


def test_planted_ties_go_to_the_lowest_index_and_stay_inside_sklearns_tied_set(ctx):
    """duplicate fit rows with DIFFERENT labels, placed so that every stage of the reduction has to break a tie: the two column
    tiles of a wave (2 / 18), two lanes of one tile (1 / 9), different waves of one 128-row step (3 / 40 / 100), different steps
    (5 / 133 / 260), and a lower index in a LATER wave of an EARLIER step than its duplicate (100 / 130, 127 / 128)"""
    from sklearn.neighbors import KNeighborsClassifier
    from gnomix_amd import DeviceModel
    C, M, cx, A = 203, 40, 7, 4
    W = C // M
    rng = np.random.RandomState(9)
    n_fit = 300
    X = rng.randint(0, 2, (n_fit, C)).astype(np.int8)
    y = rng.randint(0, A, (n_fit, W))
    groups = [(2, 18), (1, 9), (3, 40, 100, 130), (5, 133, 260), (127, 128), (250, 299)]
    for gset in groups:
        for k, r in enumerate(gset):
            X[r] = X[gset[0]]
            y[r] = (y[gset[0]] + k) % A                # the duplicates carry different labels in every window
    wins = KE.shared_windows(X, y, C, M, cx)
    Xq = np.concatenate([X[[g[0] for g in groups]], X[[g[-1] for g in groups]], _queries(rng, 20, C, X)])
    near = X[[g[0] for g in groups]].copy()
    near[:, ::17] ^= 1                                 # equally far from every duplicate: ties at a distance > 0
    Xq = np.concatenate([Xq, near])
    dev = DeviceModel(_model(C, M, A, cx, wins), ctx=ctx)
    B, idx, amb = _check(dev, Xq, wins, C, M, cx, A, "planted ties")
    for k, gset in enumerate(groups):
        for q in (k, len(groups) + k, len(Xq) - len(groups) + k):
            assert (idx[q] == gset[0]).all()           # the restatement (and so the kernel) answers the lowest index of the group
            assert amb[q].all()
    # a live classifier: whichever neighbour it reports, the class chosen here is one of the classes at ITS minimum distance
    for w, (xf, yw) in enumerate(wins):
        m = KNeighborsClassifier(n_neighbors=1).fit(xf, yw)
        xq = Xq[:, KE.window_columns(C, M, cx, w)]
        dist, ind = m.kneighbors(xq, n_neighbors=n_fit)
        mine = np.argmax(B[:, w], -1)
        for q in range(len(Xq)):
            tied = set(yw[ind[q][dist[q] == dist[q, 0]]].tolist())
            assert tied == KE.tied_classes(xq[q:q + 1], xf, yw)[0]
            assert mine[q] in tied and m.predict(xq[q:q + 1])[0] in tied


def test_int8_and_2bit_entry_points_agree_bit_for_bit_including_code_3(ctx):
    import torch
    from gnomix_amd import DeviceModel
    C, M, cx, A = 331, 60, 11, 3
    rng = np.random.RandomState(4)
    X = rng.randint(0, 3, (150, C)).astype(np.int8)
    y = rng.randint(0, A, (150, C // M))
    wins = KE.shared_windows(X, y, C, M, cx)
    Xq = rng.randint(0, 4, (70, C)).astype(np.int8)    # code 3, the largest a 2-bit row can hold, is the number 3
    Xq[0] = 3
    dev = DeviceModel(_model(C, M, A, cx, wins), ctx=ctx)
    B, idx, amb = _check(dev, Xq, wins, C, M, cx, A, "code 3")
    P = torch.from_numpy(np.ascontiguousarray(dev.pack_x(Xq))).cuda()
    assert np.array_equal(dev.base_predict_packed_device(P, f64=True).cpu().numpy(), B)
    assert np.array_equal(dev.base_predict_packed_device(P, f64=False).cpu().numpy(), B.astype(np.float32))
    assert np.array_equal(dev.base_predict_device(torch.from_numpy(Xq).cuda(), f64=True).cpu().numpy(), B)
    p, l = dev.infer(Xq)
    p2, l2 = dev.infer_packed(dev.pack_x(Xq))
    assert np.array_equal(p, p2) and np.array_equal(l, l2)


def _e2e_data(seed):
    """three splits at C = 295, M = 24 (W = 12, remainder 7), context 5, A = 3: ancestry-dependent allele frequencies, labels in
    tracts"""
    C, M, cx, A = 295, 24, 5, 3
    W = C // M
    rng = np.random.RandomState(seed)
    f = rng.uniform(0.05, 0.95, (A, C))

    def split(n):
        y = np.empty((n, W), np.int32)
        for i in range(n):
            cut = rng.randint(0, W + 1)
            y[i, :cut], y[i, cut:] = rng.randint(A), rng.randint(A)
        y[:A] = np.arange(A)[:, None]
        anc = np.repeat(y, M, axis=1)
        anc = np.concatenate([anc, np.repeat(anc[:, -1:], C - W * M, axis=1)], axis=1)
        X = (rng.uniform(size=(n, C)) < f[anc, np.arange(C)[None, :]]).astype(np.int8)
        X[rng.uniform(size=X.shape) < 0.01] = 2
        return X, y

    return (C, M, cx, A), (split(80), split(60), split(40))


def test_trains_end_to_end_saves_loads_and_serves_the_command_line(ctx, tmp_path):
    import subprocess
    import sys
    from gnomix_amd import HipGnomix, GnxModelData, synth, vcfio
    from gnomix_amd.train import untrained_model
    (C, M, cx, A), data = _e2e_data(seed=7)
    # 1-NN on its own fit set is perfect when no two rows have identical window bytes with different labels: true for this seed
    for X, y in (data[0], (np.concatenate([d[0] for d in data]), np.concatenate([d[1] for d in data]))):
        for w, (xf, yw) in enumerate(KE.shared_windows(X, y, C, M, cx)):
            d2 = KE.d2_matrix(xf, xf)
            assert not ((d2 == 0) & (yw[:, None] != yw[None, :])).any(), w
    d = untrained_model(C, M, A, 5, cx, "default", base="knn", seed=1,
                        meta=dict(snp_pos=1000 + 37 * np.arange(C), snp_ref=np.array(["A"] * C), snp_alt=np.array(["C"] * C),
                                  pop_order=["p%d" % a for a in range(A)]))
    d.gen_map_pos, d.gen_map_cm = np.array([1, 400_000]), np.array([0.0, 1.3])
    model = HipGnomix(d, ctx=ctx)
    model.train(data=data, retrain_base=True, evaluate=True)
    print("accuracies", model.accuracies)
    assert model.accuracies["base_train_acc"] == 100.0 and model.accuracies["base_train_acc_bal"] == 100.0
    assert model.accuracies["base_val_acc"] > 100.0 / A and "smooth_train_acc" in model.accuracies
    dd = model.dev.data
    assert dd.base_kind == "knn" and dd.knn_X.shape == (180, C) and dd.knn_y.shape == (180, C // M)   # retrained on everything
    allX, ally = np.concatenate([s[0] for s in data]), np.concatenate([s[1] for s in data])
    assert np.array_equal(np.argmax(model.base.predict_proba(allX), -1), ally)
    X_q = data[2][0][:40]
    p, lab = model.predict_proba(X_q), model.predict(X_q)
    Xp, Yp = model.phase(X_q)                                        # Gnofix's initial base pass
    assert np.isfinite(p).all()
    path = str(tmp_path / "knn.gnx")
    model.save(path)
    again = HipGnomix(GnxModelData.load(path), ctx=ctx)
    assert np.array_equal(again.predict_proba(X_q), p) and np.array_equal(again.predict(X_q), lab)
    Xp2, Yp2 = again.phase(X_q)
    assert np.array_equal(Xp, Xp2) and np.array_equal(Yp, Yp2)
    vcf = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X_q), len(X_q) // 2, dd.snp_pos, dd.snp_ref, dd.snp_alt, chrom="22")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gnomix.py"), vcf, str(tmp_path / "out"), "22", "False", path],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    msp = [ln.split("\t") for ln in open(tmp_path / "out" / "query_results.msp").read().splitlines()[2:]]
    assert len(msp) == C // M and (tmp_path / "out" / "query_results.fb").exists()
    assert np.array_equal(np.array([[int(v) for v in row[6:]] for row in msp]).T, lab)   # the file path answers the same labels


def test_the_c_abi_refuses_what_the_header_says(ctx):
    from gnomix_amd import DeviceModel, _lib
    C, M, cx, A = 131, 30, 4, 3
    W = C // M
    rng = np.random.RandomState(2)

    def wins():
        return [(rng.randint(0, 3, (9, M + 2 * cx + (C % M if w == W - 1 else 0))).astype(np.int8), rng.randint(0, A, 9)) for w in range(W)]

    def refused(ws, code, says, geom=(C, M, A, cx)):
        with pytest.raises(_lib.GnxError) as e:
            DeviceModel(_model(*geom, ws), ctx=ctx)
        assert e.value.code == code and says in str(e.value), str(e.value)

    DeviceModel(_model(C, M, A, cx, wins()), ctx=ctx)              # the base kind loads
    for bad in (3, -1, 127):
        ws = wins()
        ws[2][0][4, 7] = bad
        refused(ws, _lib.GNX_EINVAL, "0..2")
    for bad in (A, -1):
        ws = wins()
        ws[1][1][3] = bad
        refused(ws, _lib.GNX_EINVAL, "[0, A)")
    ws = wins()
    ws[3] = (ws[3][0][:0], ws[3][1][:0])
    refused(ws, _lib.GNX_EINVAL, "n_fit")
    ws = wins()
    ws[0] = (ws[0][0][:, :-1], ws[0][1])
    refused(ws, _lib.GNX_EINVAL, "width")
    # wider than GNX_RBF_MAX_WIDTH: valid in the reference, not built here
    Cw, Mw, cw = 8193, 4000, 2000
    refused([(np.zeros((1, 8000), np.int8), np.zeros(1, np.int32)), (np.zeros((1, 8193), np.int8), np.zeros(1, np.int32))],
            _lib.GNX_EUNSUPPORTED, "GNX_RBF_MAX_WIDTH", geom=(Cw, Mw, A, cw))
    # base_kind GNX_BASE_KNN without windows
    d = _model(C, M, A, cx, wins())
    desc, keep = d.to_desc()
    desc.knn = None
    import ctypes
    h = ctypes.c_void_p()
    assert ctx.lib.gnx_model_load(ctx.h, ctypes.byref(desc), ctypes.byref(h)) == _lib.GNX_EINVAL and not h.value
    # a description of the previous ABI version is refused whole
    desc, keep = d.to_desc()
    desc.abi_version = 15
    assert ctx.lib.gnx_model_load(ctx.h, ctypes.byref(desc), ctypes.byref(h)) == _lib.GNX_EINVAL and not h.value
    # nothing was half-loaded: the context still serves a good model
    ws = wins()
    dev = DeviceModel(_model(C, M, A, cx, ws), ctx=ctx)
    _check(dev, rng.randint(0, 3, (5, C)).astype(np.int8), ws, C, M, cx, A, "after refusals")
