"""gnx_ancestry_assoc_logit[_dev / _gt2] (csrc/summary/k_ancestry_assoc_logit.hip) and the logistic association built on it, on the MI355X,
against the numpy restatement (tests/assoc_logit_exact.py).  tests/assoc_logit_cases.py states the shared inputs, the tolerance TOL_SE
(in units of the standard error) and where it was measured: on the CPU, against scikit-learn and a converged run, never against the device.

The integers are exact and equal the linear entry's.  Floating results: where the restatement has status 0, beta, se and theta within
TOL_SE se; the status and NaN patterns equal the restatement's.  The row forms, the host / device entries, sub-ranges and the file path
agree bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import assoc_logit_cases as LC
import assoc_logit_exact as LE

pytestmark = pytest.mark.gpu

GRID = [(n, M, A, K) for n in (1, 2, 63, 257) for M in (1, 37, 1000) for A in (2, 3, 7) for K in (1, 5)]
N_CHECK = 12      # SNPs per shape the restatement fits (the device fits them all; the integers are compared on all)


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _geometry(M):
    """C, W: two windows and a wider last one (one window at M = 1000)"""
    return {1: (7, 5), 37: (37 * 3 + 9, 3), 1000: (1003, 1)}[M]


def _case(n_ind, M, A, K):
    rng = np.random.RandomState(1000 + n_ind + 7 * M + 31 * A + K)
    C, W = _geometry(M)
    N = 2 * n_ind
    lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
    X = rng.choice([0, 1, 2, -1], size=(N, C), p=[0.5, 0.44, 0.03, 0.03]).astype(np.int8)
    y = rng.randint(0, 2, size=n_ind).astype(np.float64)
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, K - 1))], 1)
    use = np.ones(n_ind, np.uint8)
    if n_ind > 2:
        use[[1, n_ind - 1]] = 0
        y[2] = np.nan
        Z[n_ind // 3, K - 1] = np.nan
    return X, lab, y, Z, use


def _codes(X):
    return np.where((X == 0) | (X == 1), X, np.where(X == -1, 3, 2)).astype(np.uint8)


def _pack(X):
    """int8 rows -> 2-bit rows (SNP j = bits 2 (j % 4).. of byte j / 4)"""
    c = _codes(X)
    N, C = c.shape
    pad = np.zeros((N, (C + 3) // 4 * 4), np.uint8)
    pad[:, :C] = c
    q = pad.reshape(N, -1, 4)
    return np.ascontiguousarray(q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6))


def _host(ctx, X, lab, M, A, y, Z, use, c0=0, c1=None, min_ac=1, check=True):
    from gnomix_amd import assoc
    return assoc.logit_host(ctx, X, lab, M, A, y, Z, use, c0, X.shape[1] if c1 is None else c1, min_ac=min_ac, check=check)


def _dev(ctx, rows, kind, lab, M, A, C, y, Z, use, c0=0, c1=None, min_ac=1):
    """the _dev entry on torch tensors (labels with a row stride of W + 3) -> (rc, LogitFit)"""
    import torch
    from gnomix_amd import assoc
    c1 = C if c1 is None else c1
    N, W = lab.shape
    K = Z.shape[1]
    wide = np.full((N, W + 3), -7, np.int32)
    wide[:, :W] = lab
    t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (rows, wide, y, Z, use)]
    sf, si, th, wf, wi = assoc.logit_buffers(A, K, c0, c1, M, W, empty=lambda s, dt: torch.zeros(s, dtype=torch.float64 if dt == np.float64 else torch.int32,
                                                                                               device="cuda"))
    n_bad = ctypes.c_int64(0)
    torch.cuda.synchronize()
    rc = ctx.lib.gnx_ancestry_assoc_logit_dev(ctx.h, t[0].data_ptr(), kind, t[0].stride(0), t[1].data_ptr(), W + 3, N, C, M, W, A, t[2].data_ptr(),
                                              t[3].data_ptr(), K, t[4].data_ptr(), min_ac, c0, c1, 1e-10, 25, sf.data_ptr(), si.data_ptr(), th.data_ptr(),
                                              wf.data_ptr(), wi.data_ptr(), ctypes.byref(n_bad))
    return rc, assoc.split_logit(*(v.cpu().numpy() for v in (sf, si, th, wf, wi)), A, K, c0, c1, M, W, n_bad.value)


def _same(a, b, what=""):
    for name, u, v in zip(a._fields, a, b):
        if name != "n_bad":
            assert np.array_equal(u, v, equal_nan=True), (what, name)


def _against(got, want, rows, A, what):
    """got (LogitFit of the whole range) against the restatement on the SNPs `rows`; -> largest distance in se"""
    for name in ("n_alt", "n_alt_case", "n_miss"):
        assert np.array_equal(getattr(got, name), want[name]), (what, name)
    for name in ("n", "n_case", "sum_h", "status0"):
        assert np.array_equal(getattr(got, name), want[name]), (what, name)
    assert np.array_equal(got.status[rows], want["status"][rows]), (what, got.status[rows], want["status"][rows])
    bad = got.status != 0
    assert np.isnan(got.beta[bad]).all() and np.isnan(got.se[bad]).all() and np.isnan(got.dev[bad]).all() and np.isnan(got.theta[bad]).all(), what
    fitted = [c for c in rows if want["status"][c] == 0 and want["kappa"][c] <= LC.KAPPA_MAX]
    worst = LC.distance(got.beta, got.se, got.theta, want, fitted)
    assert worst <= LC.TOL_SE, (what, worst)
    ok0 = want["status0"] == 0
    assert np.isnan(got.theta0[~ok0]).all() and np.allclose(got.theta0[ok0], want["theta0"][ok0], rtol=1e-9, atol=1e-9)
    return worst, fitted


@pytest.mark.parametrize("n_ind,M,A,K", GRID)
def test_grid_against_the_restatement_and_the_linear_entry(ctx, n_ind, M, A, K):
    from gnomix_amd import assoc
    X, lab, y, Z, use = _case(n_ind, M, A, K)
    C, W = _geometry(M)
    rows = sorted(set(np.linspace(0, C - 1, N_CHECK).astype(int)))
    want = LE.fit(X, lab, M, A, y, Z, use, cols=set(rows))
    got = _host(ctx, X, lab, M, A, y, Z, use)
    worst, fitted = _against(got, want, rows, A, "host")
    print("n_ind %d M %d A %d K %d: %d of %d checked SNPs fitted, largest distance %.3g se" % (n_ind, M, A, K, len(fitted), len(rows), worst))
    # the integers of the linear entry on the same inputs
    st = assoc.stats_host(ctx, X, lab, M, A, np.nan_to_num(y, nan=np.nan), Z, use, 0, C)
    assert np.array_equal(got.n_alt, st.sum_d) and np.array_equal(got.n_miss, st.n_miss) and np.array_equal(got.n, st.n) and np.array_equal(got.sum_h, st.sum_h)
    # the device entry on int8 rows and on 2-bit rows: bit for bit
    rc, d8 = _dev(ctx, X, 0, lab, M, A, C, y, Z, use)
    assert rc == 0
    _same(got, d8, "int8 _dev")
    rc, d2 = _dev(ctx, _pack(X), 1, lab, M, A, C, y, Z, use)
    assert rc == 0
    _same(got, d2, "2-bit _dev")
    # independent optimum check: from the device's theta, g^T H^-1 g on the explicit design
    for c in fitted[:4]:
        _, D, yy = LE.design(X, lab, M, A, y, Z, use, c)
        kept = want["kept"][c]
        Dk, th = D[:, kept], got.theta[c][kept]
        mu = 1.0 / (1.0 + np.exp(-(Dk @ th)))
        g = Dk.T @ (yy - mu)
        H = (Dk * (mu * (1 - mu))[:, None]).T @ Dk
        assert float(g @ np.linalg.solve(H, g)) <= 1e-18, c


@pytest.mark.parametrize("A", [2, 3, 7])
def test_logit_case_against_the_restatement(ctx, A):
    X, lab, y, Z, use = LC.logit_case(A)
    want = LC.logit_fit(A)
    ok, left_out = LC.compared(want)
    assert left_out < 0.05
    got = _host(ctx, X, lab, LC.M, A, y, Z, use)
    worst, _ = _against(got, want, list(range(LC.C)), A, "logit_case")
    print("A = %d: largest distance %.3g se (TOL_SE %.3g), %d left out; iters up to %d" % (A, worst, LC.TOL_SE, (~ok).sum(), got.iters.max()))
    assert np.allclose(got.dev[ok], want["dev"][ok], rtol=1e-12) and (got.iters[ok] <= 25).all()
    for c in np.flatnonzero(ok)[::9]:
        _, D, yy = LE.design(X, lab, LC.M, A, y, Z, use, c)
        kept = want["kept"][c]
        Dk, th = D[:, kept], got.theta[c][kept]
        mu = 1.0 / (1.0 + np.exp(-(Dk @ th)))
        g = Dk.T @ (yy - mu)
        H = (Dk * (mu * (1 - mu))[:, None]).T @ Dk
        assert float(g @ np.linalg.solve(H, g)) <= 1e-18, c


def test_ranges_equal_slices_of_the_whole(ctx):
    X, lab, y, Z, use = LC.logit_case(3)
    whole = _host(ctx, X, lab, LC.M, 3, y, Z, use)
    w_all = np.minimum(np.arange(LC.C) // LC.M, LC.W - 1)
    for c0, c1 in ((13, 47), (77, 78), (95, LC.C), (100, LC.C)):
        for kind, rows in ((0, X), (1, _pack(X))):
            rc, got = _dev(ctx, rows, kind, lab, LC.M, 3, LC.C, y, Z, use, c0, c1)
            assert rc == 0
            for name in ("beta", "se", "dev", "theta", "n_alt", "n_alt_case", "n_miss", "iters", "status"):
                assert np.array_equal(getattr(got, name), getattr(whole, name)[c0:c1], equal_nan=True), (c0, c1, kind, name)
            ws = slice(w_all[c0], w_all[c1 - 1] + 1)
            for name in ("theta0", "dev0", "n", "n_case", "sum_h", "iters0", "status0"):
                assert np.array_equal(getattr(got, name), getattr(whole, name)[ws], equal_nan=True), (c0, c1, kind, name)


def test_designed_cases(ctx):
    X, lab, y, Z, use = (v.copy() for v in LC.logit_case(3))
    M, A, K = LC.M, 3, LC.K
    # a window whose participants are all cases; a window without ancestry A - 1
    y1 = y.copy()
    lab1 = lab.copy()
    lab1[:, 1][lab1[:, 1] == 2] = 0
    r = _host(ctx, X, lab1, M, A, y1, Z, use)
    assert r.status0[1] == 1 and (r.status[20:40] == 4).all() and np.isnan(r.beta[20:40]).all() and (r.status[:20] != 4).all()
    r = _host(ctx, X, lab, M, A, np.ones_like(y), Z, use)
    assert (r.status0 != 0).all() and (r.status == 4).all() and np.isnan(r.theta0).all() and np.isnan(r.dev0).all()
    # an ALT allele of ancestry 0 present in cases only: that term NaN, the others fitted
    Xo = X.copy()
    Xo[(lab[:, 0] == 0) & np.repeat(y == 0, 2), 0] = 0
    r = _host(ctx, Xo, lab, M, A, y, Z, use, 0, 1)
    assert r.status[0] == 0 and r.n_alt_case[0, 0] == r.n_alt[0, 0] > 0 and np.isnan(r.beta[0, 0]) and np.isnan(r.se[0, 0])
    assert not np.isnan(r.beta[0, 1:]).any() and r.theta[0, K + A - 1] == 0.0
    # min_ac above a column's count: dropped
    base = _host(ctx, X, lab, M, A, y, Z, use, 0, 1)
    big = int(base.n_alt[0].min()) + 1
    r = _host(ctx, X, lab, M, A, y, Z, use, 0, 1, min_ac=big)
    a = int(np.argmin(base.n_alt[0]))
    assert r.status[0] == 0 and np.isnan(r.beta[0, a]) and (~np.isnan(r.beta[0])).sum() == (base.n_alt[0] >= big).sum()
    # a covariate equal to y: complete separation
    r = _host(ctx, X, lab, M, A, y, np.concatenate([Z, y[:, None]], 1), use, 0, 5)
    assert (r.status0 == 3).all() and (r.status == 4).all()
    # quasi-complete separation at the SNP with ALT copies on both sides (one ancestry: no carrier is a case ... every homozygote is,
    # heterozygotes are both): the dosage term passes the column rule, the null model is fine, the fit has no finite optimum
    c = 3
    lab0 = np.zeros_like(lab)
    dd = (X[0::2, c] == 1).astype(int) + (X[1::2, c] == 1)
    ys = np.where(dd == 2, 1.0, np.where(dd == 0, 0.0, (np.arange(len(dd)) % 2).astype(np.float64)))
    want = LE.fit(X, lab0, M, 1, ys, Z, use, cols={c})
    r = _host(ctx, X, lab0, M, 1, ys, Z, use, c, c + 1)
    assert want["status0"][0] == 0 and want["status"][c] == 3 and r.status0[0] == 0 and r.status[0] == 3 and np.isnan(r.beta[0]).all()
    assert 0 < r.n_alt_case[0, 0] < r.n_alt[0, 0]
    # n <= p_kept
    few = np.zeros_like(use)
    few[:5] = 1
    want = LE.fit(X, lab, M, A, y, Z[:, :1], few)
    r = _host(ctx, X, lab, M, A, y, Z[:, :1], few)
    # (status 2 is an integer rule, hence exact; with 5 individuals the fits that do run are saturated and their verdicts knife-edge)
    assert np.array_equal(r.status == 2, want["status"] == 2) and (r.status == 2).any() and np.array_equal(r.status0, want["status0"])
    assert np.array_equal(r.status == 4, want["status"] == 4)


def test_limits_and_refusals(ctx):
    from gnomix_amd import assoc, _lib
    # the largest supported (A, K): Q = 16 + 32 - 1 = 47
    A, K, n_ind, M = 16, 16, 63, 4
    rng = np.random.RandomState(5)
    C, W = 9, 2
    lab = rng.randint(0, A, size=(2 * n_ind, W)).astype(np.int32)
    lab[:8, :] = A - 1
    X = rng.randint(0, 2, size=(2 * n_ind, C)).astype(np.int8)
    y = rng.randint(0, 2, size=n_ind).astype(np.float64)
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, K - 1))], 1)
    want = LE.fit(X, lab, M, A, y, Z, None, cols={0, 5})
    got = _host(ctx, X, lab, M, A, y, Z, None)
    _against(got, want, [0, 5], A, "largest")
    print("A = 16, K = 16: status0 %s, status %s" % (got.status0.tolist(), got.status.tolist()))
    # refusals: sentinel-filled outputs stay untouched
    def call(A, K, y, Z, X=X, lab=lab):
        n_ind = len(y)
        sf, si, th, wf, wi = (np.full((64, 64), 7.5) if i in (0, 2, 3) else np.full((64, 64), 77, np.int32) for i in range(5))
        n_bad = ctypes.c_int64(-1)
        use = np.ones(n_ind, np.uint8)
        use[1] = 0
        rc = ctx.lib.gnx_ancestry_assoc_logit(ctx.h, X.ctypes.data, X.shape[1], lab.ctypes.data, lab.shape[1], X.shape[0], X.shape[1], M, W, A, y.ctypes.data,
                                              Z.ctypes.data, K, use.ctypes.data, 1, 0, X.shape[1], 1e-10, 25, sf.ctypes.data, si.ctypes.data, th.ctypes.data,
                                              wf.ctypes.data, wi.ctypes.data, ctypes.byref(n_bad))
        assert (sf == 7.5).all() and (th == 7.5).all() and (wf == 7.5).all() and (si == 77).all() and (wi == 77).all()
        return rc, n_bad.value, ctx.lib.gnx_last_error(ctx.h).decode()
    Z17 = np.ascontiguousarray(np.concatenate([Z, Z[:, :1]], 1))
    rc, _, msg = call(16, 17, y, Z17)
    assert rc == _lib.GNX_EUNSUPPORTED and "17" in msg and "48" in msg and "47" in msg
    rc, _, msg = call(17, 16, y, Z)
    assert rc == _lib.GNX_EUNSUPPORTED and "49" in msg
    yb = y.copy()
    yb[0], yb[1], yb[7] = 0.5, 0.25, 2.0          # individual 1 has use = 0: not counted
    rc, n_bad, msg = call(16, 16, yb, Z)
    assert rc == _lib.GNX_EINVAL and n_bad == 2 and "2 individuals" in msg
    for tol, mi in ((-1.0, 25), (np.nan, 25), (1e-10, 0)):
        with pytest.raises(_lib.GnxError):
            assoc.logit_host(ctx, X, lab, M, A, y, Z, None, 0, C, tol=tol, max_iter=mi)


def test_labels_out_of_range_are_reported_after_the_launch(ctx):
    X, lab, y, Z, use = LC.logit_case(3)
    bad = lab.copy()
    bad[14, 2], bad[41, 2], bad[40, 4] = 3, -1, 99        # individuals 7 and 20
    got = _host(ctx, X, bad, LC.M, 3, y, Z, use, check=False)
    assert got.n_bad == 3
    for w, n_bad, inds in ((2, 2, [7, 20]), (4, 1, [20])):       # the window concerned: as if those individuals had use = 0
        off = use.copy()
        off[inds] = 0
        ref = _host(ctx, X, lab, LC.M, 3, y, Z, off, w * LC.M, (w + 1) * LC.M if w < 5 else LC.C)
        rc_got = _host(ctx, X, bad, LC.M, 3, y, Z, use, w * LC.M, (w + 1) * LC.M, check=False)
        assert rc_got.n_bad == n_bad
        _same(ref, rc_got, "window %d" % w)
    from gnomix_amd import _lib
    with pytest.raises(_lib.GnxError, match="3 labels lie outside"):
        _host(ctx, X, bad, LC.M, 3, y, Z, use)
    assert _host(ctx, X, bad, LC.M, 3, y, Z, use, 0, 2 * LC.M).n_bad == 0


def test_model_surface(ga):
    import torch
    from gnomix_amd import synth
    d = synth.synthetic_model(C=1537, M=50, A=3, S=11, n_rounds=4, seed=5)
    X = synth.synthetic_X(160, d.C, seed=3, miss=0.03)
    rng = np.random.RandomState(1)
    n_ind = X.shape[0] // 2
    y = rng.randint(0, 2, size=n_ind).astype(np.float64)
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, 1))], 1)
    use = np.ones(n_ind, np.uint8)
    use[5] = 0
    g = ga.HipGnomix(d, device=0)
    lab = np.ascontiguousarray(g.predict(X), dtype=np.int32)
    rows = list(range(0, d.C, 127))
    want = LE.fit(X, lab, d.M, d.A, y, Z, use, cols=set(rows))
    got = g.ancestry_association(X, y, Z, use, model="logistic")
    assert type(got).__name__ == "AncestryAssocLogit" and got.beta.shape == (d.C, d.A) and got.status.dtype == np.int32
    assert np.array_equal(got.n_alt, want["n_alt"]) and np.array_equal(got.n_alt_case, want["n_alt_case"]) and np.array_equal(got.status[rows], want["status"][rows])
    win = np.minimum(np.arange(d.C) // d.M, d.W - 1)
    assert np.array_equal(got.n, want["n"][win]) and np.array_equal(got.n_hap, want["sum_h"][win])
    fitted = [c for c in rows if want["status"][c] == 0 and want["kappa"][c] <= LC.KAPPA_MAX]
    assert len(fitted) >= 3 and LC.distance(got.beta, got.se, None, want, fitted) <= LC.TOL_SE
    ok = got.status == 0
    assert np.allclose(got.lrt[fitted], (want["dev0"][win] - want["dev"])[fitted], rtol=1e-9, atol=1e-9) and (got.lrt_df[ok] == (~np.isnan(got.beta[ok])).sum(1)).all()
    assert np.array_equal(got.z, got.beta / got.se, equal_nan=True) and (got.df[ok] >= 1).all()
    got_t = g.ancestry_association(torch.from_numpy(X).cuda(), y, Z, use, model="logistic")
    for a, b in zip(got, got_t):
        assert np.array_equal(a, b, equal_nan=True)
    assert type(g.ancestry_association(X, y, Z, use)).__name__ == "AncestryAssoc"
    with pytest.raises(ValueError, match="model must be"):
        g.ancestry_association(X, y, Z, use, model="probit")
    with pytest.raises(ValueError, match="coded 0 / 1"):
        g.ancestry_association(X, y + 0.5, Z, use, model="logistic")
    g.dev.ctx.reset_stream()


def _phenotypes(path, samples, seed=4, bad=None):
    rng = np.random.RandomState(seed)
    lines = ["sample\tpheno\tage"]
    for i, s in enumerate(samples):
        if i == 1:
            continue
        ph = "NA" if i == 4 else ("0.5" if s == bad else str(rng.randint(0, 2)))
        lines.append("%s\t%s\t%.3f" % (s, ph, rng.uniform(20, 70)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def test_file_path_equals_the_matrix_path_whatever_the_batch(ga, tmp_path, monkeypatch):
    from gnomix_amd import synth, vcfio, _lib
    d = synth.synthetic_model(C=3112, M=100, A=3, S=11, n_rounds=4, seed=7)
    d.snp_pos, d.snp_ref = 1000 + 37 * np.arange(d.C), np.array(["A"] * d.C)
    X = synth.synthetic_X(120, d.C, seed=2, miss=0.03)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), 60, d.snp_pos, d.snp_ref, ["C"] * d.C)
    dev = ga.DeviceModel(d)
    vcf = vcfio.read_vcf(q, chm="22", ctx=dev.ctx)
    src, _, _ = vcfio.column_map(vcf, d.snp_pos, d.snp_ref, verbose=False)
    Xq = vcfio.vcf_to_npy(vcf, d.snp_pos, d.snp_ref, verbose=False).astype(np.int8)
    _, lab = dev.infer_gt2(vcf.gt2, 120, src, want_proba=False)
    rng = np.random.RandomState(3)
    y, Z = rng.randint(0, 2, size=60).astype(np.float64), np.concatenate([np.ones((60, 1)), rng.normal(size=(60, 1))], 1)
    use = np.ones(60, np.uint8)
    use[6] = 0
    want = dev.ancestry_assoc_logit_fit(Xq, lab, y, Z, use, 50, 3000)
    assert (want.status == 0).any()
    _same(want, dev.ancestry_assoc_logit_fit_gt2(vcf.gt2, 120, src, lab, y, Z, use, 50, 3000), "one batch")
    for batch in ("12", "44"):
        monkeypatch.setenv("GNX_HOST_BATCH", batch)
        ctx2 = _lib.Context(0)
        dev2 = ga.DeviceModel(d, ctx=ctx2)
        _same(want, dev2.ancestry_assoc_logit_fit_gt2(np.array(vcf.gt2), 120, src, lab, y, Z, use, 50, 3000), "batch " + batch)
        ctx2.close()
    monkeypatch.delenv("GNX_HOST_BATCH")


def test_command_line_writes_the_logistic_file_only_when_asked(ga, tmp_path):
    import dataclasses
    from gnomix_amd import assoc, synth, vcfio, cli
    from gnomix_amd import postprocess as pp
    d = synth.synthetic_model(C=1537, M=50, A=3, S=11, n_rounds=4, seed=5)
    X = synth.synthetic_X(120, d.C, seed=3, miss=0.03)
    pops = ["P%d" % a for a in range(d.A)]
    d = dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                            population_order=pops, gen_map_pos=np.array([1, 50_000, 200_000]), gen_map_cm=np.array([0.0, 1.5, 9.25]))
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    g = ga.HipGnomix(d, device=0)
    samples = [str(s) for s in vcfio.read_vcf(q, chm="22", ctx=g.dev.ctx)["samples"]]
    ph = _phenotypes(str(tmp_path / "pheno.tsv"), samples)

    def run(name, phase=False, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, **kw)
        return od
    absent = run("absent", ancestry_assoc_output=True, phenotype_file=ph)
    linear = run("linear", ancestry_assoc_output=True, phenotype_file=ph, ancestry_assoc_model="linear")
    logit = run("logit", ancestry_assoc_output=True, phenotype_file=ph, ancestry_assoc_model="logistic")
    assert sorted(os.listdir(str(absent))) == sorted(os.listdir(str(linear))) == ["query_results.assoc.tsv", "query_results.fb", "query_results.msp"]
    assert sorted(os.listdir(str(logit))) == ["query_results.assoc.logistic.tsv", "query_results.fb", "query_results.msp"]
    for f in os.listdir(str(absent)):
        assert (absent / f).read_bytes() == (linear / f).read_bytes()
    for f in ("query_results.fb", "query_results.msp"):
        assert (absent / f).read_bytes() == (logit / f).read_bytes()
    rows = [ln.split("\t") for ln in (logit / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)
    y, Z, use, _ = assoc.read_phenotypes(ph, samples)
    res = g.dev.ancestry_assoc_logit(X, lab, y, Z, use)
    pp.write_assoc_logit(str(tmp_path / "want"), "22", d.snp_pos, d.M, d.W, res, pops)
    text = (logit / "query_results.assoc.logistic.tsv").read_text()
    assert text == (tmp_path / "want.assoc.logistic.tsv").read_text() and len(text.splitlines()) == 1 + d.C and (res.status == 0).any()
    with pytest.raises(ValueError, match="phase=True"):
        run("phased", phase=True, ancestry_assoc_output=True, phenotype_file=ph, ancestry_assoc_model="logistic")
    assert os.listdir(str(tmp_path / "phased")) == []
    bad = _phenotypes(str(tmp_path / "bad.tsv"), samples, bad=samples[7])
    with pytest.raises(ValueError, match="sample '%s' has 0.5" % samples[7]):
        run("badpheno", ancestry_assoc_output=True, phenotype_file=bad, ancestry_assoc_model="logistic")
    assert "query_results.assoc.logistic.tsv" not in os.listdir(str(tmp_path / "badpheno"))
