"""gnx_ancestry_assoc_stats[_dev / _gt2] (csrc/summary/k_ancestry_assoc.hip) and the association built on it, on the MI355X, against
the numpy restatement (tests/assoc_exact.py).

Exact statistics.  y and Z are integer-valued with |v| <= 1024: every product and partial sum is an integer below 2^53, so every block
is independent of the summation order and must equal the restatement's bit for bit.  C = 2 * 1024 + 37.  A wave owns TC adjacent SNPs
(64 for small blocks, 32 at A = 7 / K = 16, 16 at A = 32 / K = 1, 4 at A = 32 / K = 16: the tile that still fits 64 KiB of LDS);
M = 1 (a window per SNP), M = 37 (windows that start inside a tile, a wider last window), M = 1000.  The whole grid runs:
N / 2 in {1, 63, 257} x M x A in {2, 3, 7, 32} x K in {1, 16} x both row forms; int8 rows go through the host entry AND the device
entry, 2-bit rows through the device entry.  Every case has use zeros, a non-finite y, missing calls (bytes 2 and -1; 2-bit codes 2 and
3), a label row stride larger than W, poison behind every row, and a SNP range that starts and ends inside a tile.
The restatement's blocks of a shape are computed once and shared by its row forms.

Regression results: tests/assoc_cases.py states the inputs, the tolerance and where its constant comes from."""
import ctypes

import numpy as np
import pytest

import allele_counts_exact as AE
import assoc_cases as AC
import assoc_exact as XE

pytestmark = pytest.mark.gpu

C_EXACT = 2 * 1024 + 37
GRID = [(n, M, A, K) for n in (1, 63, 257) for M in (1, 37, 1000) for A in (2, 3, 7, 32) for K in (1, 16)]
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


def _case(n_ind, M, A, K):
    key = (n_ind, M, A, K)
    if key not in _inputs:
        rng = np.random.RandomState(n_ind + 7 * M + 31 * A + K)
        N, C = 2 * n_ind, C_EXACT
        W = C // M
        X = rng.choice([0, 1, 2, -1], size=(N, C), p=[0.5, 0.4, 0.06, 0.04]).astype(np.int8)
        lab = np.repeat(rng.randint(0, A, size=(N, W // 2 + 1)), 2, axis=1)[:, :W].astype(np.int32)
        y = rng.randint(-1024, 1025, size=n_ind).astype(np.float64)
        Z = rng.randint(-1024, 1025, size=(n_ind, K)).astype(np.float64)
        Z[:, 0] = 1
        use = np.ones(n_ind, np.uint8)
        if n_ind > 2:
            use[[1, n_ind - 1]] = 0
            y[2] = np.inf
            y[n_ind // 2] = np.nan
            Z[n_ind // 3, K - 1] = np.nan
        _inputs[key] = (X, np.ascontiguousarray(lab), y, Z, use)
    return _inputs[key]


def _expected(n_ind, M, A, K):
    """the restatement's blocks of the shape; only the latest shape is kept (the row forms of one shape run one after the other)"""
    key = (n_ind, M, A, K)
    if key not in _want:
        X, lab, y, Z, use = _case(*key)
        _want.clear()
        _want[key] = XE.blocks(X, lab, M, A, y, Z, use, 0, C_EXACT)
    return _want[key]


def _codes(X):
    """int8 bytes -> 2-bit codes: -1 becomes 3, every other missing byte 2"""
    return np.where((X == 0) | (X == 1), X, np.where(X == -1, 3, 2)).astype(np.uint8)


def _outputs(A, K, c0, c1, M, W, fill=0):
    from gnomix_amd import assoc
    NF, NI, NWF, NWI = assoc.layout(A, K)
    nc = c1 - c0
    nw = min((c1 - 1) // M, W - 1) - min(c0 // M, W - 1) + 1
    return (np.full((nc, NF), float(fill)), np.full((nc, NI), fill, np.int32), np.full((nw, NWF), float(fill)), np.full((nw, NWI), fill, np.int32))


def _stats(ctx, X, lab, M, A, y, Z, use, c0, c1, kind):
    """-> rc, (snp_f64, snp_i32, win_f64, win_i32), n_bad.  Poison behind every row, labels with a row stride larger than W.
    kind 0: int8 rows through the host entry; kind 1: 2-bit rows through the device entry; kind 2: int8 rows through the device entry"""
    N, C = X.shape
    W, K = lab.shape[1], Z.shape[1]
    out = _outputs(A, K, c0, c1, M, W)
    n_bad = ctypes.c_int64(-1)
    y, Z, use = np.ascontiguousarray(y), np.ascontiguousarray(Z), np.ascontiguousarray(use)
    if kind == 0:
        rows = np.full((N, C + 5), 1, np.int8)
        rows[:, :C] = X
        wide = np.full((N, W + 3), A, np.int32)
        wide[:, :W] = lab
        rc = ctx.lib.gnx_ancestry_assoc_stats(ctx.h, rows.ctypes.data, C + 5, wide.ctypes.data, W + 3, N, C, M, W, A, y.ctypes.data, Z.ctypes.data, K,
                                              use.ctypes.data, 1, c0, c1, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                              out[3].ctypes.data, ctypes.byref(n_bad))
        return rc, out, n_bad.value
    import torch
    if kind == 2:
        rows = torch.ones((N, C + 5), dtype=torch.int8, device="cuda")
        rows[:, :C] = torch.from_numpy(X).cuda()
    else:
        rows = torch.from_numpy(AE.pack2(_codes(X), ldp=(C + 3) // 4 + 3, fill=0x55)).cuda()
    wide = torch.full((N, W + 3), A, dtype=torch.int32, device="cuda")
    wide[:, :W] = torch.from_numpy(lab).cuda()
    t = [torch.from_numpy(v).cuda() for v in (y, Z, use)]
    o = [torch.from_numpy(v).cuda() for v in out]
    rc = ctx.lib.gnx_ancestry_assoc_stats_dev(ctx.h, rows.data_ptr(), 1 if kind == 1 else 0, rows.stride(0), wide.data_ptr(), W + 3, N, C, M, W, A, t[0].data_ptr(),
                                              t[1].data_ptr(), K, t[2].data_ptr(), 1, c0, c1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                              o[3].data_ptr(), ctypes.byref(n_bad))
    return rc, tuple(v.cpu().numpy() for v in o), n_bad.value


def _same(got, want, where=""):
    for g, w, name in zip(got, want, ("snp_f64", "snp_i32", "win_f64", "win_i32")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where)
        assert np.array_equal(g, w), (name, where)


# ---------------------------------------------------------------- exact statistics -------------------------------------------------
@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("n_ind,M,A,K", GRID)
def test_blocks_equal_the_restatement_bit_for_bit(ctx, n_ind, M, A, K, packed):
    X, lab, y, Z, use = _case(n_ind, M, A, K)
    want = _expected(n_ind, M, A, K)
    C, W = C_EXACT, C_EXACT // M
    assert (_codes(X) == 3).any() and (_codes(X) == 2).any()
    if n_ind > 2:
        assert want[3][:, 0].max() == n_ind - 5          # two use zeros, two non-finite y, one non-finite covariate
    for kind in ((1,) if packed else (0, 2)):
        rc, got, n_bad = _stats(ctx, X, lab, M, A, y, Z, use, 0, C, kind)
        assert rc == 0 and n_bad == 0, ctx.lib.gnx_last_error(ctx.h)
        _same(got, want[:4], "kind %d" % kind)
    # a range that starts and ends inside a tile (and inside a window where M > 1): the same slice of the whole-range call
    c0, c1 = 1024 - 19, 2 * 1024 + 5
    rc, part, n_bad = _stats(ctx, X, lab, M, A, y, Z, use, c0, c1, kind)
    assert rc == 0 and n_bad == 0
    w0, w1 = min(c0 // M, W - 1), min((c1 - 1) // M, W - 1)
    _same(part, (got[0][c0:c1], got[1][c0:c1], got[2][w0:w1 + 1], got[3][w0:w1 + 1]), "range")


def test_use_null_and_real_valued_sums_in_the_stated_order(ctx):
    n_ind, M, A, K = 63, 37, 3, 2
    X, lab, y, Z, use = _case(n_ind, M, A, K)
    # use == NULL: everybody whose values are finite takes part
    out = _outputs(A, K, 0, C_EXACT, M, C_EXACT // M)
    rc = ctx.lib.gnx_ancestry_assoc_stats(ctx.h, X.ctypes.data, C_EXACT, lab.ctypes.data, lab.shape[1], 2 * n_ind, C_EXACT, M, lab.shape[1], A,
                                          y.ctypes.data, Z.ctypes.data, K, None, 1, 0, C_EXACT, out[0].ctypes.data, out[1].ctypes.data,
                                          out[2].ctypes.data, out[3].ctypes.data, None)
    assert rc == 0
    _same(out, XE.blocks(X, lab, M, A, y, Z, None, 0, C_EXACT)[:4], "use NULL")
    # real-valued y and Z: the float64 blocks equal the sums taken in the stated order (ascending individuals, every product rounded
    # once, no fused multiply-add: a fused form differs in the window block's last bits), for every row form and entry
    Xr, labr, yr, Zr, user = AC.regression_case(3)
    c0, c1 = 13, 101
    wantf = XE.float_blocks_in_order(Xr, labr, AC.M, 3, yr, Zr, user, c0, c1)
    assert not np.array_equal(wantf[1], np.round(wantf[1]))
    for kind in (0, 1, 2):
        rc, got, _ = _stats(ctx, Xr, labr, AC.M, 3, yr, Zr, user, c0, c1, kind)
        assert rc == 0
        assert np.array_equal(got[0], wantf[0]) and np.array_equal(got[2], wantf[1]), "kind %d" % kind


# ---------------------------------------------------------------- consistency with what exists ------------------------------------
def test_sums_equal_the_dosage_matrices_and_the_allele_counts(ctx):
    from gnomix_amd import assoc, postprocess as pp
    n_ind, M, A, K = 63, 37, 7, 16
    X, lab, y, Z, use = _case(n_ind, M, A, K)
    st = assoc.stats_host(ctx, X, lab, M, A, y, Z, use, 0, C_EXACT)
    part = XE.participation(lab, A, y, Z, use)[:, AE.windows(C_EXACT, M, lab.shape[1])]
    for a in range(A):
        dos, hap = pp.ancestry_dosage(ctx, X, lab, M, A, a)
        assert np.array_equal(st.sum_d[:, a], (dos * part).sum(0)) and np.array_equal(st.sum_h[st.window][:, a], (hap * part).sum(0))
    # all individuals participating: the allele counts' tables
    yy, ZZ = np.where(np.isfinite(y), y, 0.0), np.where(np.isfinite(Z), Z, 0.0)
    st = assoc.stats_host(ctx, X, lab, M, A, yy, ZZ, None, 0, C_EXACT)
    counts = pp.allele_counts(ctx, X, lab, M, A)
    assert np.array_equal(st.sum_d.T, counts.n_alt) and np.array_equal(st.sum_h[st.window].T, counts.n_obs + counts.n_miss)
    assert np.array_equal(st.n_miss, counts.n_miss.sum(0)) and (st.n == n_ind).all()


# ---------------------------------------------------------------- regression results ------------------------------------------------
@pytest.mark.parametrize("A", [2, 3, 7])
def test_regression_results_against_lstsq(ctx, A):
    """beta, se and t within C_TOL p kappa^2 2^-53 max|beta| of numpy.linalg.lstsq on the full design (tests/assoc_cases.py)"""
    from gnomix_amd import assoc
    X, lab, y, Z, use = AC.regression_case(A)
    want = AC.regression_fit(A)
    got = assoc.assoc_from_stats(lambda c0, c1: assoc.stats_host(ctx, X, lab, AC.M, A, y, Z, use, c0, c1), AC.C, A, AC.K)
    for name in ("n_alt", "n_hap", "n", "df", "n_miss", "status"):
        assert np.array_equal(getattr(got, name), want[name]), name
    ratio, left_out = AC.ratios(got.beta, got.se, got.t, want)
    print("A = %d: largest err / (p kappa^2 2^-53 max|beta|) = %.4g (C_TOL = %.4g), SNPs left out %.3f" % (A, ratio, AC.C_TOL, left_out))
    assert left_out < 0.05
    assert ratio <= AC.C_TOL
    assert np.array_equal(np.isnan(got.p), np.isnan(got.t)) and (got.p[~np.isnan(got.p)] <= 1).all() and (got.p[~np.isnan(got.p)] >= 0).all()


def test_dropped_terms_and_statuses_agree_with_the_restatement(ctx):
    from gnomix_amd import assoc
    X, lab, y, Z, use = (v.copy() for v in AC.regression_case(3))
    X[:, 5] = 0                                  # no ALT: every dosage term dropped
    X[:, 6] = 1                                  # all ALT: d == h, rank-deficient
    X[:, 7] = np.where(lab[:, 0] == 1, 0, X[:, 7])      # window 0, ancestry 1 never ALT at SNP 7
    lab[:, 2] = np.where(lab[:, 2] == 0, 1, lab[:, 2])  # window 2: ancestry 0 absent (its hapcount column is dropped)
    want = XE.fit(X, lab, AC.M, 3, y, Z, use, min_ac=2)
    got = assoc.assoc_from_stats(lambda c0, c1: assoc.stats_host(ctx, X, lab, AC.M, 3, y, Z, use, c0, c1, min_ac=2), AC.C, 3, AC.K, min_ac=2)
    assert want["status"][6] == 1 and want["status"][5] == 0 and np.isnan(want["beta"][5]).all() and np.isnan(want["beta"][7, 1])
    assert np.array_equal(got.status, want["status"]) and np.array_equal(got.df, want["df"])
    for name in ("beta", "se", "t"):
        assert np.array_equal(np.isnan(getattr(got, name)), np.isnan(want[name])), name
    ok = ~np.isnan(want["beta"])
    assert np.allclose(got.beta[ok], want["beta"][ok], rtol=1e-9, atol=1e-12)
    use4 = np.zeros_like(use)
    use4[:5] = 1
    got = assoc.assoc_from_stats(lambda c0, c1: assoc.stats_host(ctx, X, lab, AC.M, 3, y, Z, use4, c0, c1), AC.C, 3, AC.K)
    want = XE.fit(X, lab, AC.M, 3, y, Z, use4)
    assert np.array_equal(got.status, want["status"]) and (got.status == 2).any() and np.isnan(got.beta[got.status == 2]).all()


# ---------------------------------------------------------------- errors ------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx):
    from gnomix_amd import _lib
    N, C, M, W, A, K = 4, 20, 5, 4, 3, 2
    X, lab = np.zeros((N, C), np.int8), np.zeros((N, W), np.int32)
    y, Z, use = np.zeros(N // 2), np.ones((N // 2, 17)), np.ones(N // 2, np.uint8)
    from gnomix_amd import assoc
    NF, NI, NWF, NWI = assoc.layout(33, 17)
    out = (np.full((C, NF), -7.0), np.full((C, NI), -7, np.int32), np.full((W, NWF), -7.0), np.full((W, NWI), -7, np.int32))
    n_bad = ctypes.c_int64(-7)
    lib, h = ctx.lib, ctx.h

    def call(X=X, N=N, M=M, W=W, A=A, K=K, min_ac=1, c0=0, c1=C, ld=C, ldl=W, y=y, Z=Z, o0=out[0], lab=lab):
        p = lambda v: None if v is None else v.ctypes.data
        return lib.gnx_ancestry_assoc_stats(h, p(X), ld, p(lab), ldl, N, C, M, W, A, p(y), p(Z), K, use.ctypes.data, min_ac, c0, c1, p(o0),
                                            out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, ctypes.byref(n_bad))
    assert call(N=3) == _lib.GNX_EINVAL                                   # odd N
    assert call(K=0) == _lib.GNX_EINVAL
    assert call(M=6) == _lib.GNX_EINVAL                                   # M W > C
    assert call(min_ac=0) == _lib.GNX_EINVAL
    assert call(X=None) == _lib.GNX_EINVAL and call(lab=None) == _lib.GNX_EINVAL and call(y=None) == _lib.GNX_EINVAL
    assert call(Z=None) == _lib.GNX_EINVAL and call(o0=None) == _lib.GNX_EINVAL
    assert call(c0=5, c1=5) == _lib.GNX_EINVAL and call(c1=C + 1) == _lib.GNX_EINVAL and call(c0=-1) == _lib.GNX_EINVAL
    assert call(ld=C - 1) == _lib.GNX_EINVAL and call(ldl=W - 1) == _lib.GNX_EINVAL
    assert call(A=33) == _lib.GNX_EUNSUPPORTED and b"33" in lib.gnx_last_error(h)
    assert call(K=17) == _lib.GNX_EUNSUPPORTED and b"17" in lib.gnx_last_error(h)
    assert all((v == -7).all() for v in out) and n_bad.value == -7
    import torch
    t = torch.zeros(8, dtype=torch.uint8, device="cuda")
    assert lib.gnx_ancestry_assoc_stats_dev(h, t.data_ptr(), 2, C, t.data_ptr(), W, N, C, M, W, A, t.data_ptr(), t.data_ptr(), K, None, 1, 0, C,
                                            t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None) == _lib.GNX_EINVAL      # row_kind
    assert (t == 0).all()
    assert call() == 0 and n_bad.value == 0


@pytest.mark.parametrize("kind", [0, 1])
def test_labels_out_of_range_are_reported_after_the_launch(ctx, kind):
    """such a label is compared, never used as an index: the individual takes no part at that window; every other value is what a run
    with that individual's use = 0 gives"""
    from gnomix_amd import _lib
    n_ind, M, A, K = 63, 37, 3, 2
    X, lab, y, Z, use = _case(n_ind, M, A, K)
    C, W = C_EXACT, C_EXACT // M
    bad = lab.copy()
    bad[2 * 7, 3], bad[2 * 7 + 1, 3], bad[2 * 20 + 1, 30] = A, -1, 1 << 20        # individual 7 twice at window 3, individual 20 at window 30
    rc, got, n_bad = _stats(ctx, X, bad, M, A, y, Z, use, 0, C, kind)
    assert rc == _lib.GNX_EINVAL and n_bad == 3 and b"3 labels lie outside [0, 3)" in ctx.lib.gnx_last_error(ctx.h)
    _same(got, XE.blocks(X, bad, M, A, y, Z, use, 0, C)[:4])
    rc, clean, n0 = _stats(ctx, X, lab, M, A, y, Z, use, 0, C, kind)
    assert rc == 0 and n0 == 0
    snps = np.ones(C, bool)
    snps[3 * M:4 * M] = False
    snps[30 * M:31 * M] = False
    wins = np.ones(W, bool)
    wins[[3, 30]] = False
    assert np.array_equal(got[0][snps], clean[0][snps]) and np.array_equal(got[1][snps], clean[1][snps])      # the windows not concerned
    assert np.array_equal(got[2][wins], clean[2][wins]) and np.array_equal(got[3][wins], clean[3][wins])
    for ind, w in ((7, 3), (20, 30)):                                     # the window concerned: as if the individual had use = 0
        off = use.copy()
        off[ind] = 0
        rc, ref, _ = _stats(ctx, X, lab, M, A, y, Z, off, w * M, (w + 1) * M, kind)
        assert rc == 0
        _same((got[0][w * M:(w + 1) * M], got[1][w * M:(w + 1) * M], got[2][w:w + 1], got[3][w:w + 1]), ref, "window %d" % w)
        assert got[3][w, 0] == clean[3][w, 0] - 1
    # a range that does not touch the windows reports nothing
    rc, _, n_bad = _stats(ctx, X, bad, M, A, y, Z, use, 31 * M, C, kind)
    assert rc == 0 and n_bad == 0


# ---------------------------------------------------------------- through the model ------------------------------------------------
def test_model_surface_follows_predict_and_device_tensors_equal_host_arrays(ga):
    import torch
    from gnomix_amd import synth
    d = synth.synthetic_model(C=3037, M=50, A=4, S=11, n_rounds=4, seed=5)
    X = synth.synthetic_X(120, d.C, seed=3, miss=0.03)
    rng = np.random.RandomState(1)
    n_ind = X.shape[0] // 2
    y = rng.normal(size=n_ind)
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, 2))], 1)
    use = np.ones(n_ind, np.uint8)
    use[5] = 0
    for mf in (0, 5):
        g = ga.HipGnomix(d, device=0, mode_filter=mf)
        lab = np.ascontiguousarray(g.predict(X), dtype=np.int32)
        want = XE.fit(X, lab, d.M, d.A, y, Z, use, cols=set(range(0, d.C, 97)))
        got = g.ancestry_association(X, y, Z, use)
        assert type(got).__name__ == "AncestryAssoc" and got.beta.shape == (d.C, d.A) and got.n.dtype == np.int32
        for name in ("n_alt", "n_hap", "n", "df", "n_miss"):
            assert np.array_equal(getattr(got, name), want[name]), name
        sel = want["status"] == 0
        solved = want["status"] >= 0
        print("mode_filter %d: %d SNPs solved by the restatement, %d of them fitted" % (mf, solved.sum(), sel.sum()))
        assert sel.sum() >= 1 and np.array_equal(got.status[solved], want["status"][solved])
        assert np.array_equal(np.isnan(got.beta[sel]), np.isnan(want["beta"][sel]))
        ok = sel[:, None] & ~np.isnan(want["beta"]) & (want["kappa"] <= AC.KAPPA_MAX)[:, None]
        assert np.allclose(got.beta[ok], want["beta"][ok], rtol=1e-8, atol=1e-10) and np.allclose(got.se[ok], want["se"][ok], rtol=1e-8, atol=1e-10)
        got_t = g.ancestry_association(torch.from_numpy(X).cuda(), y, Z, use)
        for a, b in zip(got, got_t):
            assert np.array_equal(a, b, equal_nan=True)
    dev = g.dev
    Xt = torch.from_numpy(X).cuda()
    host = dev.ancestry_assoc_stats(X, lab, y, Z, use, 100, 2100)
    for rows_t in (Xt, dev.pack_device(Xt)):
        st = dev.ancestry_assoc_stats(rows_t, torch.from_numpy(lab).cuda(), y, Z, use, 100, 2100)
        for a, b in zip(host[:10], st[:10]):
            assert np.array_equal(a, b)
    icpt = dev.ancestry_assoc(X, lab, y)                    # Z = None: the intercept only
    ones = dev.ancestry_assoc(X, lab, y, np.ones((n_ind, 1)))
    assert np.array_equal(icpt.beta, ones.beta, equal_nan=True) and (icpt.df[icpt.status == 0] <= n_ind - 2).all()
    with pytest.raises(ValueError):
        dev.ancestry_assoc(X, lab, y, min_ac=0)
    dev.ctx.reset_stream()


# ---------------------------------------------------------------- the file path and the command line --------------------------------
def _phenotypes(path, samples, seed=4):
    """a phenotype file for the samples but the second (unknown to the file), one missing phenotype, one sample the query lacks"""
    rng = np.random.RandomState(seed)
    lines = ["sample\tpheno\tage"]
    for i, s in enumerate(samples):
        if i == 1:
            continue
        lines.append("%s\t%s\t%.3f" % (s, "NA" if i == 4 else "%.5f" % rng.normal(), rng.uniform(20, 70)))
    lines.append("nobody\t1.0\t33")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def test_file_path_blocks_equal_the_matrix_path_whatever_the_batch(ga, tmp_path, monkeypatch):
    from gnomix_amd import synth, vcfio, _lib
    d = synth.synthetic_model(C=4112, M=100, A=3, S=11, n_rounds=4, seed=7)
    d.snp_pos, d.snp_ref = 1000 + 37 * np.arange(d.C), np.array(["A"] * d.C)
    X = synth.synthetic_X(34, d.C, seed=2, miss=0.03)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), 17, d.snp_pos, d.snp_ref, ["C"] * d.C)
    dev = ga.DeviceModel(d)
    vcf = vcfio.read_vcf(q, chm="22", ctx=dev.ctx)
    src, _, _ = vcfio.column_map(vcf, d.snp_pos, d.snp_ref, verbose=False)
    Xq = vcfio.vcf_to_npy(vcf, d.snp_pos, d.snp_ref, verbose=False).astype(np.int8)
    _, lab = dev.infer_gt2(vcf.gt2, 34, src, want_proba=False)
    rng = np.random.RandomState(3)
    y, Z = rng.normal(size=17), np.concatenate([np.ones((17, 1)), rng.normal(size=(17, 2))], 1)
    use = np.ones(17, np.uint8)
    use[6] = 0
    want = dev.ancestry_assoc_stats(Xq, lab, y, Z, use, 50, 4000)
    got = dev.ancestry_assoc_stats_gt2(vcf.gt2, 34, src, lab, y, Z, use, 50, 4000)
    for a, b in zip(want[:10], got[:10]):
        assert np.array_equal(a, b)
    # several batches of individuals: each goes on from the sums of those before it, bit for bit the same blocks
    monkeypatch.setenv("GNX_HOST_BATCH", "12")
    ctx2 = _lib.Context(0)
    dev2 = ga.DeviceModel(d, ctx=ctx2)
    got = dev2.ancestry_assoc_stats_gt2(np.array(vcf.gt2), 34, src, lab, y, Z, use, 50, 4000)
    for a, b in zip(want[:10], got[:10]):
        assert np.array_equal(a, b)
    ctx2.close()
    monkeypatch.delenv("GNX_HOST_BATCH")
    bad = lab.copy()
    bad[3, 5] = d.A
    with pytest.raises(_lib.GnxError, match="1 labels lie outside"):
        dev.ancestry_assoc_stats_gt2(vcf.gt2, 34, src, bad, y, Z, use)
    with pytest.raises(_lib.GnxError):
        dev.ancestry_assoc_stats_gt2(vcf.gt2, 34, src, lab, y, Z, use, min_ac=0)


def test_command_line_writes_assoc_only_when_asked(ga, tmp_path):
    import dataclasses
    import os
    from gnomix_amd import assoc, synth, vcfio, cli
    from gnomix_amd import postprocess as pp
    d = synth.synthetic_model(C=3037, M=50, A=4, S=11, n_rounds=4, seed=5)
    X = synth.synthetic_X(60, d.C, seed=3, miss=0.03)
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
    off, on = run("off"), run("on", ancestry_assoc_output=True, phenotype_file=ph)
    assert sorted(os.listdir(str(off))) == ["query_results.fb", "query_results.msp"]                 # the key absent: the files as before
    assert sorted(os.listdir(str(on))) == ["query_results.assoc.tsv", "query_results.fb", "query_results.msp"]
    for f in ("query_results.fb", "query_results.msp"):
        assert (off / f).read_bytes() == (on / f).read_bytes()
    rows = [ln.split("\t") for ln in (on / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)           # the labels that went to the .msp
    y, Z, use, _ = assoc.read_phenotypes(ph, samples)
    assert use.sum() == len(samples) - 2 and Z.shape[1] == 2
    res = g.dev.ancestry_assoc(X, lab, y, Z, use)                                                      # the Python API on the matrix
    pp.write_assoc(str(tmp_path / "want"), "22", d.snp_pos, d.M, d.W, res, pops)
    text = (on / "query_results.assoc.tsv").read_text()
    assert text == (tmp_path / "want.assoc.tsv").read_text() and len(text.splitlines()) == 1 + d.C
    assert (res.status == 0).any() and (res.n <= len(samples) - 2).all()
    with pytest.raises(ValueError, match="ancestry_association"):
        run("phased", phase=True, ancestry_assoc_output=True, phenotype_file=ph)
    assert os.listdir(str(tmp_path / "phased")) == []
    with pytest.raises(ValueError, match="phenotype_file"):
        run("nofile", ancestry_assoc_output=True)
    assert os.listdir(str(tmp_path / "nofile")) == []


def test_cli_main_reads_the_config_keys(ga, tmp_path, monkeypatch):
    import os
    from gnomix_amd import synth, vcfio, cli
    d = synth.synthetic_model(C=2037, M=50, A=3, S=11, n_rounds=4, seed=9)
    d.snp_pos = 1000 + 37 * np.arange(d.C)
    d.snp_ref, d.snp_alt = np.array(["A"] * d.C), np.array(["C"] * d.C)
    d.gen_map_pos, d.gen_map_cm = np.array([1, 400_000]), np.array([0.0, 1.3])
    mp = str(tmp_path / "model.gnx")
    d.save(mp)
    X = synth.synthetic_X(40, d.C, seed=1, miss=0.02)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), 20, d.snp_pos, d.snp_ref, d.snp_alt, chrom="22")
    samples = [str(s) for s in vcfio.read_vcf(q, chm="22", ctx=None)["samples"]]
    ph = _phenotypes(str(tmp_path / "pheno.tsv"), samples)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("GNX_DEVICES", "0")
    (tmp_path / "config.yaml").write_text("inference:\n  ancestry_assoc_output: True\n  phenotype_file: %s\n" % ph)
    out = tmp_path / "out"
    assert cli.main(["gnomix.py", q, str(out), "22", "False", mp]) == 0
    lines = (out / "query_results.assoc.tsv").read_text().splitlines()
    assert len(lines) == 1 + d.C and lines[0].split("\t")[:7] == ["chm", "pos", "window", "n", "df", "status", "n_miss"]
    assert len(lines[0].split("\t")) == 7 + 6 * d.A
    with pytest.raises(ValueError, match="ancestry_association"):
        cli.main(["gnomix.py", q, str(tmp_path / "phased"), "22", "True", mp])
    assert os.listdir(str(tmp_path / "phased")) == []
    (tmp_path / "config.yaml").write_text("inference:\n  bed_file_output: False\n")
    assert cli.main(["gnomix.py", q, str(tmp_path / "off"), "22", "False", mp]) == 0
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["query_results.fb", "query_results.msp"]
