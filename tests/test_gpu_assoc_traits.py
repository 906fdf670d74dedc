"""gnx_ancestry_assoc_traits[_dev / _gt2] (csrc/summary/k_ancestry_assoc_traits.hip: D^T Y on v_mfma_f64_16x16x4_f64) and the
many-trait association built on it, on the MI355X, against the numpy restatement (tests/assoc_traits_exact.py).

Shapes: tests/assoc_traits_cases.py (n_ind in {5, 8, 9}, T in {1, 15, 16, 17, 33}, C = 37 with M = 8, A in {2, 3, 7, 9}, K in {1, 3}; every
case has missing calls, labels out of range, use zeros, NaN and +-inf in Y, a monomorphic SNP, a dosage column below min_ac, a window
with df < 1 and a window without ancestry A - 1).  int8 rows go through the host entry, 2-bit rows through the device entry.

TRAIT BLOCKS: |got - exact| <= gamma_n sum_i |term_i| with gamma_n = n 2^-53 / (1 - n 2^-53), n the participants of the window, the exact
sum in rational arithmetic: the bound of ANY summation order of n terms (n - 1 additions and at most one rounded product), so it needs no
measurement.  Measured on the MI355X: the largest excess |got - exact| / (gamma_n sum |term|) over the grid is 0.96 (n_ind = 9, T = 33, A = 7).
RESULTS: tests/assoc_cases.py's bound, C_TOL p kappa^2 2^-53 max|beta| per SNP and trait."""
import ctypes
import os

import numpy as np
import pytest

import allele_counts_exact as AE
import assoc_cases as AC
import assoc_traits_cases as TC
import assoc_traits_exact as TE

pytestmark = pytest.mark.gpu

_got = {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _codes(X):
    return np.where((X == 0) | (X == 1), X, np.where(X == -1, 3, 2)).astype(np.uint8)


def _call(ctx, X, lab, M, A, Y, Z, use, c0, c1, packed, min_ac=TC.MIN_AC, fill=-7.0):
    """-> rc, (snp_y, win_y, win_yy) with the padded trait axis, n_bad.  Poison behind every row, a label stride larger than W, a stride
    of Y larger than T.  packed 0: int8 rows through the host entry; 1: 2-bit rows through the device entry"""
    from gnomix_amd import assoc
    N, C = X.shape
    W, K, T = lab.shape[1], Z.shape[1], Y.shape[1]
    out = assoc.trait_buffers(A, K, T, c0, c1, M, W, empty=lambda shape, dt: np.full(shape, fill, dt))
    n_bad = ctypes.c_int64(-1)
    Yw = np.full((Y.shape[0], T + 2), np.nan)
    Yw[:, :T] = Y
    Z, use = np.ascontiguousarray(Z), np.ascontiguousarray(use)
    wide = np.full((N, W + 3), A, np.int32)
    wide[:, :W] = lab
    if not packed:
        rows = np.full((N, C + 5), 1, np.int8)
        rows[:, :C] = X
        rc = ctx.lib.gnx_ancestry_assoc_traits(ctx.h, rows.ctypes.data, C + 5, wide.ctypes.data, W + 3, N, C, M, W, A, Yw.ctypes.data, T + 2, T,
                                               Z.ctypes.data, K, use.ctypes.data, min_ac, c0, c1, out[0].ctypes.data, out[1].ctypes.data,
                                               out[2].ctypes.data, ctypes.byref(n_bad))
        return rc, out, n_bad.value
    import torch
    rows = torch.from_numpy(AE.pack2(_codes(X), ldp=(C + 3) // 4 + 3, fill=0x55)).cuda()
    t = [torch.from_numpy(v).cuda() for v in (wide, Yw, Z, use)]
    o = [torch.from_numpy(v).cuda() for v in out]
    rc = ctx.lib.gnx_ancestry_assoc_traits_dev(ctx.h, rows.data_ptr(), 1, rows.stride(0), t[0].data_ptr(), W + 3, N, C, M, W, A, t[1].data_ptr(), T + 2, T,
                                               t[2].data_ptr(), K, t[3].data_ptr(), min_ac, c0, c1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                               ctypes.byref(n_bad))
    return rc, tuple(v.cpu().numpy() for v in o), n_bad.value


def _same(a, b, where=""):
    for u, v, name in zip(a, b, ("snp_y", "win_y", "win_yy")):
        assert u.shape == v.shape and np.array_equal(u, v), (name, where)


@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("n_ind,T,A,K", TC.GRID)
def test_trait_blocks_against_exact_sums(ctx, n_ind, T, A, K, packed):
    from gnomix_amd import _lib
    X, lab, Y, Z, use = TC.small_case(n_ind, T, A, K)
    assert (_codes(X) == 3).any() and (_codes(X) == 2).any()
    rc, got, n_bad = _call(ctx, X, lab, TC.M, A, Y, Z, use, 0, TC.C, packed)
    assert rc == _lib.GNX_EINVAL and n_bad == n_ind - 1, ctx.lib.gnx_last_error(ctx.h)
    assert (b"%d labels lie outside [0, %d)" % (n_ind - 1, A)) in ctx.lib.gnx_last_error(ctx.h)
    for g in got:
        assert np.isfinite(g).all() and (g[..., T:] == 0).all()             # every value written, the padded columns as zeros
    key = (n_ind, T, A, K)
    if key not in _got:                                                      # the exact sums are taken once per shape
        excess, zeros_ok = TE.worst_excess(tuple(g[..., :T] for g in got), X, lab, TC.M, A, Y, Z, use, 0, TC.C)
        print("n_ind %d T %d A %d K %d: largest |got - exact| / (gamma_n sum |term|) = %.4g" % (n_ind, T, A, K, excess))
        assert zeros_ok, "an entry whose terms are all zero must be exactly 0.0"
        assert excess <= 1.0
        _got[key] = got
    else:
        _same(got, _got[key], "int8 rows against 2-bit rows")
    # two runs of the same call
    rc, again, _ = _call(ctx, X, lab, TC.M, A, Y, Z, use, 0, TC.C, packed)
    _same(again, got, "run to run")
    # a sub-range with both ends unaligned that crosses the window boundaries 8, 16 and 24: the slice of the whole range, bit for bit
    c0, c1 = 5, 29
    rc, part, n_bad = _call(ctx, X, lab, TC.M, A, Y, Z, use, c0, c1, packed)
    assert rc == _lib.GNX_EINVAL and n_bad == n_ind - 1
    _same(part, (got[0][c0:c1], got[1][0:4], got[2][0:4]), "range")
    rc, part, n_bad = _call(ctx, X, lab, TC.M, A, Y, Z, use, 17, 36, packed)       # windows 2 and 3 only: no label out of range there
    assert rc == 0 and n_bad == 0
    _same(part, (got[0][17:36], got[1][2:4], got[2][2:4]), "range 2")


def _compare_results(res, want, T):
    for k in range(T):
        w = want[k]
        for name in ("n_alt", "n_hap", "n", "df", "n_miss", "status"):
            assert np.array_equal(getattr(res, name), w[name]), (name, k)
        for name in ("beta", "se", "t"):
            assert np.array_equal(np.isnan(getattr(res, name)[:, :, k]), np.isnan(w[name])), (name, k)
        ok = (w["status"] == 0) & (w["kappa"] <= AC.KAPPA_MAX) & ~np.isnan(w["beta"]).all(1)      # (a fitted SNP may have no dosage term kept)
        if ok.any():
            scale = AC.C_TOL * w["p_kept"][ok] * w["kappa"][ok] ** 2 * 2.0 ** -53 * np.nanmax(np.abs(w["beta"][ok]), axis=1)
            for name in ("beta", "se", "t"):
                err = np.nanmax(np.abs(getattr(res, name)[ok][:, :, k] - w[name][ok]), axis=1)
                assert (err <= scale).all(), (name, k, float(np.max(err / scale)) * AC.C_TOL)
    assert np.array_equal(np.isnan(res.p), np.isnan(res.t))


@pytest.mark.parametrize("n_ind,T,A,K", TC.GRID)
def test_results_against_lstsq_per_trait(ctx, n_ind, T, A, K):
    from gnomix_amd import assoc
    X, lab, Y, Z, use = TC.small_case(n_ind, T, A, K)
    want = TE.fit(X, lab, TC.M, A, Y, Z, use, min_ac=TC.MIN_AC)
    _, _, _, use2 = assoc.trait_covariates(n_ind, Y, Z, use)

    def blocks(c0, c1):
        return (assoc.stats_host(ctx, X, lab, TC.M, A, np.zeros(n_ind), Z, use2, c0, c1, min_ac=TC.MIN_AC, check=False),
                assoc.traits_host(ctx, X, lab, TC.M, A, Y, Z, use, c0, c1, min_ac=TC.MIN_AC, check=False))
    res = assoc.traits_concat(assoc.traits_chunks(blocks, TC.C, A, K, T, TC.MIN_AC), TC.C, A, T)
    assert res.beta.shape == (TC.C, A, T) and res.status.shape == (TC.C,)
    _compare_results(res, want, T)
    assert (res.status[8:16] == 2).all() and ((res.status[16:24] == 1) | (res.df[16:24] < 1)).all()
    assert np.isnan(res.beta[5]).all() and np.isnan(res.beta[6]).all()


@pytest.mark.parametrize("A", [2, 7])
def test_regression_results_on_well_conditioned_designs(ctx, A):
    """257 individuals, 130 SNPs, three traits (tests/assoc_traits_cases.py): every SNP is fitted, so the bound is exercised everywhere"""
    from gnomix_amd import assoc
    X, lab, Y, Z, use = TC.regression_traits(A)
    want = TE.fit(X, lab, AC.M, A, Y, Z, use)
    _, _, _, use2 = assoc.trait_covariates(AC.N_IND, Y, Z, use)
    blocks = lambda c0, c1: (assoc.stats_host(ctx, X, lab, AC.M, A, np.zeros(AC.N_IND), Z, use2, c0, c1),
                             assoc.traits_host(ctx, X, lab, AC.M, A, Y, Z, use, c0, c1))
    res = assoc.traits_concat(assoc.traits_chunks(blocks, AC.C, A, AC.K, 3), AC.C, A, 3)
    assert (res.status == 0).all()
    _compare_results(res, want, 3)


def test_refusals_leave_the_outputs_untouched(ctx):
    from gnomix_amd import _lib, assoc
    N, C, M, W, A, K, T = 4, 20, 5, 4, 3, 2, 3
    X, lab = np.zeros((N, C), np.int8), np.zeros((N, W), np.int32)
    Y, Z, use = np.zeros((N // 2, T)), np.ones((N // 2, 17)), np.ones(N // 2, np.uint8)
    out = tuple(np.full((C * 33 * 16,), -7.0) for _ in range(3))
    n_bad = ctypes.c_int64(-7)
    lib, h = ctx.lib, ctx.h

    def call(X=X, N=N, M=M, A=A, K=K, T=T, ldy=T, min_ac=1, c0=0, c1=C, ld=C, Y=Y, Z=Z, o0=out[0]):
        p = lambda v: None if v is None else v.ctypes.data
        return lib.gnx_ancestry_assoc_traits(h, p(X), ld, lab.ctypes.data, W, N, C, M, W, A, p(Y), ldy, T, p(Z), K, use.ctypes.data, min_ac, c0, c1,
                                             p(o0), out[1].ctypes.data, out[2].ctypes.data, ctypes.byref(n_bad))
    assert call(N=3) == _lib.GNX_EINVAL and call(K=0) == _lib.GNX_EINVAL and call(M=6) == _lib.GNX_EINVAL and call(min_ac=0) == _lib.GNX_EINVAL
    assert call(T=0) == _lib.GNX_EINVAL and call(ldy=T - 1) == _lib.GNX_EINVAL
    assert call(X=None) == _lib.GNX_EINVAL and call(Y=None) == _lib.GNX_EINVAL and call(Z=None) == _lib.GNX_EINVAL and call(o0=None) == _lib.GNX_EINVAL
    assert call(c0=5, c1=5) == _lib.GNX_EINVAL and call(c1=C + 1) == _lib.GNX_EINVAL and call(ld=C - 1) == _lib.GNX_EINVAL
    assert call(A=33) == _lib.GNX_EUNSUPPORTED and b"33" in lib.gnx_last_error(h)
    assert call(K=17) == _lib.GNX_EUNSUPPORTED and b"17" in lib.gnx_last_error(h)
    assert call(T=assoc.MAX_T + 1, ldy=assoc.MAX_T + 1) == _lib.GNX_EUNSUPPORTED and b"65537" in lib.gnx_last_error(h)
    assert all((v == -7).all() for v in out) and n_bad.value == -7
    assert call() == 0 and n_bad.value == 0


def _model_inputs(n_hap=120, T=17, seed=1):
    from gnomix_amd import synth
    d = synth.synthetic_model(C=3037, M=50, A=4, S=11, n_rounds=4, seed=5)
    X = synth.synthetic_X(n_hap, d.C, seed=3, miss=0.03)
    rng = np.random.RandomState(seed)
    n_ind = n_hap // 2
    Y = rng.normal(size=(n_ind, T))
    Y[7, 3] = np.nan
    Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, 2))], 1)
    use = np.ones(n_ind, np.uint8)
    use[5] = 0
    return d, X, Y, Z, use


def test_model_surface_chunks_and_device_tensors(ga):
    import torch
    from gnomix_amd import assoc
    d, X, Y, Z, use = _model_inputs()
    T = Y.shape[1]
    g = ga.HipGnomix(d, device=0)
    dev = g.dev
    lab = np.ascontiguousarray(g.predict(X), dtype=np.int32)
    res = g.ancestry_association(X, Y, Z, use)
    assert type(res).__name__ == "AncestryAssocTraits" and res.beta.shape == (d.C, d.A, T) and res.n.shape == (d.C,) and res.n.dtype == np.int32
    assert (res.n <= X.shape[0] // 2 - 2).all()
    cols = set(range(0, d.C, 211))
    want = TE.fit(X, lab, d.M, d.A, Y[:, [0, 3, T - 1]], Z, use & np.isfinite(Y).all(1), cols=cols)
    for k, t in enumerate((0, 3, T - 1)):
        w = want[k]
        for name in ("n_alt", "n_hap", "n", "df", "n_miss"):
            assert np.array_equal(getattr(res, name), w[name]), name
        solved = w["status"] >= 0
        assert np.array_equal(res.status[solved], w["status"][solved])
        ok = (w["status"] == 0) & (w["kappa"] <= AC.KAPPA_MAX)
        assert ok.sum() >= 1
        scale = (AC.C_TOL * w["p_kept"][ok] * w["kappa"][ok] ** 2 * 2.0 ** -53 * np.nanmax(np.abs(w["beta"][ok]), axis=1))[:, None]
        for name in ("beta", "se", "t"):
            gv, wv = getattr(res, name)[ok][:, :, t], w[name][ok]
            assert np.array_equal(np.isnan(gv), np.isnan(wv)) and (np.abs(gv - wv)[~np.isnan(wv)] <= np.broadcast_to(scale, wv.shape)[~np.isnan(wv)]).all()
    # T = 1 through the 2-D path: the same model as the single-trait entry, within the project's bound of each other (not bit for bit)
    one = g.ancestry_association(X, np.where(np.isfinite(Y[:, 3]), Y[:, 3], np.nan), Z, use)
    many = g.ancestry_association(X, Y[:, 3:4], Z, use)
    for name in ("n_alt", "n_hap", "n", "df", "n_miss", "status"):
        assert np.array_equal(getattr(one, name), getattr(many, name)), name
    sel = (want[1]["status"] == 0) & (want[1]["kappa"] <= AC.KAPPA_MAX)
    assert np.nanmax(np.abs(one.beta[sel] - many.beta[sel][:, :, 0])) <= 1e-8 * np.nanmax(np.abs(one.beta[sel]))
    with pytest.raises(NotImplementedError):
        g.ancestry_association(X, Y, Z, use, model="logistic")
    # host arrays against CUDA tensors (int8 and 2-bit rows), bit for bit
    Xt, labt = torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda()
    host = dev.ancestry_assoc_traits_stats(X, lab, Y, Z, use, 100, 2101)
    for rows_t in (Xt, dev.pack_device(Xt)):
        st = dev.ancestry_assoc_traits_stats(rows_t, labt, Y, Z, use, 100, 2101)
        for a, b in zip(host[:4], st[:4]):
            assert np.array_equal(a, b)
    res_t = g.ancestry_association(Xt, Y, Z, use)
    for a, b in zip(res, res_t):
        assert np.array_equal(a, b, equal_nan=True)
    # chunked against unchunked
    per = max(assoc.layout(d.A, 3)[0] * 8 + assoc.layout(d.A, 3)[1] * 4 + d.A * 32 * 8, 4 * d.A * T * 8)
    chunks = list(dev.ancestry_assoc_traits_chunks(X, lab, Y, Z, use, chunk_bytes=per * 1100))
    assert len(chunks) == 3 and [c[0] for c in chunks] == [0, 1100, 2200] and chunks[-1][1] == d.C
    for f in res._fields:
        assert np.array_equal(np.concatenate([getattr(c[2], f) for c in chunks]), getattr(res, f), equal_nan=True), f
    hits = dev.ancestry_assoc_traits(X, lab, Y, Z, use, p_max=0.01)
    keep = res.p <= 0.01
    assert keep.any() and np.array_equal(np.isnan(hits.p), ~keep) and np.array_equal(hits.beta[keep], res.beta[keep])
    with pytest.raises(ValueError, match=str(assoc.traits_result_bytes(d.C, d.A, T))):
        dev.ancestry_assoc_traits(X, lab, Y, Z, use, max_bytes=1 << 20)
    with pytest.raises(ValueError):
        dev.ancestry_assoc_traits(X, lab, Y, Z, use, min_ac=0)
    dev.ctx.reset_stream()


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
    Y, Z = rng.normal(size=(17, 17)), np.concatenate([np.ones((17, 1)), rng.normal(size=(17, 2))], 1)
    Y[9, 16] = np.inf
    use = np.ones(17, np.uint8)
    use[6] = 0
    want = dev.ancestry_assoc_traits_stats(Xq, lab, Y, Z, use, 50, 4000)
    got = dev.ancestry_assoc_traits_stats_gt2(vcf.gt2, 34, src, lab, Y, Z, use, 50, 4000)
    for a, b in zip(want[:4], got[:4]):
        assert np.array_equal(a, b)
    # GNX_HOST_BATCH of 5 individuals (odd): the batches are cut at whole groups of 4 individuals all the same, and every MFMA sees the
    # four individuals a single launch gives it
    monkeypatch.setenv("GNX_HOST_BATCH", "10")
    ctx2 = _lib.Context(0)
    dev2 = ga.DeviceModel(d, ctx=ctx2)
    got = dev2.ancestry_assoc_traits_stats_gt2(np.array(vcf.gt2), 34, src, lab, Y, Z, use, 50, 4000)
    for a, b in zip(want[:4], got[:4]):
        assert np.array_equal(a, b)
    whole = dev.ancestry_assoc_traits(Xq, lab, Y, Z, use)
    filed = dev2.ancestry_assoc_traits_gt2(np.array(vcf.gt2), 34, src, lab, Y, Z, use)
    for a, b in zip(whole, filed):
        assert np.array_equal(a, b, equal_nan=True)
    ctx2.close()
    monkeypatch.delenv("GNX_HOST_BATCH")
    bad = lab.copy()
    bad[3, 5] = d.A
    with pytest.raises(_lib.GnxError, match="1 labels lie outside"):
        dev.ancestry_assoc_traits_stats_gt2(vcf.gt2, 34, src, bad, Y, Z, use)
    assert dev.ancestry_assoc_traits_stats_gt2(vcf.gt2, 34, src, bad, Y, Z, use, check=False).n_bad == 1


def test_command_line_writes_one_file_per_trait(ga, tmp_path):
    import dataclasses
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
    rng = np.random.RandomState(8)
    lines, cov = ["sample\theight\tbmi"], ["sample\tage"]
    for i, s in enumerate(samples):
        if i != 1:                                                       # the second sample is unknown to the trait file
            lines.append("%s\t%s\t%.5f" % (s, "NA" if i == 4 else "%.5f" % rng.normal(), rng.normal()))
        cov.append("%s\t%.3f" % (s, rng.uniform(20, 70)))
    tf, cf = str(tmp_path / "traits.tsv"), str(tmp_path / "cov.tsv")
    open(tf, "w").write("\n".join(lines) + "\n")
    open(cf, "w").write("\n".join(cov) + "\n")

    def run(name, phase=False, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, **kw)
        return od
    off, on = run("off", trait_file=tf), run("on", ancestry_assoc_output=True, trait_file=tf, covariate_file=cf)
    assert sorted(os.listdir(str(off))) == ["query_results.fb", "query_results.msp"]
    assert sorted(os.listdir(str(on))) == ["query_results.assoc.bmi.tsv", "query_results.assoc.height.tsv", "query_results.fb", "query_results.msp"]
    rows = [ln.split("\t") for ln in (on / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)
    Y, Z, use, names, _ = assoc.read_traits(tf, samples, cf)
    assert names == ["height", "bmi"] and use.sum() == len(samples) - 1 and Z.shape[1] == 2
    res = g.dev.ancestry_assoc_traits(X, lab, Y, Z, use)
    assert (res.status == 0).any() and (res.n == len(samples) - 2).all()
    for t, name in enumerate(names):
        one = assoc.AncestryAssoc(*(v[:, :, t] for v in res[:4]), *res[4:])
        pp.write_assoc(str(tmp_path / ("want_" + name)), "22", d.snp_pos, d.M, d.W, one, pops)
        text = (on / ("query_results.assoc.%s.tsv" % name)).read_text()
        assert text == (tmp_path / ("want_%s.assoc.tsv" % name)).read_text() and len(text.splitlines()) == 1 + d.C
    with pytest.raises(ValueError, match="ancestry_association"):
        run("phased", phase=True, ancestry_assoc_output=True, trait_file=tf)
    assert os.listdir(str(tmp_path / "phased")) == []
    with pytest.raises(ValueError, match="trait_file"):
        run("logit", ancestry_assoc_output=True, trait_file=tf, ancestry_assoc_model="logistic")
    assert os.listdir(str(tmp_path / "logit")) == []
