"""gnx_ancestry_admixmap[_dev] (csrc/summary/k_ancestry_assoc_admix.hip: [Z, H]^T Y per window on v_mfma_f64_16x16x4_f64, from the labels
alone) and admixture mapping built on it, on the MI355X, against the restatement (tests/admixmap_exact.py).

Shapes: tests/admixmap_cases.py.  Every call puts poison behind the rows: a label stride of W + 3 with labels out of range in the gap, a
stride of Y of T + 2 with NaN in the gap.
BLOCKS: the integers exact; |got - exact| <= gamma_n sum_i |term_i| with gamma_n = n 2^-53 / (1 - n 2^-53), n the participants of the window,
the exact sum in rational arithmetic: the bound of ANY summation order of n terms, so it needs no measurement (the largest excess is
printed; measured on the MI355X: 0.86 at n_ind = 3, T = 17, A = 12, K = 5).  RESULTS (measured: ratio 94.3 of C_TOL = 400 at A = 2, K = 1; F at
1.4e-3 r_ref): assoc_cases' bound, C_TOL p kappa^2 2^-53 max|beta|, and 64 r_ref for F (tests/test_admixmap_host.py)."""
import ctypes

import numpy as np
import pytest

import admixmap_cases as MC
import admixmap_exact as XE
import assoc_cases as AC
import test_admixmap_host as TH

pytestmark = pytest.mark.gpu

FILL = -7.0
_got, _exact = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _call(ctx, lab, A, Y, Z, use, w0, w1, dev, gap=True):
    """-> rc, (win_i, win_g, win_y, win_yy) with the padded trait axis (poisoned before the call), n_bad, message"""
    from gnomix_amd import admixmap
    N, W = lab.shape
    K, T = Z.shape[1], Y.shape[1]
    out = admixmap.stats_buffers(A, K, T, w0, w1, empty=lambda shape, dt: np.full(shape, FILL, dt))
    n_bad = ctypes.c_int64(-1)
    ldl, ldy = (W + 3, T + 2) if gap else (W, T)
    Yw = np.full((Y.shape[0], ldy), np.nan)
    Yw[:, :T] = Y
    wide = np.full((N, ldl), A, np.int32)
    wide[:, :W] = lab
    Z, use = np.ascontiguousarray(Z), np.ascontiguousarray(use)
    if not dev:
        rc = ctx.lib.gnx_ancestry_admixmap(ctx.h, wide.ctypes.data, ldl, N, W, A, Yw.ctypes.data, ldy, T, Z.ctypes.data, K, use.ctypes.data, w0, w1,
                                           *(o.ctypes.data for o in out), ctypes.byref(n_bad))
    else:
        import torch
        t = [torch.from_numpy(v).cuda() for v in (wide, Yw, Z, use)]
        o = [torch.from_numpy(v).cuda() for v in out]
        rc = ctx.lib.gnx_ancestry_admixmap_dev(ctx.h, t[0].data_ptr(), ldl, N, W, A, t[1].data_ptr(), ldy, T, t[2].data_ptr(), K, t[3].data_ptr(), w0, w1,
                                               *(v.data_ptr() for v in o), ctypes.byref(n_bad))
        out = tuple(v.cpu().numpy() for v in o)
    return rc, out, n_bad.value, ctx.lib.gnx_last_error(ctx.h).decode()


def _blocks(ctx, key, dev):
    if (key, dev) not in _got:
        lab, Y, Z, use = MC.case(*key)
        _got[(key, dev)] = _call(ctx, lab, key[3], Y, Z, use, 0, lab.shape[1], dev)
    return _got[(key, dev)]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _bound_excess(got, exact, sumabs, n):
    """the largest |got - exact| / (gamma_n sum |term|); an entry whose terms are all zero must be exactly 0.0"""
    worst = 0.0
    for g, e, s, m in zip(got.reshape(len(n), -1), exact.reshape(len(n), -1), sumabs.reshape(len(n), -1), n):
        gam = m * 2.0 ** -53 / (1 - m * 2.0 ** -53)
        for gv, ev, sv in zip(g, e, s):
            if sv == 0:
                assert gv == 0.0
            else:
                worst = max(worst, float(abs(XE.Fraction(float(gv)) - ev) / sv) / gam)
    return worst


@pytest.mark.parametrize("key", MC.GRID + [MC.FIT[3]])
def test_blocks(ctx, key):
    """both entries: integers exact, floats inside the summation bound, zeros exact, padded columns zero, everything finite, n_bad and its
    message, host == _dev and a second run == the first, bit for bit"""
    from gnomix_amd import _lib
    lab, Y, Z, use = MC.case(*key)
    T, A, K = key[1], key[3], key[4]
    if key not in _exact:
        _exact[key] = XE.blocks(lab, A, Y, Z, use, 0, lab.shape[1])
    ex = _exact[key]
    rc, out, n_bad, msg = _blocks(ctx, key, False)
    assert rc == _lib.GNX_EINVAL and n_bad == ex["n_bad"] > 0
    assert msg == "ancestry_admixmap: %d labels lie outside [0, %d); an individual with such a label takes no part at that window" % (n_bad, A)
    wi, wg, wy, wyy = out
    assert np.array_equal(wi, ex["win_i"])
    assert all(np.isfinite(v).all() for v in (wg, wy, wyy))
    assert np.array_equal(wy[:, :, T:], np.zeros_like(wy[:, :, T:])) and np.array_equal(wyy[:, T:], np.zeros_like(wyy[:, T:]))
    n = ex["win_i"][:, 0]
    excess = max(_bound_excess(wg, ex["g"], ex["g_abs"], n), _bound_excess(wy[:, :, :T], ex["y"], ex["y_abs"], n),
                 _bound_excess(wyy[:, :T], ex["yy"], ex["yy_abs"], n))
    print("largest excess", key, excess)
    assert excess <= 1.0
    rc2, out2, n_bad2, _ = _blocks(ctx, key, True)
    assert (rc2, n_bad2) == (rc, n_bad) and _same(out, out2)
    rc3, out3, _, _ = _call(ctx, lab, A, Y, Z, use, 0, lab.shape[1], False)
    assert rc3 == rc and _same(out, out3)


def test_sub_range_and_stride_independence(ctx):
    key = (9, 17, 19, 13, 4)
    lab, Y, Z, use = MC.case(*key)
    _, whole, _, _ = _blocks(ctx, key, False)
    for dev in (False, True):
        _, part, _, _ = _call(ctx, lab, key[3], Y, Z, use, 3, 18, dev)
        assert _same([v[3:18] for v in whole], part)
    _, plain, _, _ = _call(ctx, lab, key[3], Y, Z, use, 0, 19, True, gap=False)
    assert _same(whole, plain)


def test_independent_of_trait_tiles(ctx):
    """T = 17 (two trait tiles per workgroup) against T = 16 (one) on the same columns, the participation unchanged"""
    key = (9, 17, 19, 7, 3)
    lab, Y, Z, use = MC.case(*key)
    Y = Y.copy()
    Y[~np.isfinite(Y).all(1)] = 1.5           # complete rows: dropping column 16 changes nobody's participation
    _, a, _, _ = _call(ctx, lab, key[3], Y, Z, use, 0, 19, True)
    _, b, _, _ = _call(ctx, lab, key[3], np.ascontiguousarray(Y[:, :16]), Z, use, 0, 19, True)
    assert _same(a[:2], b[:2]) and a[2][:, :, :16].tobytes() == b[2].tobytes() and a[3][:, :16].tobytes() == b[3].tobytes()


def test_four_trait_tiles_against_one(ctx):
    """T = 64 (four trait tiles per workgroup, k_ancestry_assoc_admix_main<1, 4>) columns 0 .. 15 against a T = 16 call on those columns"""
    key = (9, 64, 19, 7, 3)
    lab, Y, Z, use = MC.case(*key)
    Y = Y.copy()
    Y[~np.isfinite(Y).all(1)] = -0.75
    _, a, _, _ = _call(ctx, lab, key[3], Y, Z, use, 0, 19, True)
    _, b, _, _ = _call(ctx, lab, key[3], np.ascontiguousarray(Y[:, :16]), Z, use, 0, 19, False)
    assert _same(a[:2], b[:2]) and a[2][:, :, :16].tobytes() == b[2].tobytes() and a[3][:, :16].tobytes() == b[3].tobytes()
    _, c, _, _ = _call(ctx, lab, key[3], np.ascontiguousarray(Y[:, 48:]), Z, use, 0, 19, True)
    assert a[2][:, :, 48:].tobytes() == c[2].tobytes() and a[3][:, 48:].tobytes() == c[3].tobytes()


def test_refusals_write_nothing(ctx):
    from gnomix_amd import _lib
    lab, Y, Z, use = MC.case(9, 16, 19, 7, 3)
    big = lambda K: np.ones((9, K))

    def refused(code, lab=lab, A=7, Y=Y, Z=Z, w0=0, w1=19):
        rc, out, _, _ = _call(ctx, lab, A, Y, Z, use[:lab.shape[0] // 2], w0, w1, True)
        assert rc == code and all((v == FILL).all() for v in out)

    refused(_lib.GNX_EUNSUPPORTED, A=_lib.GNX_ALLELE_MAX_A + 1)
    refused(_lib.GNX_EUNSUPPORTED, Z=big(17))
    refused(_lib.GNX_EUNSUPPORTED, lab=lab[:-1])
    refused(_lib.GNX_EINVAL, w0=5, w1=5)
    refused(_lib.GNX_EINVAL, w0=-1)
    n_bad = ctypes.c_int64(-1)
    out = np.full(64, FILL)
    p = out.ctypes.data
    for args, code in ((dict(T=65537, ldy=65537), _lib.GNX_EUNSUPPORTED), (dict(N=(1 << 28) + 2), _lib.GNX_EUNSUPPORTED), (dict(ldy=15), _lib.GNX_EINVAL),
                       (dict(ldl=18), _lib.GNX_EINVAL), (dict(w1=20), _lib.GNX_EINVAL)):
        a = dict(N=18, T=16, ldy=16, ldl=19, w1=19)
        a.update(args)
        rc = ctx.lib.gnx_ancestry_admixmap(ctx.h, lab.ctypes.data, a["ldl"], a["N"], 19, 7, Y.ctypes.data, a["ldy"], a["T"], Z.ctypes.data, 3, None, 0, a["w1"],
                                           p, p, p, p, ctypes.byref(n_bad))
        assert rc == code and (out == FILL).all(), args


@pytest.mark.parametrize("key", MC.FIT + [MC.FIT_RAW])
def test_results_end_to_end(ctx, key):
    from gnomix_amd import admixmap
    lab, Y, Z, use = MC.case(*key)
    want = MC.check_fit_case(key)
    res = admixmap.admixture_mapping(ctx, lab, key[3], Y, Z, use, MC.MIN_HAP, check=False)
    TH._exact_fields(res, want)
    ratio, fr, r_ref = TH.result_ratio(res, want), TH.f_ratio(res, want), _r_ref()
    print("results", key, "ratio", ratio, "F", fr, "r_ref", r_ref)
    assert ratio <= AC.C_TOL and fr <= 64 * r_ref
    import torch
    res_t = admixmap.admixture_mapping(ctx, torch.from_numpy(lab).cuda(), key[3], Y, Z, use, MC.MIN_HAP, check=False)
    assert all(np.array_equal(getattr(res, f), getattr(res_t, f), equal_nan=True) for f in ("beta", "se", "t", "p", "F", "p_joint", "n_hap"))
    with pytest.raises(Exception, match="labels lie outside"):
        admixmap.admixture_mapping(ctx, lab, key[3], Y, Z, use, MC.MIN_HAP)


def _r_ref():
    if "r_ref" not in _exact:
        _exact["r_ref"] = TH.f_reference_error()
    return _exact["r_ref"]


def test_permutations(ctx):
    from gnomix_amd import admixmap
    want, mt, mF = MC.perm_reference()
    lab, Y, Z, use = MC.case(*MC.PERM)
    A = MC.PERM[3]
    res = admixmap.admixture_mapping(ctx, lab, A, Y, Z, use, MC.MIN_HAP, MC.N_PERM, MC.SEED, check=False)
    # perm_max_t is the |t| of one fitted cell: the results' bound of that cell (p kappa^2 2^-53 max|beta| of its window and column)
    scale = XE.permutation_maxima(lab, A, Y, Z, use, MC.MIN_HAP, MC.N_PERM, MC.SEED, want_scale=True)[2]
    print("perm_max_t", np.max(np.abs(res.perm_max_t - mt) / scale), "of", AC.C_TOL, "perm_max_F", np.max(np.abs(res.perm_max_F - mF) / mF))
    assert np.all(np.abs(res.perm_max_t - mt) <= AC.C_TOL * scale) and np.all(np.abs(res.perm_max_F - mF) <= 64 * _r_ref() * mF)
    assert np.array_equal(res.p_adj_t, XE.adjusted(np.abs(want["t"]), mt), equal_nan=True)
    assert np.array_equal(res.p_adj_F, XE.adjusted(want["F"], mF), equal_nan=True)


def test_chunked_columns_bit_equal(ctx):
    """two column chunks (16 + 16 of 32 permuted columns) against one call"""
    from gnomix_amd import admixmap
    lab, Y, Z, use = MC.case(*MC.PERM)
    A = MC.PERM[3]
    W = lab.shape[1]
    one_chunk = admixmap.columns_per_chunk(W, A, 3, 1 << 40)
    small = W * ((3 + A + 1) * 8 + (3 * A + 1) * 8) * 16
    assert admixmap.columns_per_chunk(W, A, 3, small) == 16 and one_chunk > 32
    a = admixmap.admixture_mapping(ctx, lab, A, Y, Z, use, MC.MIN_HAP, 16, MC.SEED, check=False)
    b = admixmap.admixture_mapping(ctx, lab, A, Y, Z, use, MC.MIN_HAP, 16, MC.SEED, check=False, chunk_bytes=small)
    assert all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in a._fields)


def test_model_level(ctx):
    """HipGnomix.admixture_mapping equals admixmap.admixture_mapping on predict's labels; labels= is honoured; CUDA-tensor labels give the
    same bits as host labels"""
    import torch
    import gnomix_amd
    from gnomix_amd import admixmap, synth
    data = synth.synthetic_model(C=6037, M=100, A=7, S=21, n_rounds=12, seed=3)
    X = synth.synthetic_X(40, data.C, seed=2)
    g = gnomix_amd.HipGnomix(data, device=0)
    rng = np.random.RandomState(3)
    y = rng.normal(size=20)
    Z = np.concatenate([np.ones((20, 1)), rng.normal(size=(20, 1))], 1)
    lab = g.predict(X)
    want = admixmap.admixture_mapping(g.dev.ctx, lab, data.A, y, Z)
    got = g.admixture_mapping(X, y, Z)
    assert got.beta.shape == (data.W, data.A, 1)
    same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in ("beta", "se", "t", "p", "F", "p_joint", "n_hap", "status"))
    assert same(got, want)
    other = np.ascontiguousarray(lab[::-1])
    assert same(g.admixture_mapping(None, y, Z, labels=other), admixmap.admixture_mapping(g.dev.ctx, other, data.A, y, Z))
    assert same(g.admixture_mapping(None, y, Z, labels=torch.from_numpy(other).cuda()), g.admixture_mapping(None, y, Z, labels=other))
    assert same(g.admixture_mapping(torch.from_numpy(X).cuda(), y, Z), want)


def test_command_line(tmp_path):
    """inference.admixture_mapping_output with phase False and phase True on the suite's small query: the file parses and equals the Python
    API's result on the labels the .msp holds; a trait file gives one file per trait; a missing file is refused before any work"""
    import dataclasses
    import os
    import gnomix_amd
    from gnomix_amd import admixmap, assoc, cli, synth, vcfio
    from gnomix_amd import postprocess as pp
    d = synth.synthetic_model(C=3037, M=50, A=4, S=11, n_rounds=4, seed=5)
    X = synth.synthetic_X(60, d.C, seed=3, miss=0.03)
    pops = ["P%d" % a for a in range(d.A)]
    d = dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                            population_order=pops, gen_map_pos=np.array([1, 50_000, 200_000]), gen_map_cm=np.array([0.0, 1.5, 9.25]))
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    g = gnomix_amd.HipGnomix(d, device=0)
    samples = [str(s) for s in vcfio.read_vcf(q, chm="22", ctx=g.dev.ctx)["samples"]]
    rng = np.random.RandomState(8)
    ph, tr = ["sample\tpheno\tage"], ["sample\theight\tbmi"]
    for i, s in enumerate(samples):
        if i != 1:                                                       # the second sample is unknown to both files
            ph.append("%s\t%s\t%.3f" % (s, "NA" if i == 4 else "%.5f" % rng.normal(), rng.uniform(20, 70)))
            tr.append("%s\t%.5f\t%.5f" % (s, rng.normal(), rng.normal()))
    pf, tf = str(tmp_path / "pheno.tsv"), str(tmp_path / "traits.tsv")
    open(pf, "w").write("\n".join(ph) + "\n")
    open(tf, "w").write("\n".join(tr) + "\n")

    def run(name, phase=False, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, **kw)
        return od
    y, Z, use, _ = assoc.read_phenotypes(pf, samples)
    for phase in (False, True):
        od = run("phase%d" % phase, phase=phase, admixture_mapping_output=True, phenotype_file=pf, admixture_mapping_perms=3, admixture_mapping_seed=11,
                 admixture_mapping_min_hap=2)
        assert "query_results.admixmap.tsv" in os.listdir(str(od))
        msp = pp.read_msp(str(od / "query_results.msp"))
        assert msp.samples == samples and msp.populations == pops
        want = admixmap.admixture_mapping(g.dev.ctx, msp.labels, d.A, y, Z, use, 2, 3, 11)
        assert (want.status == 0).any() and want.perm_max_t.shape == (1, 3)
        pp.write_admixmap(str(tmp_path / ("want%d" % phase)), msp.meta, want, pops)
        text = (od / "query_results.admixmap.tsv").read_text()
        assert text == (tmp_path / ("want%d.admixmap.tsv" % phase)).read_text()
        rows = [ln.split("\t") for ln in text.splitlines()]
        assert len(rows) == 1 + d.W and all(len(r) == len(rows[0]) for r in rows) and rows[0][-1] == "P3.p_adj"
        assert [int(r[6]) for r in rows[1:]] == list(want.n) and float(rows[1][10]) == float(format(want.F[0, 0], ".6g"))
    assert (tmp_path / "phase0" / "query_results.msp").read_bytes() != (tmp_path / "phase1" / "query_results.msp").read_bytes()
    od = run("traits", admixture_mapping_output=True, trait_file=tf)
    assert sorted(os.listdir(str(od))) == ["query_results.admixmap.bmi.tsv", "query_results.admixmap.height.tsv", "query_results.fb", "query_results.msp"]
    assert "p_adj" not in (od / "query_results.admixmap.bmi.tsv").read_text().splitlines()[0]
    assert sorted(os.listdir(str(run("off", phenotype_file=pf)))) == ["query_results.fb", "query_results.msp"]
    with pytest.raises(ValueError, match="no such file"):
        run("absent", admixture_mapping_output=True, phenotype_file=str(tmp_path / "absent.tsv"))
    assert os.listdir(str(tmp_path / "absent")) == []
