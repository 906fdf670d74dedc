"""gnx_ancestry_score[_dev / _gt2] (csrc/summary/k_ancestry_score.hip) and the layers built on it, on the MI355X, against the numpy
restatement (tests/score_exact.py): every float64 output bit for bit, every integer exactly.

THE ORDER the restatement and the kernel share: per haplotype and window a partial from +0.0 over the applying SNPs in ascending c;
per (individual, ancestry, score) the partials of the haplotypes that carry the ancestry, ascending window, row 2 i before row 2 i + 1.
The weights (tests/score_cases.py: normal x 2^u, u in [-20, 20]) make another order give other bits.

The kernel's sizes the shapes are chosen by: a workgroup owns 256 haplotypes; a column chunk is 256 columns of int8 rows and 512 of
packed rows; the staged weights of a sub-chunk are at most 32 KiB (256 / 512 columns at A = 7, S = 1; 8 columns at A = 32, S = 16).
Row forms: 'i8h' int8 rows through the host entry with a stride of C + 5 (unaligned: the byte route); 'i8d' int8 rows through the
device entry with a 16-byte aligned stride; 'p2h' / 'p2d' 2-bit rows likewise (stride + 3 bytes / a multiple of 4).  Poison behind
every row, labels with a row stride of W + 3."""
import ctypes
import os

import numpy as np
import pytest

import allele_counts_exact as AE
import score_cases as SC
import score_exact as SE

pytestmark = pytest.mark.gpu

ROW_TILE, CHUNK_I8, CHUNK_P2 = 256, 256, 512
FORMS = ("i8h", "i8d", "p2h", "p2d")
_want = {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _err(ctx):
    return ctx.lib.gnx_last_error(ctx.h).decode()


def _expected(key, X, lab, M, A, w, eff):
    """the restatement of a case, computed once and shared by the row forms"""
    if key not in _want:
        if len(_want) > 8:
            _want.clear()
        _want[key] = SE.scores(X, lab, M, A, w, eff)
    return _want[key]


def _run(ctx, form, X, lab, M, A, w, eff, wpb=0, rpp=0, fill=None, outs=(1, 1, 1, 1)):
    """-> rc, (score, n_effect, n_scored, n_miss), n_bad"""
    N, C = X.shape
    W, S = lab.shape[1], w.shape[2]
    packed = form.startswith("p2")
    if packed:
        ld = (C + 3) // 4 + 3 if form == "p2h" else ((C + 3) // 4 + 3) // 4 * 4 + 4
        rows = AE.pack2(SC.codes(X), ldp=ld, fill=0x55)
    else:
        ld = C + 5 if form == "i8h" else (C + 15) // 16 * 16 + 16
        rows = np.full((N, ld), 1, np.int8)
        rows[:, :C] = X
    wide = np.full((N, W + 3), A, np.int32)
    wide[:, :W] = lab
    w, eff = np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(eff, dtype=np.uint8)
    poison = -7 if fill is None else fill
    out = [np.full((N // 2, A, S), float(poison)), np.full((N // 2, A), poison, np.int32), np.full((N // 2, A), poison, np.int32),
           np.full((N // 2, A), poison, np.int32)]
    n_bad = ctypes.c_int64(-1)
    if form.endswith("h"):
        p = [o.ctypes.data if use else None for o, use in zip(out, outs)]
        rc = ctx.lib.gnx_ancestry_score(ctx.h, rows.ctypes.data, int(packed), ld, wide.ctypes.data, W + 3, N, C, M, W, A, w.ctypes.data, S, eff.ctypes.data,
                                        p[0], p[1], p[2], p[3], wpb, rpp, ctypes.byref(n_bad))
        return rc, out, n_bad.value
    import torch
    t = [torch.from_numpy(v).cuda() for v in (rows, wide, w, eff)]
    o = [torch.from_numpy(v).cuda() for v in out]
    p = [v.data_ptr() if use else None for v, use in zip(o, outs)]
    rc = ctx.lib.gnx_ancestry_score_dev(ctx.h, t[0].data_ptr(), int(packed), ld, t[1].data_ptr(), W + 3, N, C, M, W, A, t[2].data_ptr(), S, t[3].data_ptr(),
                                        p[0], p[1], p[2], p[3], wpb, rpp, ctypes.byref(n_bad))
    torch.cuda.synchronize()
    return rc, [v.cpu().numpy() for v in o], n_bad.value


def _same(got, want, where=""):
    for g, w, name in zip(got, want, ("score", "n_effect", "n_scored", "n_miss")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where)
        assert np.array_equal(g, w), (name, where)


# ---------------------------------------------------------------- the grid of shapes -----------------------------------------------
COLS = [(1, 1, 1), (23, 5, 4), (CHUNK_I8 + 1, 100, 2), (CHUNK_P2 + 1, 100, 5)]        # (C, M, W): the last window of 23 takes 8


@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("A", [1, 2, 3, 7, 32])
def test_grid_equals_the_restatement_bit_for_bit(ctx, A, S):
    for N in (2, 14, ROW_TILE + 2, 2 * ROW_TILE + 2):
        for C, M, W in COLS:
            X, lab, w, eff = SC.case(N, C, M, W, A, S)
            want = _expected((N, C, M, A, S), X, lab, M, A, w, eff)
            assert want[4] == 0
            for form in FORMS:
                rc, got, n_bad = _run(ctx, form, X, lab, M, A, w, eff)
                assert rc == 0 and n_bad == 0, (form, N, C, _err(ctx))
                _same(got, want, (form, N, C, M))


OTHER = {
    "M = 1": (6, 300, 1, 300, 3, 2),
    "W = 1, M W < C": (6, 300, 200, 1, 3, 2),
    "M longer than the weight sub-chunk (8 columns at A = 32, S = 16)": (4, 100, 37, 2, 32, 16),
    "M longer than the weight sub-chunk (256 / 512 columns at A = 7, S = 1)": (4, 1400, 650, 2, 7, 1),
    "C not a multiple of 4, windows inside groups of 16": (10, 1023, 7, 146, 4, 3),
    "S padded to 8": (6, 200, 50, 4, 5, 5),
}


@pytest.mark.parametrize("name", list(OTHER))
def test_other_shapes(ctx, name):
    N, C, M, W, A, S = OTHER[name]
    X, lab, w, eff = SC.case(N, C, M, W, A, S)
    want = SE.scores(X, lab, M, A, w, eff)
    for form in FORMS:
        rc, got, _ = _run(ctx, form, X, lab, M, A, w, eff)
        assert rc == 0, (form, _err(ctx))
        _same(got, want, form)


def test_bits_do_not_depend_on_the_grid_the_passes_the_run_or_N(ctx):
    N, C, M, W, A, S = 2 * ROW_TILE + 6, 777, 20, 38, 3, 2
    X, lab, w, eff = SC.case(N, C, M, W, A, S)
    want = SE.scores(X, lab, M, A, w, eff)
    for form in ("i8d", "p2d"):
        base = _run(ctx, form, X, lab, M, A, w, eff)[1]
        _same(base, want, form)
        _same(_run(ctx, form, X, lab, M, A, w, eff)[1], base, "run to run")
        for wpb, rpp in ((1, 0), (5, 0), (W, 0), (1000, 0), (0, 256), (3, 300)):
            _same(_run(ctx, form, X, lab, M, A, w, eff, wpb, rpp)[1], base, (form, wpb, rpp))
        half = N // 2 // 2 * 2                                               # the first half of the individuals alone: the same rows
        _same(_run(ctx, form, X[:half], lab[:half], M, A, w, eff)[1], [v[:half // 2] for v in base], "first half")
        one = _run(ctx, form, X[10:12], lab[10:12], M, A, w, eff)[1]
        _same(one, [v[5:6] for v in base], "one individual")
    # any output may be NULL: the others are written, a NULL one is not touched
    rc, got, _ = _run(ctx, "i8d", X, lab, M, A, w, eff, outs=(1, 0, 1, 0))
    assert rc == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and (got[1] == -7).all() and (got[3] == -7).all()
    rc, got, _ = _run(ctx, "p2h", X, lab, M, A, w, eff, outs=(0, 1, 0, 1))
    assert rc == 0 and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3]) and (got[0] == -7).all()


def test_labels_out_of_range_are_counted_and_count_for_no_ancestry(ctx):
    from gnomix_amd import _lib
    N, C, M, W, A, S = 20, 500, 50, 10, 4, 2
    X, lab, w, eff = SC.case(N, C, M, W, A, S)
    bad = lab.copy()
    bad[3, 0], bad[3, 9], bad[8, 4], bad[19, 9] = A, -1, 2 ** 30, -2 ** 31
    want = SE.scores(X, bad, M, A, w, eff)
    assert want[4] == 4
    for form in FORMS:
        rc, got, n_bad = _run(ctx, form, X, bad, M, A, w, eff)
        assert rc == _lib.GNX_EINVAL and n_bad == 4 and "4 labels lie outside [0, 4)" in _err(ctx), (form, rc, n_bad)
        _same(got, want, form)


def test_refusals_leave_the_outputs_untouched(ctx):
    from gnomix_amd import _lib
    N, C, M, W, A, S = 6, 40, 10, 4, 3, 2
    X, lab, w, eff = SC.case(N, C, M, W, A, S)
    lib, h = ctx.lib, ctx.h
    out = [np.full((N // 2, A, S), -7.0)] + [np.full((N // 2, A), -7, np.int32) for _ in range(3)]
    wide_w = SC.weights(np.random.RandomState(0), C, A, 17)

    def call(X=X, kind=0, ld=C, lab=lab, ldl=W, N=N, C=C, M=M, W=W, A=A, w=w, S=S, eff=eff, wpb=0, rpp=0):
        p = lambda v: None if v is None else v.ctypes.data
        return lib.gnx_ancestry_score(h, p(X), kind, ld, p(lab), ldl, N, C, M, W, A, p(w), S, p(eff), p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                      wpb, rpp, None)
    einval = [dict(kind=2), dict(N=-2), dict(N=5), dict(C=0), dict(A=0), dict(M=0), dict(W=0), dict(M=11), dict(W=5), dict(ld=C - 1),
              dict(kind=1, ld=(C + 3) // 4 - 1), dict(ldl=W - 1), dict(X=None), dict(lab=None), dict(S=0), dict(w=None), dict(eff=None),
              dict(wpb=-1), dict(rpp=-1)]
    for kw in einval:
        assert call(**kw) == _lib.GNX_EINVAL, kw
    assert call(A=33) == _lib.GNX_EUNSUPPORTED and call(S=17, w=wide_w) == _lib.GNX_EUNSUPPORTED
    assert call(C=2 ** 30, M=1, W=1, ld=2 ** 30) == _lib.GNX_EUNSUPPORTED
    # the device's checking pass: an effect byte outside {0, 1, 255}; a weight that is not finite at a scored SNP
    e2 = eff.copy()
    e2[[3, 17]] = 2, 254
    assert call(eff=e2) == _lib.GNX_EINVAL and "2 effect bytes" in _err(ctx)
    scored = np.nonzero(eff != 255)[0]
    w2 = w.copy()
    w2[scored[0], 1, 0], w2[scored[1], 2, 1], w2[scored[1], 0, 0] = np.nan, np.inf, -np.inf
    assert call(w=w2) == _lib.GNX_EINVAL and "3 weights at scored SNPs are not finite" in _err(ctx)
    assert all((v == -7).all() for v in out)
    # ... while a weight that is not finite at a SNP that is not scored is never read into a sum
    w3 = w.copy()
    w3[np.nonzero(eff == 255)[0]] = np.nan
    assert call(w=w3) == 0
    _same(out, SE.scores(X, lab, M, A, w, eff)[:4])
    for v in out:
        v[...] = -7
    assert call(N=0) == 0 and all((v == -7).all() for v in out)              # nobody: nothing is launched, nothing written
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.gnx_ancestry_score_dev(h, t.data_ptr(), 0, C, t.data_ptr(), W, 5, C, M, W, A, t.data_ptr(), S, t.data_ptr(), None, None, None, None, 0, 0,
                                      None) == _lib.GNX_EINVAL


# ---------------------------------------------------------------- through the model ------------------------------------------------
def _model(C=3037, M=50, A=4, seed=5):
    import dataclasses
    from gnomix_amd import synth
    d = synth.synthetic_model(C=C, M=M, A=A, S=11, n_rounds=4, seed=seed)
    return dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                               population_order=["P%d" % a for a in range(d.A)], gen_map_pos=np.array([1, 50_000, 200_000]),
                               gen_map_cm=np.array([0.0, 1.5, 9.25]))


def test_model_surface_follows_predict_and_equals_the_dosage_route(ga):
    import torch
    from gnomix_amd import synth
    from gnomix_amd import postprocess as pp
    d = _model()
    X = synth.synthetic_X(120, d.C, seed=3, miss=0.03)
    rng = np.random.RandomState(2)
    w = SC.weights(rng, d.C, d.A, 18)                       # more than GNX_SCORE_MAX_S scores: served in chunks
    for mf in (0, 5):
        g = ga.HipGnomix(d, device=0, mode_filter=mf)
        lab = np.ascontiguousarray(g.predict(X), dtype=np.int32)
        got = g.ancestry_scores(X, w)                       # effect = None: ALT everywhere
        assert type(got).__name__ == "AncestryScores" and got.score.shape == (60, d.A, 18) and got.n_effect.dtype == np.int32
        # the former route: the dosage matrix of each ancestry (gnx_ancestry_dosage) times the weights on the host, within the
        # derived bound (n - 1) 2^-53 sum |terms| of a sum of n terms in any order, on both sides (matmul's order is its own)
        for a in range(d.A):
            dos, hap = g.dev.ancestry_dosage(X, lab, a)
            n_terms = dos.sum(1, dtype=np.int64)
            assert np.array_equal(got.n_effect[:, a], n_terms)
            ref = dos.astype(np.float64) @ w[:, a, :]
            mag = dos.astype(np.float64) @ np.abs(w[:, a, :])
            tol = 2 * SE.bound(n_terms[:, None], mag[:, None, :])[:, 0, :]
            assert (np.abs(got.score[:, a, :] - ref) <= tol).all(), (mf, a)
        want = SE.scores(X, lab, d.M, d.A, w, np.ones(d.C, np.uint8))
        _same(got, want[:4], "HipGnomix, mode_filter %d" % mf)
        got_t = g.ancestry_scores(torch.from_numpy(X).cuda(), w)
        assert got_t.score.is_cuda and got_t.n_miss.dtype == torch.int32
        _same([v.cpu().numpy() for v in got_t], want[:4], "CUDA tensor")
    dev = g.dev
    Xt, lt = torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda()
    eff = rng.choice([1, 0, 255], size=d.C).astype(np.uint8)
    want = SE.scores(X, lab, d.M, d.A, w[:, :, :2], eff)[:4]
    _same(dev.ancestry_scores(X, lab, w[:, :, :2], eff), want, "host")
    _same(dev.ancestry_scores(dev.pack_x(X), lab, w[:, :, :2], eff, packed=True), want, "host, packed")
    for rows_t in (Xt, dev.pack_device(Xt)):
        _same([v.cpu().numpy() for v in dev.ancestry_scores_device(rows_t, lt, w[:, :, :2], eff)], want, "device")
    res_t = dev.ancestry_scores_device(Xt, lt, torch.from_numpy(w[:, :, :2]).cuda(), torch.from_numpy(eff).cuda())
    _same([v.cpu().numpy() for v in res_t], want, "device tables")
    one = dev.ancestry_scores(X, lab, w[:, 0, 0])          # (C,): the same weight for every ancestry
    same = dev.ancestry_scores(X, lab, np.repeat(w[:, :1, :1], d.A, axis=1))
    assert np.array_equal(one.score, same.score) and one.score.shape == (60, d.A, 1)
    assert np.allclose(pp.AncestryScores(*want).avg()[want[2] > 0], (want[0] / np.maximum(want[2], 1)[:, :, None])[want[2] > 0])
    dev.ctx.reset_stream()


def test_file_path_equals_the_matrix_path_whatever_the_batch(ga, tmp_path, monkeypatch):
    from gnomix_amd import synth, vcfio, _lib
    d = _model(C=4112, M=100, A=3, seed=7)
    X = synth.synthetic_X(34, d.C, seed=2, miss=0.03)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), 17, d.snp_pos, d.snp_ref, ["C"] * d.C)
    dev = ga.DeviceModel(d)
    vcf = vcfio.read_vcf(q, chm="22", ctx=dev.ctx)
    src, _, _ = vcfio.column_map(vcf, d.snp_pos, d.snp_ref, verbose=False)
    Xq = vcfio.vcf_to_npy(vcf, d.snp_pos, d.snp_ref, verbose=False).astype(np.int8)
    _, lab = dev.infer_gt2(vcf.gt2, 34, src, want_proba=False)
    rng = np.random.RandomState(3)
    w, eff = SC.weights(rng, d.C, d.A, 3), rng.choice([1, 0, 255], size=d.C).astype(np.uint8)
    want = dev.ancestry_scores(Xq, lab, w, eff)
    _same(want, SE.scores(Xq, lab, d.M, d.A, w, eff)[:4], "matrix path")
    _same(dev.ancestry_scores_gt2(vcf.gt2, 34, src, lab, w, eff), want, "one batch")
    # the library reads GNX_HOST_BATCH once per CONTEXT (gnx_init): two other batch sizes, each set for a fresh context's call alone
    for batch in ("12", "4"):
        monkeypatch.setenv("GNX_HOST_BATCH", batch)
        ctx2 = _lib.Context(0)
        monkeypatch.delenv("GNX_HOST_BATCH")
        dev2 = ga.DeviceModel(d, ctx=ctx2)
        _same(dev2.ancestry_scores_gt2(np.array(vcf.gt2), 34, src, lab, w, eff), want, "GNX_HOST_BATCH=" + batch)
        ctx2.close()
    bad = lab.copy()
    bad[3, 5] = d.A
    with pytest.raises(_lib.GnxError, match="1 labels lie outside"):
        dev.ancestry_scores_gt2(vcf.gt2, 34, src, bad, w, eff)
    w[np.nonzero(eff != 255)[0][0], 0, 0] = np.nan
    with pytest.raises(_lib.GnxError, match="1 weights at scored SNPs are not finite"):
        dev.ancestry_scores_gt2(vcf.gt2, 34, src, lab, w, eff)


def test_command_line_writes_sscore_only_when_asked(ga, tmp_path):
    from gnomix_amd import score, synth, vcfio, cli
    from gnomix_amd import postprocess as pp
    d = _model()
    pops = list(d.population_order)
    X = synth.synthetic_X(60, d.C, seed=3, miss=0.03)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    g = ga.HipGnomix(d, device=0)
    samples = [str(s) for s in vcfio.read_vcf(q, chm="22", ctx=g.dev.ctx)["samples"]]
    rng = np.random.RandomState(8)
    lines = ["chm\tpos\teffect_allele\tprs\tlipid:P1\tlipid:P3"]
    for c in range(0, d.C, 3):
        lines.append("22\t%d\t%s\t%r\t%r\t%r" % (d.snp_pos[c], "AC"[c % 2], *[float(v) for v in rng.normal(size=3) * np.exp2(rng.randint(-20, 21, 3))]))
    lines += ["21\t1000\tC\t1\t1\t1", "22\t7\tC\t1\t1\t1", "22\t%d\tG\t1\t1\t1" % d.snp_pos[1]]
    sf = tmp_path / "scores.tsv"
    sf.write_text("\n".join(lines) + "\n")

    def run(name, phase=False, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, **kw)
        return od
    off, on = run("off"), run("on", ancestry_score_output=True, score_file=str(sf))
    assert sorted(os.listdir(str(off))) == ["query_results.fb", "query_results.msp"]                 # the key absent: the files as before
    assert sorted(os.listdir(str(on))) == ["query_results.fb", "query_results.msp", "query_results.sscore.tsv"]
    for f in ("query_results.fb", "query_results.msp"):
        assert (off / f).read_bytes() == (on / f).read_bytes()
    rows = [ln.split("\t") for ln in (on / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)           # the labels that went to the .msp
    w, eff, names, rep = score.read_score_file(str(sf), "22", d.snp_pos, d.snp_ref, d.snp_alt, pops)
    assert names == ["prs", "lipid"] and rep == {"scored": len(range(0, d.C, 3)), "other_chm": 1, "not_in_model": 1, "allele_mismatch": 1}
    res = g.dev.ancestry_scores(X, lab, w, eff)                                                        # the Python API on the matrix
    _same(res, SE.scores(X, lab, d.M, d.A, w, eff)[:4], "Python API")
    pp.write_sscore(str(tmp_path / "want"), res, names, pops, samples)
    text = (on / "query_results.sscore.tsv").read_text()
    assert text == (tmp_path / "want.sscore.tsv").read_text() and len(text.splitlines()) == 1 + len(samples)
    assert res.n_effect.sum() > 0 and (eff == 0).any() and (eff == 1).any()
    with pytest.raises(ValueError, match="ancestry_scores"):
        run("phased", phase=True, ancestry_score_output=True, score_file=str(sf))
    assert os.listdir(str(tmp_path / "phased")) == []
    with pytest.raises(ValueError, match="score_file"):
        run("nofile", ancestry_score_output=True)
    assert os.listdir(str(tmp_path / "nofile")) == []
