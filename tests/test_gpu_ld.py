"""gnx_ancestry_ld_counts[_dev / _gt2] (csrc/summary/k_ancestry_ld.hip) and the layers built on it, on the MI355X, against the numpy
restatement (tests/ld_exact.py): all four int32 tables exactly.

The kernel's sizes the shapes are chosen by (tests/ld_cases.py): an MFMA tile of 16 SNPs, a SNP tile of 64, K = 64 haplotypes, a staging
chunk of 128 haplotypes, items of 4 haplotypes x 16 SNPs.  Row forms: 'i8h' int8 rows through the host entry with a stride of C + 5
(unaligned: the byte route); 'i8d' int8 rows through the device entry with a 16-byte aligned stride; 'p2h' / 'p2d' 2-bit rows likewise
(stride + 3 bytes / a multiple of 4).  Poison behind every row, labels with a row stride of W + 3, tables with a row stride of band + 3."""
import ctypes
import os

import numpy as np
import pytest

import allele_counts_exact as AE
import ld_cases as LC
import ld_exact as LE

pytestmark = pytest.mark.gpu

FORMS = ("i8h", "i8d", "p2h", "p2d")
NAMES = ("n11", "n1o", "no1", "noo")
POISON = -7


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


class Rows:
    """one case in one row form, built (and for the device forms uploaded) once, run for any range and band"""

    def __init__(self, ctx, form, X, lab, M, A, a):
        self.ctx, self.form, self.M, self.A, self.a = ctx, form, M, A, a
        self.N, self.C = X.shape
        self.W = lab.shape[1]
        self.packed = form.startswith("p2")
        C = self.C
        if self.packed:
            self.ld = (C + 3) // 4 + 3 if form == "p2h" else ((C + 3) // 4 + 3) // 4 * 4 + 4
            self.rows = AE.pack2(LC.codes(X), ldp=self.ld, fill=0x55)
        else:
            self.ld = C + 5 if form == "i8h" else (C + 15) // 16 * 16 + 16
            self.rows = np.full((self.N, self.ld), 1, np.int8)
            self.rows[:, :C] = X
        self.wide = np.full((self.N, self.W + 3), a, np.int32)
        self.wide[:, :self.W] = lab
        if form.endswith("d"):
            import torch
            self.t = [torch.from_numpy(v).cuda() for v in (self.rows, self.wide)]

    def run(self, c0, c1, band, dbg=0, outs=(1, 1, 1, 1), pad=3):
        """-> rc, the four (c1 - c0, band + pad) int32 tables with POISON where nothing was written, n_bad"""
        lib, h = self.ctx.lib, self.ctx.h
        out = [np.full((c1 - c0, band + pad), POISON, np.int32) for _ in range(4)]
        n_bad = ctypes.c_int64(-1)
        head = (int(self.packed), self.ld)
        geo = (self.W + 3, self.N, self.C, self.M, self.W, self.A, self.a, c0, c1, band)
        if self.form.endswith("h"):
            p = [o.ctypes.data if use else None for o, use in zip(out, outs)]
            rc = lib.gnx_ancestry_ld_counts(h, self.rows.ctypes.data, *head, self.wide.ctypes.data, *geo, *p, band + pad, dbg, ctypes.byref(n_bad))
            return rc, out, n_bad.value
        import torch
        o = [torch.from_numpy(v).cuda() for v in out]
        p = [v.data_ptr() if use else None for v, use in zip(o, outs)]
        rc = lib.gnx_ancestry_ld_counts_dev(h, self.t[0].data_ptr(), *head, self.t[1].data_ptr(), *geo, *p, band + pad, dbg, ctypes.byref(n_bad))
        torch.cuda.synchronize()
        return rc, [v.cpu().numpy() for v in o], n_bad.value


def _same(got, want, where="", outs=(1, 1, 1, 1)):
    for g, w, use, name in zip(got, want, outs, NAMES):
        band = w.shape[1]
        assert g.dtype == np.int32 and (g[:, band:] == POISON).all(), (name, where)       # nothing behind a row's band columns
        if use:
            assert np.array_equal(g[:, :band], w), (name, where)
        else:
            assert (g == POISON).all(), (name, where)


# ---------------------------------------------------------------- the grid of shapes -----------------------------------------------
@pytest.mark.parametrize("A", LC.AS)
@pytest.mark.parametrize("N", LC.NS)
def test_grid_equals_the_restatement(ctx, N, A):
    asym = False
    for C in LC.CS:
        for M0 in LC.MS:
            M, W = LC.geometry(C, M0)
            X, lab = LC.case(N, C, M, W, A)
            a = (C + M) % A
            full = LE.full_tables(X, lab, M, a)
            asym = asym or not np.array_equal(full[1], full[2])           # n1o != no1 on the data: a swapped or transposed store cannot pass
            rows = [Rows(ctx, form, X, lab, M, A, a) for form in FORMS]
            for band in LC.bands_for(C):
                want = LE.tables(X, lab, M, A, a, 0, C, band, full=full)
                assert want[4] == 0
                for r in rows:
                    rc, got, n_bad = r.run(0, C, band)
                    assert rc == 0 and n_bad == 0, (r.form, N, C, M, band, _err(ctx))
                    _same(got, want, (r.form, N, C, M, band))
    assert asym


@pytest.mark.parametrize("N,M", [(129, 24), (5, 1)])
def test_ranges_partitions_split_and_null_tables(ctx, N, M):
    C, A, a = 200, 3, 1
    M, W = LC.geometry(C, M)
    X, lab = LC.case(N, C, M, W, A, seed=2)
    full = LE.full_tables(X, lab, M, a)
    for fi, form in enumerate(FORMS):
        r = Rows(ctx, form, X, lab, M, A, a)
        for band in (17, 65, 130):
            for c0, c1 in LC.RANGES:
                want = LE.tables(X, lab, M, A, a, c0, c1, band, full=full)
                ref = None
                for dbg in (0, 4, 128, 132):
                    rc, got, n_bad = r.run(c0, c1, band, dbg=dbg, pad=fi)
                    assert rc == 0 and n_bad == 0, (form, c0, c1, band, dbg, _err(ctx))
                    _same(got, want, (form, c0, c1, band, dbg))
                    ref = got if ref is None else ref
                    assert all(np.array_equal(g, q) for g, q in zip(got, ref))              # the split changes nothing
            # a range's tables are the stacked tables of a partition of it
            whole = LE.tables(X, lab, M, A, a, 3, 197, band, full=full)
            cuts = (3, 16, 64, 70, 131, 197)
            parts = [r.run(u, v, band, pad=0)[1] for u, v in zip(cuts[:-1], cuts[1:])]
            for q in range(4):
                assert np.array_equal(np.concatenate([p[q] for p in parts], axis=0), whole[q]), (form, band, NAMES[q])
        whole = LE.tables(X, lab, M, A, a, 0, C, 65, full=full)
        for outs in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
            for dbg in (0, 128):
                rc, got, _ = r.run(0, C, 65, dbg=dbg, outs=outs)
                assert rc == 0
                _same(got, whole, (form, outs, dbg), outs)


def test_an_ancestry_nobody_carries_and_one_everybody_carries(ctx):
    N, C, M, A, band = 130, 200, 5, 3, 70
    M, W = LC.geometry(C, M)
    X, lab = LC.case(N, C, M, W, 2)                       # labels in {0, 1}: nobody carries 2
    for form in FORMS:
        rc, got, _ = Rows(ctx, form, X, lab, M, A, 2).run(0, C, band)
        assert rc == 0 and all((g[:, :band] == 0).all() for g in got), form
    lab[...] = 1
    want = LE.tables(X, lab, M, A, 1, 0, C, band)
    obs = ((X == 0) | (X == 1)).astype(np.int64)
    assert np.array_equal(want[3], LE.banded(obs.T @ obs, 0, C, band)) and want[3][0, 0] < N      # row 1 is all missing
    for form in FORMS:
        rc, got, _ = Rows(ctx, form, X, lab, M, A, 1).run(0, C, band)
        assert rc == 0
        _same(got, want, form)


def test_labels_out_of_range_are_counted_after_the_launch(ctx):
    from gnomix_amd import _lib
    N, C, M, A, a, band = 35, 200, 7, 3, 2, 40
    M, W = LC.geometry(C, M)
    X, lab = LC.case(N, C, M, W, A, seed=3, bad=9)
    counts = set()
    for c0, c1 in ((0, C), (30, 60), (100, 101)):
        want = LE.tables(X, lab, M, A, a, c0, c1, band)
        counts.add(want[4])
        for form in FORMS:
            rc, got, n_bad = Rows(ctx, form, X, lab, M, A, a).run(c0, c1, band)
            if want[4]:
                assert rc == _lib.GNX_EINVAL and "%d labels lie outside [0, %d)" % (want[4], A) in _err(ctx), form
            else:
                assert rc == 0
            assert n_bad == want[4]
            _same(got, want, form)
    assert 9 in counts and len(counts) > 1
    # the band's windows count, not the range's alone
    assert LE.n_bad(lab, M, A, C, 100, 101, band) == LE.n_bad(lab, M, A, C, 100, 140, 1)


def test_refusals_leave_the_outputs_untouched(ctx):
    from gnomix_amd import _lib
    lib, h = ctx.lib, ctx.h
    N, C, M, W, A, band = 5, 40, 7, 5, 3, 6
    X, lab = LC.case(N, C, M, W, A)
    out = [np.full((C, band), POISON, np.int32) for _ in range(4)]
    n_bad = ctypes.c_int64(-1)

    def call(**kw):
        v = dict(kind=0, ld_rows=C, ldl=W, N=N, C=C, M=M, W=W, A=A, a=1, c0=0, c1=C, band=band, ld=band, dbg=0)
        v.update(kw)
        return lib.gnx_ancestry_ld_counts(h, X.ctypes.data, v["kind"], v["ld_rows"], lab.ctypes.data, v["ldl"], v["N"], v["C"], v["M"], v["W"], v["A"],
                                          v["a"], v["c0"], v["c1"], v["band"], out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                          out[3].ctypes.data, v["ld"], v["dbg"], ctypes.byref(n_bad))
    einval = [dict(N=-2), dict(C=0), dict(A=0), dict(M=0), dict(W=0), dict(W=6), dict(ld_rows=C - 1), dict(ldl=W - 1), dict(kind=2),
              dict(a=-1), dict(a=A), dict(c0=-1), dict(c1=0), dict(c0=7, c1=7), dict(c1=C + 1), dict(band=0), dict(band=-3), dict(ld=band - 1),
              dict(dbg=-1), dict(N=2 ** 31)]
    for kw in einval:
        assert call(**kw) == _lib.GNX_EINVAL, kw
        assert all((v == POISON).all() for v in out), kw
    assert call(A=33, a=1) == _lib.GNX_EUNSUPPORTED and "at most 32" in _err(ctx)
    assert call(band=_lib.GNX_LD_MAX_BAND + 1, ld=_lib.GNX_LD_MAX_BAND + 1) == _lib.GNX_EUNSUPPORTED and "at most 4096" in _err(ctx)
    assert all((v == POISON).all() for v in out)
    assert call(N=0) == 0 and all((v == POISON).all() for v in out) and n_bad.value == 0   # nobody: nothing launched, nothing written
    assert call() == 0                                                                     # (N = 5: odd is fine here)
    want = LE.tables(X, lab, M, A, 1, 0, C, band)
    assert all(np.array_equal(g, w) for g, w in zip(out, want[:4]))
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.gnx_ancestry_ld_counts_dev(h, t.data_ptr(), 0, C, t.data_ptr(), W, 5, C, M, W, A, 0, 0, C, 0, None, None, None, None, 3, 0,
                                          None) == _lib.GNX_EINVAL


# ---------------------------------------------------------------- through the model ------------------------------------------------
def _model(C=3037, M=50, A=3, seed=5):
    import dataclasses
    from gnomix_amd import synth
    d = synth.synthetic_model(C=C, M=M, A=A, S=11, n_rounds=4, seed=seed)
    return dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                               population_order=["P%d" % a for a in range(d.A)], gen_map_pos=np.array([1, 50_000, 200_000]),
                               gen_map_cm=np.array([0.0, 1.5, 9.25]))


def _eq(got, want, where=""):
    for g, w, name in zip(got[:4], want[:4], NAMES):
        g = g.cpu().numpy() if hasattr(g, "is_cuda") else g
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, where)


def _query(tmp_path, d, n_ind, rng, drop=150, flip_frac=0.05, miss=0.02):
    """SNP metadata for the model + a query VCF that lacks `drop` model SNPs, has SNPs of its own, REF mismatches and missing calls"""
    from gnomix_amd import synth, vcfio
    d.snp_pos = np.sort(rng.choice(np.arange(10_000, 9_000_000), size=d.C, replace=False))
    d.snp_ref = rng.choice(list("ACGT"), size=d.C)
    d.snp_alt = rng.choice(list("ACGT"), size=d.C)
    keep = np.sort(rng.choice(d.C, size=d.C - drop, replace=False))
    extra = np.setdiff1d(rng.choice(np.arange(10_000, 9_000_000), size=200), d.snp_pos)
    qpos = np.concatenate([d.snp_pos[keep], extra])
    qref = np.concatenate([d.snp_ref[keep], rng.choice(list("ACGT"), len(extra))])
    fl = rng.random(len(keep)) < flip_frac
    qref[:len(keep)][fl] = np.where(qref[:len(keep)][fl] == "A", "C", "A")
    order = np.argsort(qpos)
    Xq = synth.synthetic_X(2 * n_ind, len(qpos), seed=int(rng.integers(1 << 30)), miss=miss)
    return synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(Xq[:, order]), n_ind, qpos[order], qref[order], ["N"] * len(qpos), chrom="22")


def test_file_path_equals_the_matrix_path_whatever_the_batch(ga, tmp_path, monkeypatch):
    from gnomix_amd import synth, vcfio, _lib
    C_, M, A, n_ind, band = 2130, 64, 3, 67, 70            # 134 haplotypes: two chunks
    rng = np.random.default_rng(C_)
    d = synth.synthetic_model(C=C_, M=M, A=A, S=11, n_rounds=4, seed=C_)
    q = _query(tmp_path, d, n_ind, rng)
    dev = ga.DeviceModel(d)
    vcf = vcfio.read_vcf(q, chm="22", ctx=dev.ctx)
    src, _, _ = vcfio.column_map(vcf, d.snp_pos, d.snp_ref, verbose=False)
    assert (src >> 30 == 1).any() and (src == -1).any()     # a REF-flipped SNP, a model SNP the query lacks
    N = 2 * n_ind
    Xq = vcfio.vcf_to_npy(vcf, d.snp_pos, d.snp_ref, verbose=False).astype(np.int8)
    _, lab = dev.infer_gt2(vcf.gt2, N, src, want_proba=False)
    a = int(np.bincount(lab.ravel(), minlength=A).argmax())
    for c0, c1 in ((0, C_), (77, 1990)):
        want = LE.tables(Xq, lab, M, A, a, c0, c1, band)
        assert want[3].sum() > 0
        _eq(dev.ancestry_ld_counts(Xq, lab, a, c0, c1, band), want, "matrix path")
        got = dev.ancestry_ld_counts_gt2(vcf.gt2, N, src, lab, a, c0, c1, band)
        assert type(got).__name__ == "LDCounts" and (got.c0, got.band) == (c0, band)
        _eq(got, want, "one batch")
    want = LE.tables(Xq, lab, M, A, a, 0, C_, band)
    # the library reads GNX_HOST_BATCH once per CONTEXT (gnx_init): two other batch sizes, each set for a fresh context's call alone
    for batch in ("40", "4"):
        monkeypatch.setenv("GNX_HOST_BATCH", batch)
        ctx2 = _lib.Context(0)
        monkeypatch.delenv("GNX_HOST_BATCH")
        dev2 = ga.DeviceModel(d, ctx=ctx2)
        _eq(dev2.ancestry_ld_counts_gt2(np.array(vcf.gt2), N, src, lab, a, band=band), want, "GNX_HOST_BATCH=" + batch)
        ctx2.close()
    bad = lab.copy()
    bad[3, 5] = A
    with pytest.raises(_lib.GnxError, match="1 labels lie outside"):
        dev.ancestry_ld_counts_gt2(vcf.gt2, N, src, bad, a, band=band)
    with pytest.raises(_lib.GnxError, match="ancestry outside"):
        dev.ancestry_ld_counts_gt2(vcf.gt2, N, src, lab, A, band=band)
    worse = src.copy()
    worse[0] = vcf.gt2.shape[0]
    with pytest.raises(_lib.GnxError, match="column map entry"):
        dev.ancestry_ld_counts_gt2(vcf.gt2, N, worse, lab, a, band=band)


def _assoc_like(C, A, seed):
    """p-values that give every ancestry index SNPs, clumped SNPs and SNPs left out; ties and NaN among them"""
    import collections
    rng = np.random.RandomState(seed)
    p = np.round(10.0 ** rng.uniform(-6, 0, size=(C, A)), 6)
    p[rng.choice(C, 40, replace=False), rng.randint(0, A, size=40)] = np.nan
    return collections.namedtuple("Res", "beta p")(rng.standard_normal((C, A)), p)


def test_clump_through_the_model_equals_the_literal_loops(ga):
    import torch
    from gnomix_amd import ld, score
    d = _model(C=1237, M=50, A=3, seed=7)
    X = LC.linked(130, d.C, seed=3, block=5)
    g = ga.HipGnomix(d, device=0)
    lab = np.ascontiguousarray(g.predict(X), dtype=np.int32)
    res = _assoc_like(d.C, d.A, 1)
    opts = dict(p1=1e-3, p2=5e-2, r2=0.3, kb=0.5)
    band = ld.band_for(d.snp_pos, opts["kb"])
    assert band == 14                                                       # 37 bp apart: 500 bp reach 13 SNPs further
    got = g.ancestry_clump(X, res, **opts)
    assert got.shape == (d.C, d.A) and got.dtype == np.int64
    for a in range(d.A):
        tabs = LE.tables(X, lab, d.M, d.A, a, 0, d.C, band)[:4]
        want = LE.clump_literal(res.p[:, a], d.snp_pos, tabs, band, **opts)
        assert np.array_equal(got[:, a], want), a
        _eq(g.ancestry_ld(X, a, 101, 900, band), LE.tables(X, lab, d.M, d.A, a, 101, 900, band), "ancestry_ld")
    assert ((got >= 0) & (got != np.arange(d.C)[:, None])).sum() > 20       # clumps with members
    assert np.array_equal(g.ancestry_clump(torch.from_numpy(X).cuda(), res, **opts), got)
    t = g.ancestry_ld(torch.from_numpy(X).cuda(), 0, 5, 70, 9)
    assert t.noo.is_cuda and t.n11.dtype == torch.int32 and tuple(t.n1o.shape) == (65, 9)
    w = score.weights_from_assoc(res, 1e-3, got)
    assert np.array_equal(w != 0, (got == np.arange(d.C)[:, None]) & (res.p <= 1e-3))
    g.dev.ctx.reset_stream()


def test_command_line_writes_clumps_only_when_asked(ga, tmp_path):
    from gnomix_amd import assoc, ld, synth, vcfio, cli
    from gnomix_amd import postprocess as pp
    d = _model(C=1237, M=50, A=3, seed=7)
    X = LC.linked(120, d.C, seed=5, block=5)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    g = ga.HipGnomix(d, device=0)
    vcf = vcfio.read_vcf(q, chm="22", ctx=g.dev.ctx)
    src, _, _ = vcfio.column_map(vcf, d.snp_pos, d.snp_ref, verbose=False)
    samples = [str(s) for s in vcf["samples"]]
    rng = np.random.RandomState(2)
    y = X[0::2, 300].astype(np.float64) + X[1::2, 300] + X[0::2, 800] + X[1::2, 800] + 0.5 * rng.standard_normal(len(samples))
    ph = tmp_path / "pheno.tsv"
    ph.write_text("sample\tpheno\n" + "".join("%s\t%r\n" % (s, float(v)) for s, v in zip(samples, y)))

    def run(name, phase=False, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, **kw)
        return od
    opts = dict(p1=1e-2, p2=0.2, r2=0.2, kb=0.5)
    off = run("off", ancestry_assoc_output=True, phenotype_file=str(ph))
    on = run("on", ancestry_assoc_output=True, phenotype_file=str(ph), ancestry_clump_output=True,
             **{"ancestry_clump_" + k: v for k, v in opts.items()})
    base = ["query_results.assoc.tsv", "query_results.fb", "query_results.msp"]
    assert sorted(os.listdir(str(off))) == base                                 # the key absent: the files as before
    assert sorted(os.listdir(str(on))) == sorted(base + ["query_results.clumped.tsv"])
    for f in base:
        assert (off / f).read_bytes() == (on / f).read_bytes()
    # the Python route: the labels that went to the .msp, the association of the matrix path, clump over the restatement-checked tables
    rows = [ln.split("\t") for ln in (on / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)
    yy, Z, use, _ = assoc.read_phenotypes(str(ph), samples)
    res = g.dev.ancestry_assoc_gt2(vcf.gt2, X.shape[0], src, lab, yy, Z, use)
    band = ld.band_for(d.snp_pos, opts["kb"])
    index_of = np.full((d.C, d.A), -1, np.int64)
    for a in range(d.A):
        tabs = LE.tables(X, lab, d.M, d.A, a, 0, d.C, band)[:4]
        index_of[:, a] = LE.clump_literal(res.p[:, a], d.snp_pos, tabs, band, **opts)
    pp.write_clumps(str(tmp_path / "want"), "22", d.snp_pos, index_of, res.p, d.population_order)
    text = (on / "query_results.clumped.tsv").read_text()
    assert text == (tmp_path / "want.clumped.tsv").read_text()
    assert text.count("\n") > 3 and any(ln.split("\t")[4] != "0" for ln in text.splitlines()[1:])
    with pytest.raises(ValueError, match="ancestry_clump"):
        run("phased", phase=True, ancestry_assoc_output=True, phenotype_file=str(ph), ancestry_clump_output=True)
    assert os.listdir(str(tmp_path / "phased")) == []
