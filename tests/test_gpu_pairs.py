"""gnx_ancestry_pair_counts[_dev / _gt2] (csrc/summary/k_ancestry_pairs.hip) and the layers built on it, on the MI355X, against the numpy
restatement (tests/pairs_exact.py): all three int32 tables exactly.

The kernel's sizes the shapes are chosen by (tests/pairs_cases.py): an MFMA tile of 16 individuals, a macro-tile of 64, K = 64 SNPs, a
staging chunk of 128 SNPs, groups of 16 SNPs.  Row forms: 'i8h' int8 rows through the host entry with a stride of C + 5 (unaligned:
the byte route); 'i8d' int8 rows through the device entry with a 16-byte aligned stride; 'p2h' / 'p2d' 2-bit rows likewise (stride + 3
bytes / a multiple of 4).  Poison behind every row, labels with a row stride of W + 3, tables with a row stride of n + 3."""
import ctypes
import os

import numpy as np
import pytest

import allele_counts_exact as AE
import pairs_cases as PC
import pairs_exact as PE

pytestmark = pytest.mark.gpu

FORMS = ("i8h", "i8d", "p2h", "p2d")
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


def _run(ctx, form, X, lab, M, A, a, c0=0, c1=None, dbg=0, outs=(1, 1, 1), pad=3):
    """-> rc, [DD, DO, OO] (n, n + pad) int32 with POISON where nothing was written, n_bad"""
    N, C = X.shape
    W = lab.shape[1]
    c1 = C if c1 is None else c1
    packed = form.startswith("p2")
    if packed:
        ld = (C + 3) // 4 + 3 if form == "p2h" else ((C + 3) // 4 + 3) // 4 * 4 + 4
        rows = AE.pack2(PC.codes(X), ldp=ld, fill=0x55)
    else:
        ld = C + 5 if form == "i8h" else (C + 15) // 16 * 16 + 16
        rows = np.full((N, ld), 1, np.int8)
        rows[:, :C] = X
    wide = np.full((N, W + 3), a, np.int32)
    wide[:, :W] = lab
    n = N // 2
    out = [np.full((n, n + pad), POISON, np.int32) for _ in range(3)]
    n_bad = ctypes.c_int64(-1)
    if form.endswith("h"):
        p = [o.ctypes.data if use else None for o, use in zip(out, outs)]
        rc = ctx.lib.gnx_ancestry_pair_counts(ctx.h, rows.ctypes.data, int(packed), ld, wide.ctypes.data, W + 3, N, C, M, W, A, a, c0, c1, p[0], p[1], p[2],
                                              n + pad, dbg, ctypes.byref(n_bad))
        return rc, out, n_bad.value
    import torch
    t = [torch.from_numpy(v).cuda() for v in (rows, wide)]
    o = [torch.from_numpy(v).cuda() for v in out]
    p = [v.data_ptr() if use else None for v, use in zip(o, outs)]
    rc = ctx.lib.gnx_ancestry_pair_counts_dev(ctx.h, t[0].data_ptr(), int(packed), ld, t[1].data_ptr(), W + 3, N, C, M, W, A, a, c0, c1, p[0], p[1], p[2],
                                              n + pad, dbg, ctypes.byref(n_bad))
    torch.cuda.synchronize()
    return rc, [v.cpu().numpy() for v in o], n_bad.value


def _same(got, want, where="", outs=(1, 1, 1)):
    for g, w, use, name in zip(got, want, outs, ("DD", "DO", "OO")):
        n = w.shape[0]
        assert g.dtype == np.int32 and (g[:, n:] == POISON).all(), (name, where)          # nothing behind a row's n columns
        if use:
            assert np.array_equal(g[:, :n], w), (name, where)
        else:
            assert (g == POISON).all(), (name, where)


# ---------------------------------------------------------------- the grid of shapes -----------------------------------------------
@pytest.mark.parametrize("A", PC.AS)
@pytest.mark.parametrize("N", PC.NS)
def test_grid_equals_the_restatement(ctx, N, A):
    asym = False
    for C in PC.CS:
        for M0 in PC.MS:
            M, W = PC.geometry(C, M0)
            X, lab = PC.case(N, C, M, W, A)
            a = (C + M) % A
            want = PE.tables(X, lab, M, A, a)
            assert want[3] == 0
            asym = asym or not np.array_equal(want[1], want[1].T)
            assert np.array_equal(want[0], want[0].T) and np.array_equal(want[2], want[2].T)
            assert np.array_equal(np.diagonal(want[2]), (PE.d_o(X, lab, M, a)[1] ** 2).sum(1))
            for form in FORMS:
                rc, got, n_bad = _run(ctx, form, X, lab, M, A, a)
                assert rc == 0 and n_bad == 0, (form, N, C, M, _err(ctx))
                _same(got, want, (form, N, C, M))
    assert asym or N == 2               # DO != DO^T on the data: a transposed store cannot pass


def test_an_ancestry_nobody_carries_and_one_everybody_carries(ctx):
    N, C, M, A = 130, 200, 7, 3
    M, W = PC.geometry(C, M)
    X, lab = PC.case(N, C, M, W, 2)                       # labels in {0, 1}: nobody carries 2
    for form in FORMS:
        rc, got, _ = _run(ctx, form, X, lab, M, A, 2)
        assert rc == 0 and all((g[:, :N // 2] == 0).all() for g in got), form
    lab[...] = 1
    want = PE.tables(X, lab, M, A, 1)
    obs = ((X == 0) | (X == 1)).astype(np.int64)
    o = obs[0::2] + obs[1::2]
    assert np.array_equal(want[2], o @ o.T) and want[2][0, 0] < 4 * C      # row 1 is all missing: individual 0 has one haplotype
    for form in FORMS:
        rc, got, _ = _run(ctx, form, X, lab, M, A, 1)
        assert rc == 0
        _same(got, want, form)
    assert not np.array_equal(want[1], want[1].T)


@pytest.mark.parametrize("N,C,M", [(34, 1031, 7), (258, 333, 64), (6, 65, 1)])
def test_ranges_partitions_split_and_null_tables(ctx, N, C, M):
    A, a = 3, 1
    M, W = PC.geometry(C, M)
    X, lab = PC.case(N, C, M, W, A, seed=2)
    whole = PE.tables(X, lab, M, A, a)
    cuts = sorted({0, min(C, 5), min(C, 64), C // 2 + 1, min(C, 2 * (C // 3) + 3), C})    # inside windows, groups and chunks
    for fi, form in enumerate(FORMS):
        total = [np.zeros_like(whole[0]) for _ in range(3)]
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            want = PE.tables(X, lab, M, A, a, c0, c1)
            ref = None
            for dbg in (0, 64, 192):
                rc, got, n_bad = _run(ctx, form, X, lab, M, A, a, c0, c1, dbg=dbg, pad=fi)
                assert rc == 0 and n_bad == 0, (form, c0, c1, dbg, _err(ctx))
                _same(got, want, (form, c0, c1, dbg))
                ref = got if ref is None else ref
                assert all(np.array_equal(g, r) for g, r in zip(got, ref))                 # the split changes nothing
            for q in range(3):
                total[q] += want[q]
        assert all(np.array_equal(t, w) for t, w in zip(total, whole[:3]))                 # a partition adds up to the whole
        for outs in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
            for dbg in (0, 128):
                rc, got, _ = _run(ctx, form, X, lab, M, A, a, dbg=dbg, outs=outs)
                assert rc == 0
                _same(got, whole, (form, outs, dbg), outs)


def test_labels_out_of_range_are_counted_after_the_launch(ctx):
    from gnomix_amd import _lib
    N, C, M, A, a = 34, 200, 7, 3, 2
    M, W = PC.geometry(C, M)
    X, lab = PC.case(N, C, M, W, A, seed=3, bad=5)
    for c0, c1 in ((0, C), (30, 100)):
        want = PE.tables(X, lab, M, A, a, c0, c1)
        assert want[3] > 0 if (c0, c1) == (0, C) else True
        for form in FORMS:
            rc, got, n_bad = _run(ctx, form, X, lab, M, A, a, c0, c1)
            if want[3]:
                assert rc == _lib.GNX_EINVAL and "%d labels lie outside [0, %d)" % (want[3], A) in _err(ctx), form
            else:
                assert rc == 0
            assert n_bad == want[3]
            _same(got, want, form)
    assert PE.tables(X, lab, M, A, a)[3] == 5


def test_refusals_leave_the_outputs_untouched(ctx):
    from gnomix_amd import _lib
    lib, h = ctx.lib, ctx.h
    N, C, M, W, A = 6, 40, 7, 5, 3
    X, lab = PC.case(N, C, M, W, A)
    out = [np.full((3, 3), POISON, np.int32) for _ in range(3)]
    n_bad = ctypes.c_int64(-1)

    def call(**kw):
        v = dict(kind=0, ld_rows=C, ldl=W, N=N, C=C, M=M, W=W, A=A, a=1, c0=0, c1=C, ld=3, dbg=0)
        v.update(kw)
        return lib.gnx_ancestry_pair_counts(h, X.ctypes.data, v["kind"], v["ld_rows"], lab.ctypes.data, v["ldl"], v["N"], v["C"], v["M"], v["W"], v["A"],
                                            v["a"], v["c0"], v["c1"], out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, v["ld"], v["dbg"],
                                            ctypes.byref(n_bad))
    einval = [dict(N=-2), dict(C=0), dict(A=0), dict(M=0), dict(W=0), dict(W=6), dict(ld_rows=C - 1), dict(ldl=W - 1), dict(kind=2), dict(N=5),
              dict(a=-1), dict(a=A), dict(c0=-1), dict(c1=0), dict(c0=7, c1=7), dict(c1=C + 1), dict(ld=2), dict(dbg=-1), dict(N=2 ** 31)]
    for kw in einval:
        assert call(**kw) == _lib.GNX_EINVAL, kw
        assert all((v == POISON).all() for v in out), kw
    assert call(A=33, a=1) == _lib.GNX_EUNSUPPORTED and "at most 32" in _err(ctx)
    big = 2 ** 29 + 8
    assert call(C=big, M=big, W=1, ld_rows=big, c1=big) == _lib.GNX_EUNSUPPORTED and "2^29" in _err(ctx)
    assert call(C=big, M=big, W=1, ld_rows=big, c0=1, c1=2 ** 29 + 1) == _lib.GNX_EUNSUPPORTED
    assert all((v == POISON).all() for v in out)
    assert call(N=0) == 0 and all((v == POISON).all() for v in out) and n_bad.value == 0   # nobody: nothing launched, nothing written
    assert call() == 0
    want = PE.tables(X, lab, M, A, 1)
    assert all(np.array_equal(g, w) for g, w in zip(out, want[:3]))
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.gnx_ancestry_pair_counts_dev(h, t.data_ptr(), 0, C, t.data_ptr(), W, 5, C, M, W, A, 0, 0, C, None, None, None, 3, 0, None) == _lib.GNX_EINVAL


# ---------------------------------------------------------------- through the model ------------------------------------------------
def _model(C=3037, M=50, A=4, seed=5):
    import dataclasses
    from gnomix_amd import synth
    d = synth.synthetic_model(C=C, M=M, A=A, S=11, n_rounds=4, seed=seed)
    return dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                               population_order=["P%d" % a for a in range(d.A)], gen_map_pos=np.array([1, 50_000, 200_000]),
                               gen_map_cm=np.array([0.0, 1.5, 9.25]))


def _eq(got, want, where=""):
    for g, w, name in zip(got, want, ("DD", "DO", "OO")):
        g = g.cpu().numpy() if hasattr(g, "is_cuda") else g
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, where)


def test_model_surface_follows_predict(ga):
    import torch
    from gnomix_amd import synth
    d = _model()
    X = synth.synthetic_X(70, d.C, seed=3, miss=0.03)
    for mf in (0, 5):
        g = ga.HipGnomix(d, device=0, mode_filter=mf)
        lab = np.ascontiguousarray(g.predict(X), dtype=np.int32)
        a = int(np.bincount(lab.ravel(), minlength=d.A).argmax())
        want = PE.tables(X, lab, d.M, d.A, a)[:3]
        got = g.ancestry_pair_counts(X, a)
        assert type(got).__name__ == "PairCounts" and got.DO.shape == (35, 35)
        _eq(got, want, "HipGnomix, mode_filter %d" % mf)
        got_t = g.ancestry_pair_counts(torch.from_numpy(X).cuda(), a)
        assert got_t.DD.is_cuda and got_t.OO.dtype == torch.int32
        _eq(got_t, want, "CUDA tensor")
    dev = g.dev
    Xt, lt = torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda()
    rng_ = (101, 2900)
    want = PE.tables(X, lab, d.M, d.A, a, *rng_)[:3]
    _eq(dev.ancestry_pair_counts(X, lab, a, rng_), want, "host")
    _eq(dev.ancestry_pair_counts(dev.pack_x(X), lab, a, rng_, packed=True), want, "host, packed")
    for rows_t in (Xt, dev.pack_device(Xt)):
        _eq(dev.ancestry_pair_counts_device(rows_t, lt, a, rng_), want, "device")
    parts = dev.ancestry_pair_counts(X, lab, a, (0, 101)) + dev.ancestry_pair_counts(X, lab, a, rng_) + dev.ancestry_pair_counts(X, lab, a, (2900, d.C))
    _eq(parts, PE.tables(X, lab, d.M, d.A, a)[:3], "PairCounts.__add__ over a partition")
    dev.ctx.reset_stream()


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
    C_, M, A, n_ind = 4112, 100, 3, 67                      # 134 haplotypes: two macro-tiles of individuals
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
    for rng_ in (None, (77, 3990)):
        c0, c1 = rng_ or (0, C_)
        want = PE.tables(Xq, lab, M, A, a, c0, c1)[:3]
        assert want[2].sum() > 0
        _eq(dev.ancestry_pair_counts(Xq, lab, a, rng_), want, "matrix path")
        _eq(dev.ancestry_pair_counts_gt2(vcf.gt2, N, src, lab, a, rng_), want, "one batch")
    want = PE.tables(Xq, lab, M, A, a)[:3]
    # the library reads GNX_HOST_BATCH once per CONTEXT (gnx_init): two other batch sizes, each set for a fresh context's call alone
    for batch in ("40", "4"):
        monkeypatch.setenv("GNX_HOST_BATCH", batch)
        ctx2 = _lib.Context(0)
        monkeypatch.delenv("GNX_HOST_BATCH")
        dev2 = ga.DeviceModel(d, ctx=ctx2)
        _eq(dev2.ancestry_pair_counts_gt2(np.array(vcf.gt2), N, src, lab, a), want, "GNX_HOST_BATCH=" + batch)
        ctx2.close()
    bad = lab.copy()
    bad[3, 5] = A
    with pytest.raises(_lib.GnxError, match="1 labels lie outside"):
        dev.ancestry_pair_counts_gt2(vcf.gt2, N, src, bad, a)
    with pytest.raises(_lib.GnxError, match="ancestry outside"):
        dev.ancestry_pair_counts_gt2(vcf.gt2, N, src, lab, A)
    worse = src.copy()
    worse[0] = vcf.gt2.shape[0]
    with pytest.raises(_lib.GnxError, match="column map entry"):
        dev.ancestry_pair_counts_gt2(vcf.gt2, N, worse, lab, a)


def test_command_line_writes_asmds_only_when_asked(ga, tmp_path):
    from gnomix_amd import asmds, synth, vcfio, cli
    from gnomix_amd import postprocess as pp
    d = _model()
    pops = list(d.population_order)
    X = synth.synthetic_X(60, d.C, seed=3, miss=0.03)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    g = ga.HipGnomix(d, device=0)
    samples = [str(s) for s in vcfio.read_vcf(q, chm="22", ctx=g.dev.ctx)["samples"]]

    def run(name, phase=False, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, **kw)
        return od
    off = run("off")
    on = run("on", ancestry_mds_output=True, ancestry_mds_components=2, ancestry_mds_min_sites=40)
    assert sorted(os.listdir(str(off))) == ["query_results.fb", "query_results.msp"]                 # the key absent: the files as before
    assert sorted(os.listdir(str(on))) == ["query_results.asmds.tsv", "query_results.fb", "query_results.msp"]
    for f in ("query_results.fb", "query_results.msp"):
        assert (off / f).read_bytes() == (on / f).read_bytes()
    rows = [ln.split("\t") for ln in (on / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)           # the labels that went to the .msp
    results = []
    for a in range(d.A):
        t = PE.tables(X, lab, d.M, d.A, a)[:3]
        results.append(asmds.ancestry_mds(asmds.PairCounts(*(v.astype(np.int32) for v in t)), k=2, min_sites=40))
    pp.write_asmds(str(tmp_path / "want"), results, pops, samples)
    text = (on / "query_results.asmds.tsv").read_text()
    assert text == (tmp_path / "want.asmds.tsv").read_text()
    assert any(r is not None for r in results) and text.count("sample\tpopulation") == d.A
    with pytest.raises(ValueError, match="ancestry_mds"):
        run("phased", phase=True, ancestry_mds_output=True)
    assert os.listdir(str(tmp_path / "phased")) == []


def test_ancestry_mds_separates_two_planted_sub_populations(ga):
    """two sub-populations whose allele frequencies differ (0.5 +- 0.35 per SNP, the sign drawn per SNP) are planted at EVERY SNP, so they
    are there inside whichever ancestry predict calls; the embedding of the most-called ancestry must split the two halves on PC1"""
    d = _model(C=3037, M=50, A=3, seed=9)
    X, group = PC.planted(40, d.C, seed=4)
    g = ga.HipGnomix(d, device=0)
    lab = np.ascontiguousarray(g.predict(X), dtype=np.int32)
    a = int(np.bincount(lab.ravel(), minlength=d.A).argmax())
    _eq(g.ancestry_pair_counts(X, a), PE.tables(X, lab, d.M, d.A, a)[:3], "the tables behind the embedding")
    res = g.ancestry_mds(X, a, k=2, min_sites=50)
    assert res is not None and res.coords.shape == (res.kept.size, 2) and res.kept.size >= 20
    pc1, grp = res.coords[:, 0], group[res.kept]
    assert (grp == 0).any() and (grp == 1).any()
    s0, s1 = np.sign(pc1[grp == 0]), np.sign(pc1[grp == 1])
    assert (s0 == s0[0]).all() and (s1 == s1[0]).all() and s0[0] == -s1[0] != 0        # every individual on its own side of zero
