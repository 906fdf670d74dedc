"""gnx_ancestry_allele_counts[_dev / _gt2] and gnx_ancestry_dosage[_dev] (csrc/summary/k_allele_counts.hip) on the MI355X against the
numpy restatement (tests/allele_counts_exact.py): integer tables, np.array_equal throughout.

Shapes.  A workgroup owns a tile of 1024 columns, a lane 16 adjacent ones (one packed 32-bit word); a lane whose 16 columns lie in one
window takes the wide route, any other lane the per-column route; a batch of rows is min(flush_every, 4096 / windows the tile spans).
CASES holds, all tiny: C = 3 (less than one lane's group), C = 1025 (one tile + 1, no multiple of 4), M = 1 and M = 3 (hundreds of
windows in a tile, borders inside a packed byte, batches of 4 and 12 rows), M = 1100 (a window wider than a tile), remainders 2, 40 (> M)
and 100, W = 1, A = 1 and A = 32 (the 96 KiB table), N = 1, odd N, and M = 16 / 20 (lanes on both routes in one wave).
The restatement's tables are computed once per case and shared."""
import ctypes as C
import os

import numpy as np
import pytest

import allele_counts_exact as AE

pytestmark = pytest.mark.gpu

#         N   C     M     W    A
CASES = [(5, 3, 1, 3, 2),
         (7, 1025, 3, 341, 3),
         (9, 1025, 1, 1025, 4),
         (6, 2300, 1100, 2, 2),
         (4, 100, 30, 2, 1),
         (3, 70, 70, 1, 32),
         (1, 50, 16, 3, 3),
         (11, 130, 20, 6, 7),
         (40, 1500, 50, 30, 32)]
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


def _case(N, C, M, W, A):
    """X (N, C) int8 with REF / ALT and the missing bytes 2, -1 and 7; column 1 % C all missing, column 2 % C all ALT; labels in blocks"""
    key = (N, C, M, W, A)
    if key not in _inputs:
        rng = np.random.RandomState(N + 13 * C + 7 * M + A)
        X = rng.choice([0, 1, 2, -1, 7], size=(N, C), p=[0.44, 0.4, 0.06, 0.05, 0.05]).astype(np.int8)
        X[:, 1 % C] = rng.choice([2, -1, 7], size=N)
        X[:, 2 % C] = 1
        lab = np.repeat(rng.randint(0, A, size=(N, W // 3 + 1)), 3, axis=1)[:, :W].astype(np.int32)
        _inputs[key] = (X, np.ascontiguousarray(lab))
    return _inputs[key]


def _expected(N, C, M, W, A):
    key = (N, C, M, W, A)
    if key not in _want:
        X, lab = _case(*key)
        _want[key] = AE.allele_counts(X, lab, M, A)
    return _want[key]


def _codes(X):
    """int8 bytes -> 2-bit codes: 7 becomes 3, every other missing byte 2"""
    return np.where((X == 0) | (X == 1), X, np.where(X == 7, 3, 2)).astype(np.uint8)


def _padded(a, extra, poison):
    out = np.full((a.shape[0], a.shape[1] + extra), poison, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _rows(X, kind, extra):
    """the rows as the entry takes them, `extra` poison bytes behind every row (poison = ALT: counted if ever read)"""
    if kind == 1:
        return AE.pack2(_codes(X), ldp=(X.shape[1] + 3) // 4 + extra, fill=0x55)
    return _padded(X, extra, 1)


def _host_counts(ctx, rows, kind, lab, N, C, M, W, A, rpc=0, fe=0, tables=None):
    t = [np.full((A, C), -7, np.int32) for _ in range(3)] if tables is None else tables
    rc = ctx.lib.gnx_ancestry_allele_counts(ctx.h, rows.ctypes.data, kind, rows.shape[1], lab.ctypes.data, lab.shape[1], N, C, M, W, A,
                                            t[0].ctypes.data, t[1].ctypes.data, t[2].ctypes.data, rpc, fe)
    return rc, t


def _same(got, want):
    for g, w, name in zip(got, want, ("n_obs", "n_alt", "n_miss")):
        assert np.array_equal(np.asarray(g), w), name


# ---------------------------------------------------------------- geometry and codes ----------------------------------------------
@pytest.mark.parametrize("N,C,M,W,A", CASES)
def test_counts_equal_the_restatement_for_both_row_forms(ctx, N, C, M, W, A):
    from gnomix_amd import _lib
    X, lab = _case(N, C, M, W, A)
    want = _expected(N, C, M, W, A)
    assert want[2][:, 1 % C].sum() == N and want[0][:, 1 % C].sum() == 0 and want[1][:, 2 % C].sum() == N       # all missing, all ALT
    assert (_codes(X) == 3).any() or N * C < 30
    for kind in (_lib.GNX_ROWS_INT8, _lib.GNX_ROWS_PACKED2):
        for extra, lextra in ((0, 0), (5, 3)):       # minimal strides; strides with poison behind every row
            rc, got = _host_counts(ctx, _rows(X, kind, extra), kind, _padded(lab, lextra, A), N, C, M, W, A)
            assert rc == _lib.GNX_OK, ctx.lib.gnx_last_error(ctx.h)
            _same(got, want)


def test_packed_codes_2_and_3_and_int8_minus_one_and_seven_are_missing(ctx):
    N, C, M, W, A = 4, 21, 5, 4, 2
    lab = np.zeros((N, W), np.int32)
    lab[2:] = 1
    for kind, missing in ((1, (2, 3)), (0, (-1, 7, 2, -128, 127))):
        for v in missing:
            X = np.zeros((N, C), np.int8)
            X[0, 4], X[3, 20] = 1, 1
            code = X.copy()
            code[1, 7], code[2, 19] = v, v
            rows = AE.pack2(code) if kind == 1 else code
            rc, (obs, alt, miss) = _host_counts(ctx, np.ascontiguousarray(rows), kind, lab, N, C, M, W, A)
            assert rc == 0
            assert miss.sum() == 2 and miss[0, 7] == 1 and miss[1, 19] == 1 and alt.sum() == 2 and alt[0, 4] == 1 and alt[1, 20] == 1
            assert np.array_equal(obs + miss, np.full((A, C), 2))


def test_no_rows_zeroes_the_tables(ctx):
    rows, lab = np.zeros((1, 8), np.int8), np.zeros((1, 2), np.int32)
    rc, got = _host_counts(ctx, rows, 0, lab, 0, 8, 4, 2, 3)
    assert rc == 0 and all((t == 0).all() and t.shape == (3, 8) for t in got)


# ---------------------------------------------------------------- accumulation -----------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_chunks_flushes_and_repeated_calls_give_the_same_tables(ctx, kind):
    N, C, M, W, A = 10, 1025, 3, 341, 3
    rng = np.random.RandomState(5)
    X = rng.choice([0, 1, 2], size=(N, C), p=[0.5, 0.4, 0.1]).astype(np.int8)
    lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
    want = AE.allele_counts(X, lab, M, A)
    rows = _rows(X, kind, 0)
    rc, base = _host_counts(ctx, rows, kind, lab, N, C, M, W, A)
    assert rc == 0
    _same(base, want)
    rc, again = _host_counts(ctx, rows, kind, lab, N, C, M, W, A, tables=base)      # overwritten, not accumulated
    assert rc == 0
    _same(again, want)
    for rpc, fe in ((4, 0), (0, 3), (4, 3), (1, 1)):       # rpc = 4: three workgroups per column tile, the last one with two rows
        rc, got = _host_counts(ctx, rows, kind, lab, N, C, M, W, A, rpc=rpc, fe=fe)
        assert rc == 0, (rpc, fe)
        _same(got, want)


def test_more_rows_than_a_byte_counter_takes(ctx):
    """600 rows of one ancestry in one chunk: the 8-bit counters are flushed at 255 rows at the latest"""
    N, C, M, W, A = 600, 40, 20, 2, 2
    X = np.ones((N, C), np.int8)
    X[:, 3] = 2
    lab = np.zeros((N, W), np.int32)
    for kind in (0, 1):
        rc, (obs, alt, miss) = _host_counts(ctx, _rows(X, kind, 0), kind, lab, N, C, M, W, A, rpc=N)
        assert rc == 0 and (alt[0, [0, 1, 2] + list(range(4, C))] == N).all() and miss[0, 3] == N and obs[0, 3] == 0 and (obs[1] == 0).all()


# ---------------------------------------------------------------- refusals ----------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx):
    from gnomix_amd import _lib
    N, C, M, W, A = 4, 20, 5, 4, 3
    X, lab = np.zeros((N, C), np.int8), np.zeros((N, W), np.int32)
    lib, h = ctx.lib, ctx.h
    t = [np.full((33, C), -7, np.int32) for _ in range(3)]
    d = [np.full((N // 2, C), 9, np.uint8) for _ in range(2)]

    def counts(rows=X, kind=0, ld=C, ldl=W, N=N, C=C, M=M, W=W, A=A):
        return lib.gnx_ancestry_allele_counts(h, rows.ctypes.data, kind, ld, lab.ctypes.data, ldl, N, C, M, W, A, t[0].ctypes.data,
                                              t[1].ctypes.data, t[2].ctypes.data, 0, 0)

    def dosage(N=N, M=M, W=W, A=A, anc=0, ld=C, ldd=C):
        return lib.gnx_ancestry_dosage(h, X.ctypes.data, 0, ld, lab.ctypes.data, W, N, C, M, W, A, anc, d[0].ctypes.data, ldd, d[1].ctypes.data, C)
    assert counts(A=33) == _lib.GNX_EUNSUPPORTED and b"33" in lib.gnx_last_error(h)
    assert counts(M=6) == _lib.GNX_EINVAL            # M W > C
    assert counts(M=0) == _lib.GNX_EINVAL
    assert counts(W=0) == _lib.GNX_EINVAL
    assert counts(ld=C - 1) == _lib.GNX_EINVAL
    assert counts(kind=1, ld=(C + 3) // 4 - 1) == _lib.GNX_EINVAL
    assert counts(ldl=W - 1) == _lib.GNX_EINVAL
    assert counts(kind=2) == _lib.GNX_EINVAL
    assert dosage(N=3) == _lib.GNX_EINVAL            # odd N
    assert dosage(anc=A) == _lib.GNX_EINVAL and dosage(anc=-1) == _lib.GNX_EINVAL
    assert dosage(A=33) == _lib.GNX_EUNSUPPORTED
    assert dosage(M=6) == _lib.GNX_EINVAL and dosage(M=0) == _lib.GNX_EINVAL and dosage(ld=C - 1) == _lib.GNX_EINVAL
    assert dosage(ldd=C - 1) == _lib.GNX_EINVAL
    assert all((x == -7).all() for x in t) and all((x == 9).all() for x in d)
    assert counts() == 0 and dosage() == 0


@pytest.mark.parametrize("kind", [0, 1])
def test_labels_out_of_range_are_reported_after_the_launch(ctx, kind):
    """well-formed memory, malformed values: such a label is compared, never used as an index; it counts for no ancestry"""
    from gnomix_amd import _lib
    N, C, M, W, A = 8, 1100, 7, 150, 3
    X, lab = _case(N, C, M, W, A)
    lab = lab.copy()
    lab[1, 17], lab[4, 149], lab[6, 146] = A, -1, 200         # window 146 starts at column 1022 and crosses the tile border
    want = AE.allele_counts(X, lab, M, A)
    clean = _expected(N, C, M, W, A)
    assert not np.array_equal(want[0], clean[0])
    rc, got = _host_counts(ctx, _rows(X, kind, 0), kind, lab, N, C, M, W, A)
    assert rc == _lib.GNX_EINVAL and b"3 labels lie outside [0, 3)" in ctx.lib.gnx_last_error(ctx.h)
    _same(got, want)
    dos = [np.zeros((N // 2, C), np.uint8) for _ in range(2)]
    rows = _rows(X, kind, 0)
    rc = ctx.lib.gnx_ancestry_dosage(ctx.h, rows.ctypes.data, kind, rows.shape[1], lab.ctypes.data, W, N, C, M, W, A, 1, dos[0].ctypes.data, C,
                                     dos[1].ctypes.data, C)
    assert rc == _lib.GNX_EINVAL and b"3 labels lie outside [0, 3)" in ctx.lib.gnx_last_error(ctx.h)
    wd, wh = AE.dosage(X, lab, M, A, 1)
    assert np.array_equal(dos[0], wd) and np.array_equal(dos[1], wh)


# ---------------------------------------------------------------- dosage ---------------------------------------------------------------
@pytest.mark.parametrize("N,C,M,W,A", CASES)
def test_dosage_equals_the_restatement_and_sums_to_the_device_counts(ctx, N, C, M, W, A):
    from gnomix_amd import postprocess as pp
    X, lab = _case(N, C, M, W, A)
    n = N // 2 * 2
    if n == 0:
        X, lab, n = np.concatenate([X, X]), np.concatenate([lab, lab]), 2       # (N = 1: the row twice is one individual)
    X, lab = np.ascontiguousarray(X[:n]), np.ascontiguousarray(lab[:n])
    counts = pp.allele_counts(ctx, X, lab, M, A)
    P = AE.pack2(_codes(X))
    for a in sorted({0, A // 2, A - 1}):
        wd, wh = AE.dosage(X, lab, M, A, a)
        dos, hap = pp.ancestry_dosage(ctx, X, lab, M, A, a)
        assert dos.dtype == hap.dtype == np.uint8 and np.array_equal(dos, wd) and np.array_equal(hap, wh)
        dp, hp = pp.ancestry_dosage(ctx, P, lab, M, A, a, packed=True, C=C)
        assert np.array_equal(dp, wd) and np.array_equal(hp, wh)
        assert np.array_equal(dos.sum(axis=0), counts.n_alt[a]) and np.array_equal(hap.sum(axis=0), counts.n_obs[a] + counts.n_miss[a])
    # strided outputs keep the bytes between the rows
    d, h_ = np.full((n // 2, C + 4), 9, np.uint8), np.full((n // 2, C + 2), 9, np.uint8)
    assert ctx.lib.gnx_ancestry_dosage(ctx.h, X.ctypes.data, 0, C, lab.ctypes.data, W, n, C, M, W, A, 0, d.ctypes.data, C + 4, h_.ctypes.data, C + 2) == 0
    wd, wh = AE.dosage(X, lab, M, A, 0)
    assert np.array_equal(d[:, :C], wd) and np.array_equal(h_[:, :C], wh) and (d[:, C:] == 9).all() and (h_[:, C:] == 9).all()


# ---------------------------------------------------------------- through the model ---------------------------------------------
@pytest.fixture(scope="module")
def model(ga):
    """a logistic base with a tree smoother (as tests/test_gpu_labels.py and tests/test_gpu_summary.py build it)"""
    from gnomix_amd import synth
    d = synth.synthetic_model(C=3037, M=50, A=4, S=11, n_rounds=4, seed=5)
    X = synth.synthetic_X(26, d.C, seed=3, miss=0.03)
    return d, X


def test_allele_frequencies_follow_predict_and_device_forms_equal_host_forms(ga, model):
    import torch
    d, X = model
    for mf in (0, 5):
        g = ga.HipGnomix(d, device=0, mode_filter=mf)
        lab = g.predict(X)
        want = AE.allele_counts(X, lab, d.M, d.A)
        assert want[2].sum() > 0
        got = g.allele_frequencies(X)
        assert type(got).__name__ == "AlleleCounts" and got.n_obs.dtype == np.int32 and got.n_obs.shape == (d.A, d.C)
        _same(got, want)
        f = got.freq()
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = np.where(want[0] > 0, want[1] / want[0].astype(np.float64), np.nan)
        assert np.array_equal(f, ref, equal_nan=True)
        got_t = g.allele_frequencies(torch.from_numpy(X).cuda())
        assert got_t.n_obs.is_cuda and got_t.n_obs.dtype == torch.int32
        _same([t.cpu().numpy() for t in got_t], want)
        assert np.array_equal(got_t.freq(), ref, equal_nan=True)
    dev = g.dev
    lab32 = np.ascontiguousarray(lab, dtype=np.int32)
    Xt = torch.from_numpy(X).cuda()
    wide = torch.full((X.shape[0], d.W + 3), d.A, dtype=torch.int32, device="cuda")       # labels with a row stride of their own
    wide[:, :d.W] = torch.from_numpy(lab32).cuda()
    lt = wide[:, :d.W]
    host = dev.ancestry_allele_counts(X, lab32)
    _same(host, want)
    _same(dev.ancestry_allele_counts(dev.pack_x(X.clip(0, 2)), lab32, packed=True), want)
    for rows_t in (Xt, dev.pack_device(Xt)):
        _same([t.cpu().numpy() for t in dev.ancestry_allele_counts_device(rows_t, lt)], want)
        for a in (0, d.A - 1):
            wd, wh = dev.ancestry_dosage(X, lab32, a)
            assert np.array_equal(wd, AE.dosage(X, lab32, d.M, d.A, a)[0])
            dt, ht = dev.ancestry_dosage_device(rows_t, lt, a)
            assert dt.is_cuda and dt.dtype == torch.uint8 and np.array_equal(dt.cpu().numpy(), wd) and np.array_equal(ht.cpu().numpy(), wh)
    dev.ctx.reset_stream()


# ---------------------------------------------------------------- the file path ------------------------------------------------
def _x_from(code, src):
    """numpy statement of vcf_to_npy's fill / flip / missing rule (src/utils.py:125-151), as tests/test_gpu_vcf.py states it"""
    N = code.shape[1]
    X = np.full((N, len(src)), 2, np.int8)
    have = src >= 0
    v, flip = src[have] & 0x3FFFFFFF, (src[have] >> 30) & 1
    c = code[v].T.astype(np.int8)
    X[:, have] = np.where(c >= 2, 2, np.where(flip[None, :] == 1, 1 - c, c))
    return X


def _query(tmp_path, d, n_ind, rng, drop=200, flip_frac=0.05, miss=0.02):
    """SNP metadata for the model + a query VCF that lacks `drop` model SNPs, has SNPs of its own, REF mismatches and missing calls"""
    from gnomix_amd import synth, vcfio
    d.snp_pos = np.sort(rng.choice(np.arange(10_000, 9_000_000), size=d.C, replace=False))
    d.snp_ref = rng.choice(list("ACGT"), size=d.C)
    d.snp_alt = rng.choice(list("ACGT"), size=d.C)
    keep = np.sort(rng.choice(d.C, size=d.C - drop, replace=False))
    extra = np.setdiff1d(rng.choice(np.arange(10_000, 9_000_000), size=300), d.snp_pos)
    qpos = np.concatenate([d.snp_pos[keep], extra])
    qref = np.concatenate([d.snp_ref[keep], rng.choice(list("ACGT"), len(extra))])
    fl = rng.random(len(keep)) < flip_frac
    qref[:len(keep)][fl] = np.where(qref[:len(keep)][fl] == "A", "C", "A")
    order = np.argsort(qpos)
    Xq = synth.synthetic_X(2 * n_ind, len(qpos), seed=int(rng.integers(1 << 30)), miss=miss)
    return synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(Xq[:, order]), n_ind, qpos[order], qref[order], ["N"] * len(qpos), chrom="22")


def test_allele_counts_gt2_equals_the_counts_of_the_vcf_to_npy_matrix(ga, tmp_path, monkeypatch):
    from gnomix_amd import synth, vcfio, _lib
    from gnomix_amd.multi import DeviceGroup
    C_, M, A, n_ind = 4112, 100, 4, 17
    rng = np.random.default_rng(C_)
    d = synth.synthetic_model(C=C_, M=M, A=A, S=11, n_rounds=4, seed=C_)
    p = _query(tmp_path, d, n_ind, rng)
    dev = ga.DeviceModel(d)
    vcf = vcfio.read_vcf(p, chm="22", ctx=dev.ctx)
    src, _, _ = vcfio.column_map(vcf, d.snp_pos, d.snp_ref, verbose=False)
    N = 2 * n_ind
    assert (src >> 30 == 1).any() and (src == -1).any()                         # a REF-flipped SNP, a model SNP the query lacks
    G = np.array(vcf.gt2)
    code = np.stack([(G[:, np.arange(N) // 4] >> (2 * (np.arange(N) % 4)).astype(np.uint8)) & 3])[0]
    X = _x_from(code, src)
    assert np.array_equal(X, vcfio.vcf_to_npy(vcf, d.snp_pos, d.snp_ref, verbose=False)) and (X[:, src >= 0] == 2).any()
    _, lab = dev.infer_gt2(vcf.gt2, N, src, want_proba=False)
    want = AE.allele_counts(X, lab, M, A)
    absent = np.flatnonzero(src == -1)
    assert (want[0][:, absent] == 0).all() and (want[2][:, absent].sum(axis=0) == N).all()
    _same(dev.allele_counts_gt2(vcf.gt2, N, src, lab), want)
    # several haplotype batches, pageable genotype rows
    monkeypatch.setenv("GNX_HOST_BATCH", "12")
    ctx2 = _lib.Context(0)
    dev2 = ga.DeviceModel(d, ctx=ctx2)
    _same(dev2.allele_counts_gt2(G, N, src, lab), want)
    ctx2.close()
    monkeypatch.delenv("GNX_HOST_BATCH")
    # two contexts on one GPU: each counts its own individuals, the tables add up to one context's
    with DeviceGroup(d, [0, 0], first=dev) as grp:
        assert len(grp.models) == 2
        _same(grp.allele_counts_gt2(vcf.gt2, N, src, lab), want)
    bad = lab.copy()
    bad[3, 5] = A
    with pytest.raises(_lib.GnxError, match="1 labels lie outside"):
        dev.allele_counts_gt2(vcf.gt2, N, src, bad)


def test_command_line_writes_afreq_only_when_asked(ga, model, tmp_path):
    import dataclasses
    from gnomix_amd import synth, vcfio, cli
    from gnomix_amd.multi import DeviceGroup
    d, X = model
    pops = ["P%d" % a for a in range(d.A)]
    d = dataclasses.replace(d, snp_pos=1000 + 37 * np.arange(d.C), snp_ref=np.array(["A"] * d.C), snp_alt=np.array(["C"] * d.C),
                            population_order=pops, gen_map_pos=np.array([1, 50_000, 200_000]), gen_map_cm=np.array([0.0, 1.5, 9.25]))
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), X.shape[0] // 2, d.snp_pos, d.snp_ref, ["C"] * d.C)
    g = ga.HipGnomix(d, device=0)

    def run(name, phase=False, devices=None, **kw):
        od = tmp_path / name
        od.mkdir()
        cli.run_inference({"query_file": q, "chm": "22", "output_basename": str(od), "phase": phase}, g, verbose=False, devices=devices, **kw)
        return od
    off, on = run("off"), run("on", ancestry_allele_freq_output=True)
    assert sorted(os.listdir(str(off))) == ["query_results.fb", "query_results.msp"]
    assert sorted(os.listdir(str(on))) == ["query_results.afreq.tsv", "query_results.fb", "query_results.msp"]
    for f in ("query_results.fb", "query_results.msp"):
        assert (off / f).read_bytes() == (on / f).read_bytes()
    rows = [ln.split("\t") for ln in (on / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)           # the labels that went to the .msp
    obs, alt, _ = AE.allele_counts(X, lab, d.M, d.A)
    want = AE.afreq_text("22", d.snp_pos, d.M, d.W, obs, alt, pops)
    text = (on / "query_results.afreq.tsv").read_text()
    assert text == want and len(text.splitlines()) == 1 + d.C and "\tnan" in text
    with pytest.raises(ValueError, match="allele_frequencies"):
        run("phased", phase=True, ancestry_allele_freq_output=True)
    assert os.listdir(str(tmp_path / "phased")) == []
    with DeviceGroup(d, [0, 0], first=g.dev) as grp:
        two = run("two", devices=grp, ancestry_allele_freq_output=True)
    assert (two / "query_results.afreq.tsv").read_text() == want


def test_cli_main_reads_the_config_key(ga, tmp_path, monkeypatch):
    """cli.main in pre-trained mode with ./config.yaml switching the key on: the file equals write_afreq of the restatement's tables for
    the labels in the .msp; with phase=True the ValueError comes before any output"""
    from gnomix_amd import synth, vcfio, cli
    from gnomix_amd import postprocess as pp
    d = synth.synthetic_model(C=2037, M=50, A=3, S=11, n_rounds=4, seed=9)
    d.snp_pos = 1000 + 37 * np.arange(d.C)
    d.snp_ref, d.snp_alt = np.array(["A"] * d.C), np.array(["C"] * d.C)
    d.gen_map_pos, d.gen_map_cm = np.array([1, 400_000]), np.array([0.0, 1.3])
    mp = str(tmp_path / "model.gnx")
    d.save(mp)
    X = synth.synthetic_X(8, d.C, seed=1, miss=0.02)
    q = synth.write_vcf_gt2(str(tmp_path / "q.vcf"), vcfio.pack_gt2(X), 4, d.snp_pos, d.snp_ref, d.snp_alt, chrom="22")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("GNX_DEVICES", "0")
    (tmp_path / "config.yaml").write_text("inference:\n  ancestry_allele_freq_output: True\n")
    out = tmp_path / "out"
    assert cli.main(["gnomix.py", q, str(out), "22", "False", mp]) == 0
    rows = [ln.split("\t") for ln in (out / "query_results.msp").read_text().splitlines()[2:]]
    lab = np.ascontiguousarray(np.array([[int(v) for v in r[6:]] for r in rows], np.int32).T)
    pops = (out / "query_results.afreq.tsv").read_text().splitlines()[0].split("\t")[3::3]
    pops = [p[:-len(".n_obs")] for p in pops]
    assert len(pops) == d.A
    want = pp.AlleleCounts(*AE.allele_counts(X, lab, d.M, d.A))
    pp.write_afreq(str(tmp_path / "want"), "22", d.snp_pos, d.M, d.W, want, pops)
    assert (out / "query_results.afreq.tsv").read_bytes() == (tmp_path / "want.afreq.tsv").read_bytes()
    with pytest.raises(ValueError, match="allele_frequencies"):
        cli.main(["gnomix.py", q, str(tmp_path / "phased"), "22", "True", mp])
    assert os.listdir(str(tmp_path / "phased")) == []
    (tmp_path / "config.yaml").write_text("inference:\n  bed_file_output: False\n")
    assert cli.main(["gnomix.py", q, str(tmp_path / "off"), "22", "False", mp]) == 0
    assert "query_results.afreq.tsv" not in os.listdir(str(tmp_path / "off"))
