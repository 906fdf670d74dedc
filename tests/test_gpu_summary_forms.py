"""What the six ancestry-specific ops of csrc/summary/ share on the host side (gnx_summary_host.h), pinned across all of them at once: the
refusals on the geometry, on the file path's arguments and on the column map, with their literal messages, and the verdict on a label
outside [0, A) (count, the op's own sentence, n_bad, outputs handed over all the same).

One tiny case: 8 haplotypes, C = 37 (ragged last packed byte, a tail in the 16-column groups), M = 9, W = 4 (the last window is longer
than M), A = 3, int8 rows with a stride of C + 7, 2-bit rows with a stride of ceil(C / 4) + 3 (kind=1: the forms that take a row_kind),
labels with a stride of W + 3.  The file path's forms run on a model of that geometry in a context with GNX_HOST_BATCH=4: two batches."""
import ctypes
import os

import numpy as np
import pytest

import allele_counts_exact as AE

pytestmark = pytest.mark.gpu

N, C, M, W, A, K, S = 8, 37, 9, 4, 3, 2, 2
BAND = 5                                        # of the LD tables: the bands of the last four SNPs reach past C (no owner, zeroed first)
LD, LDP, LDL = C + 7, (C + 3) // 4 + 3, W + 3
POISON = -7
NI = A * (A + 1) // 2 + A * (A - 1) + A + 1     # int32 words of one SNP's block of the linear statistics

TAIL_COUNTS = "such a label counts for no ancestry"
TAIL_ASSOC = "an individual with such a label takes no part at that window"
TAIL_HAP = "such a haplotype counts for no ancestry at that window"
NULL_ASSOC = "a null pointer (only use and n_bad may be NULL)"
NULL_LOGIT = "a null pointer (only use, theta and n_bad may be NULL)"
NULL_ROWS = "no rows or no labels"

# form -> (C entry point, the name its geometry refusals carry, the tail of the label verdict, the null-rows message, needs an even N)
FORMS = {
    "counts": ("gnx_ancestry_allele_counts", "ancestry_allele_counts", TAIL_COUNTS, NULL_ROWS, False),
    "counts_dev": ("gnx_ancestry_allele_counts_dev", "ancestry_allele_counts", TAIL_COUNTS, NULL_ROWS, False),
    "counts_gt2": ("gnx_ancestry_allele_counts_gt2", "ancestry_allele_counts_gt2", TAIL_COUNTS, None, False),
    "dosage": ("gnx_ancestry_dosage", "ancestry_dosage", TAIL_COUNTS, NULL_ROWS, True),
    "dosage_dev": ("gnx_ancestry_dosage_dev", "ancestry_dosage", TAIL_COUNTS, NULL_ROWS, True),
    "assoc": ("gnx_ancestry_assoc_stats", "ancestry_assoc_stats", TAIL_ASSOC, NULL_ASSOC, True),
    "assoc_dev": ("gnx_ancestry_assoc_stats_dev", "ancestry_assoc_stats", TAIL_ASSOC, NULL_ASSOC, True),
    "assoc_gt2": ("gnx_ancestry_assoc_stats_gt2", "ancestry_assoc_stats", TAIL_ASSOC, None, True),
    "logit": ("gnx_ancestry_assoc_logit", "ancestry_assoc_logit", TAIL_ASSOC, NULL_LOGIT, True),
    "logit_dev": ("gnx_ancestry_assoc_logit_dev", "ancestry_assoc_logit", TAIL_ASSOC, NULL_LOGIT, True),
    "logit_gt2": ("gnx_ancestry_assoc_logit_gt2", "ancestry_assoc_logit", TAIL_ASSOC, None, True),
    "score": ("gnx_ancestry_score", "ancestry_score", TAIL_HAP, NULL_ROWS, True),
    "score_dev": ("gnx_ancestry_score_dev", "ancestry_score", TAIL_HAP, NULL_ROWS, True),
    "score_gt2": ("gnx_ancestry_score_gt2", "ancestry_score_gt2", TAIL_HAP, None, True),
    "pairs": ("gnx_ancestry_pair_counts", "ancestry_pair_counts", TAIL_HAP, NULL_ROWS, True),
    "pairs_dev": ("gnx_ancestry_pair_counts_dev", "ancestry_pair_counts", TAIL_HAP, NULL_ROWS, True),
    "pairs_gt2": ("gnx_ancestry_pair_counts_gt2", "ancestry_pair_counts_gt2", TAIL_HAP, None, True),
    "ld": ("gnx_ancestry_ld_counts", "ancestry_ld_counts", TAIL_HAP, NULL_ROWS, False),
    "ld_dev": ("gnx_ancestry_ld_counts_dev", "ancestry_ld_counts", TAIL_HAP, NULL_ROWS, False),
    "ld_gt2": ("gnx_ancestry_ld_counts_gt2", "ancestry_ld_counts_gt2", TAIL_HAP, None, False),
}
HAS_ROW_KIND = {f for f in FORMS if not f.endswith("gt2") and f not in ("assoc", "logit")}
HAS_N_BAD = {f for f in FORMS if not f.startswith(("counts", "dosage"))}


@pytest.fixture(scope="module")
def env():
    """the case, a context with GNX_HOST_BATCH=4 (read once per context) and a model of the case's geometry in it"""
    import gnomix_amd
    from gnomix_amd import _lib, synth, vcfio
    gnomix_amd.load_library()
    old = os.environ.get("GNX_HOST_BATCH")
    os.environ["GNX_HOST_BATCH"] = "4"
    try:
        ctx = _lib.Context(0)
    finally:
        if old is None:
            del os.environ["GNX_HOST_BATCH"]
        else:
            os.environ["GNX_HOST_BATCH"] = old
    d = synth.synthetic_model(C=C, M=M, A=A, S=1, n_rounds=2, seed=C)    # (the smoother needs W >= 2 S)
    assert (d.C, d.M, d.W, d.A) == (C, M, W, A)
    dev = gnomix_amd.DeviceModel(d, ctx=ctx)
    rng = np.random.default_rng(C)
    X = synth.synthetic_X(N, C, seed=5, miss=0.1).astype(np.int8)
    lab = rng.integers(0, A, size=(N, W)).astype(np.int32)
    e = dict(ctx=ctx, dev=dev, lib=ctx.lib, X=X, lab=lab, G=np.ascontiguousarray(vcfio.pack_gt2(X)), src=np.arange(C, dtype=np.int32),
             y=np.array([0.0, 1.0, 1.0, 0.0]), Z=np.ascontiguousarray(np.stack([np.ones(N // 2), rng.normal(size=N // 2)], axis=1)),
             w=rng.normal(size=(C, A, S)), eff=rng.integers(0, 2, size=C).astype(np.uint8))
    assert e["G"].shape[0] == C and e["G"].shape[1] > (N + 3) // 4     # padded rows: the strided upload of G
    yield e
    ctx.close()


def _outputs(form):
    """the form's outputs, poisoned: name -> array"""
    op = form.split("_")[0]
    n = N // 2
    if op == "counts":
        shapes = {k: ((A, C), np.int32) for k in ("n_obs", "n_alt", "n_miss")}
    elif op == "dosage":
        shapes = {k: ((n, C), np.uint8) for k in ("dosage", "hapcount")}
    elif op == "assoc":
        shapes = {"sf": ((C, A * (K + 1)), np.float64), "si": ((C, NI), np.int32), "wf": ((W, (K + A) ** 2), np.float64), "wi": ((W, 1 + A), np.int32)}
    elif op == "logit":
        shapes = {"sf": ((C, 2 * A + 1), np.float64), "si": ((C, 2 * A + 3), np.int32), "th": ((C, K + 2 * A - 1), np.float64),
                  "wf": ((W, K + A), np.float64), "wi": ((W, A + 4), np.int32)}
    elif op == "score":
        shapes = {"score": ((n, A, S), np.float64), "ne": ((n, A), np.int32), "ns": ((n, A), np.int32), "nm": ((n, A), np.int32)}
    elif op == "ld":
        shapes = {k: ((C, BAND), np.int32) for k in ("n11", "n1o", "no1", "noo")}
    else:
        shapes = {k: ((n, n), np.int32) for k in ("DD", "DO", "OO")}
    return {k: np.full(s, _poison(t), t) for k, (s, t) in shapes.items()}


def _poison(dtype):
    return POISON % 256 if np.dtype(dtype) == np.uint8 else POISON


def _call(e, form, lab=None, **v):
    """one call of the form with the case's arguments, `v` overriding the scalar ones -> rc, message, n_bad (None: the form has none), outputs"""
    import torch
    lib, op, kind = e["lib"], form.split("_")[0], form.split("_")[-1]
    lab = e["lab"] if lab is None else lab
    packed = v.get("kind") == 1                  # 2-bit rows (X holds the codes 0, 1, 2), poison bytes behind every row
    rows = AE.pack2(e["X"], ldp=LDP, fill=0x55) if packed else np.full((N, LD), 1, np.int8)
    if not packed:
        rows[:, :C] = e["X"]
    wide = np.full((N, LDL), 0, np.int32)
    wide[:, :W] = lab
    out = _outputs(form)
    ins = dict(rows=rows, wide=wide, y=e["y"], Z=e["Z"], w=e["w"], eff=e["eff"])
    keep = []                                    # device tensors stay alive until the call returns
    if kind == "dev":
        def ptr(a):
            keep.append(torch.from_numpy(a).cuda())
            return keep[-1].data_ptr()
        dout = {k: torch.from_numpy(a).cuda() for k, a in out.items()}
        o = {k: t.data_ptr() for k, t in dout.items()}
    else:
        def ptr(a):
            return a.ctypes.data
        o = {k: a.ctypes.data for k, a in out.items()}
    p = {k: ptr(a) for k, a in ins.items()}
    g = dict(kind=0, ld=LDP if packed else LD, ldl=LDL, N=N, C=C, M=M, W=W, A=A, rows=p["rows"], V=C, ldg=e["G"].shape[1], src=e["src"].ctypes.data, G=e["G"].ctypes.data)
    g.update(v)
    n_bad = ctypes.c_int64(-5)
    nb = ctypes.byref(n_bad)
    if kind == "gt2":
        head = (e["dev"].h, g["G"], g["V"], g["ldg"], g["N"], g["src"], lab.ctypes.data)
    elif form in ("assoc", "logit"):
        head = (e["ctx"].h, g["rows"], g["ld"], p["wide"], g["ldl"], g["N"], g["C"], g["M"], g["W"], g["A"])
    else:
        head = (e["ctx"].h, g["rows"], g["kind"], g["ld"], p["wide"], g["ldl"], g["N"], g["C"], g["M"], g["W"], g["A"])
    if op == "counts":
        tail = (o["n_obs"], o["n_alt"], o["n_miss"]) + (() if kind == "gt2" else (0, 0))
    elif op == "dosage":
        tail = (1, o["dosage"], C, o["hapcount"], C)
    elif op == "assoc":
        tail = (p["y"], p["Z"], K, None, 1, 0, C, o["sf"], o["si"], o["wf"], o["wi"], nb)
    elif op == "logit":
        tail = (p["y"], p["Z"], K, None, 1, 0, C, 1e-8, 5, o["sf"], o["si"], o["th"], o["wf"], o["wi"], nb)
    elif op == "score":
        tail = (p["w"], S, p["eff"], o["score"], o["ne"], o["ns"], o["nm"]) + (() if kind == "gt2" else (0, 0)) + (nb,)
    elif op == "ld":
        tail = (1, 0, C, BAND, o["n11"], o["n1o"], o["no1"], o["noo"], BAND) + (() if kind == "gt2" else (0,)) + (nb,)
    else:
        tail = (1, 0, C, o["DD"], o["DO"], o["OO"], N // 2) + (() if kind == "gt2" else (0,)) + (nb,)
    rc = getattr(lib, FORMS[form][0])(*head, *tail)
    msg = lib.gnx_last_error(e["ctx"].h).decode()
    if kind == "dev":
        torch.cuda.synchronize()
        out = {k: t.cpu().numpy() for k, t in dout.items()}
    return rc, msg, (n_bad.value if form in HAS_N_BAD else None), out


def _refused(e, form, message, code=None, **v):
    from gnomix_amd import _lib
    rc, msg, _, out = _call(e, form, **v)
    assert rc == (_lib.GNX_EINVAL if code is None else code) and msg == message, (form, v, rc, msg)
    for k, a in out.items():
        assert (a == _poison(a.dtype)).all(), (form, v, k)     # a refusal writes no output


@pytest.mark.parametrize("form", sorted(FORMS))
def test_refusals_carry_the_literal_messages(env, form):
    _, who, _, null_msg, even = FORMS[form]
    if form.endswith("gt2"):
        # the file path's own arguments, then the column map
        name = FORMS[form][0][4:]
        bad_args = name + ": bad G / V / ldg / N / src" + (" / labels" if form == "counts_gt2" else "")
        _refused(env, form, bad_args, ldg=(N + 3) // 4 - 1)
        _refused(env, form, bad_args, src=None)
        worse = env["src"].copy()
        worse[C - 1] = C                         # one past the last variant row
        _refused(env, form, name + ": column map entry outside the variant rows", src=worse.ctypes.data)
        if even:
            _refused(env, form, who + ": N must be even (an individual has two haplotype rows)", N=N - 1)
        return
    if form in HAS_ROW_KIND:
        _refused(env, form, who + ": row_kind is GNX_ROWS_INT8 or GNX_ROWS_PACKED2", kind=2)
        _refused(env, form, who + ": the rows' stride is smaller than a row (C bytes, or ceil(C / 4) packed)", kind=1, ld=(C + 3) // 4 - 1)
    if even:
        _refused(env, form, who + ": N must be even (an individual has two haplotype rows)", N=N - 1)
    _refused(env, form, who + ": need M >= 1, W >= 1 and M * W <= C", M=M + 1)
    _refused(env, form, who + ": the rows' stride is smaller than a row (C bytes, or ceil(C / 4) packed)", ld=C - 1)
    _refused(env, form, who + ": the labels' row stride is smaller than W", ldl=W - 1)
    _refused(env, form, who + ": " + null_msg, rows=None)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_one_label_out_of_range_is_counted_and_the_outputs_are_handed_over(env, form):
    from gnomix_amd import _lib
    name, _, tail, _, _ = FORMS[form]
    who = name[4:-4] if form.endswith("_dev") else name[4:]
    bad = env["lab"].copy()
    bad[5, 2] = A
    for v in ({}, {"kind": 1}) if form in HAS_ROW_KIND else ({},):
        rc, msg, n_bad, good = _call(env, form, **v)
        assert rc == _lib.GNX_OK and n_bad in (None, 0), (form, v, rc, msg)
        rc, msg, n_bad, out = _call(env, form, lab=bad, **v)
        assert rc == _lib.GNX_EINVAL and msg == "%s: 1 labels lie outside [0, %d); %s" % (who, A, tail), (form, v, rc, msg)
        assert n_bad in (None, 1)
        for k, a in out.items():
            assert not (a == _poison(a.dtype)).any(), (form, v, k)     # every output was written


@pytest.mark.parametrize("op", ["counts", "assoc", "logit", "score", "pairs", "ld"])
def test_the_forms_of_an_op_agree_bit_for_bit(env, op):
    """host rows, device rows (int8, and 2-bit where the form takes a row_kind) and the rows the file path builds (two batches) are the
    same matrix: so are the outputs"""
    from gnomix_amd import _lib
    got = {}
    for kind in ("", "_dev", "_gt2"):
        for v in ({}, {"kind": 1}) if op + kind in HAS_ROW_KIND else ({},):
            rc, msg, _, out = _call(env, op + kind, **v)
            assert rc == _lib.GNX_OK, (op + kind, v, msg)
            got[kind + ("/2-bit" if v else "")] = out
    for which, out in got.items():
        # (the score kernel's tiles differ by row form, and with them the order of its float64 sums: its 2-bit forms are held to each other)
        ref = got["/2-bit"] if op == "score" and which.endswith("/2-bit") else got[""]
        for k, a in ref.items():
            assert a.tobytes() == out[k].tobytes(), (op, which, k)
