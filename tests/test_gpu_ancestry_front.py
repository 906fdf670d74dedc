"""Every ancestry-specific op through DeviceModel in every form it has (host int8, host 2-bit, CUDA int8, CUDA 2-bit, the parsed query):
the forms are one op over three fronts (gnomix_amd/ancestry_ops.py), so they return the same bits, give the same verdict on a label out
of range, and HipGnomix returns the same from a numpy X and from the same X as a CUDA tensor.

The tiny case of test_gpu_summary_forms.py: 8 haplotypes, C = 37, M = 9, W = 4, A = 3, K = 2 covariates, S = 2 scores, T = 3 traits, band
5, SNP range [5, 30) (it starts and ends inside a window), a synthetic model of that geometry in a context with GNX_HOST_BATCH=4: the file
path's forms run two batches."""
import os

import numpy as np
import pytest

import allele_counts_exact as AE

pytestmark = pytest.mark.gpu

N, C, M, W, A, K, S, T = 8, 37, 9, 4, 3, 2, 2, 3
BAND, C0, C1 = 5, 5, 30


@pytest.fixture(scope="module")
def env():
    import torch
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
    d = synth.synthetic_model(C=C, M=M, A=A, S=1, n_rounds=2, seed=C)
    assert (d.C, d.M, d.W, d.A) == (C, M, W, A)
    dev = gnomix_amd.DeviceModel(d, ctx=ctx)
    rng = np.random.default_rng(C)
    X = synth.synthetic_X(N, C, seed=5, miss=0.1).astype(np.int8)
    assert set(np.unique(X)) <= {0, 1, 2}
    lab = rng.integers(0, A, size=(N, W)).astype(np.int32)
    Xt = torch.from_numpy(X).cuda()
    e = dict(ctx=ctx, dev=dev, data=d, X=X, lab=lab, P=np.array(dev.pack_x(X)), Xt=Xt, Pt=dev.pack_device(Xt), G=np.ascontiguousarray(vcfio.pack_gt2(X)),
             src=np.arange(C, dtype=np.int32), y=np.array([0.0, 1.0, 1.0, 0.0]), Y=rng.normal(size=(N // 2, T)),
             Z=np.ascontiguousarray(np.stack([np.ones(N // 2), rng.normal(size=N // 2)], axis=1)),
             w=rng.normal(size=(C, A, S)), eff=rng.integers(0, 2, size=C).astype(np.uint8))
    yield e
    ctx.close()


def _forms(e, lab, op, check=None):
    """form -> a thunk of DeviceModel's method of `op` in that form under the labels `lab`; check: passed on where the form takes it"""
    import torch
    dev, G, src = e["dev"], e["G"], e["src"]
    lt = torch.from_numpy(lab).cuda()
    rows = {"host": (e["X"], lab), "host/2-bit": (e["P"], lab), "cuda": (e["Xt"], lt), "cuda/2-bit": (e["Pt"], lt)}
    ck = {} if check is None else {"check": check}
    out = {}
    for form, (x, l) in rows.items():
        on_dev, packed = form.startswith("cuda"), {"packed": True} if form == "host/2-bit" else {}
        if op == "counts":
            out[form] = lambda x=x, l=l, on_dev=on_dev, packed=packed: (dev.ancestry_allele_counts_device if on_dev else dev.ancestry_allele_counts)(x, l, **packed)
        elif op == "dosage":
            out[form] = lambda x=x, l=l, on_dev=on_dev, packed=packed: (dev.ancestry_dosage_device if on_dev else dev.ancestry_dosage)(x, l, 1, **packed)
        elif op == "score":
            out[form] = lambda x=x, l=l, on_dev=on_dev, packed=packed: (dev.ancestry_scores_device if on_dev else dev.ancestry_scores)(x, l, e["w"], e["eff"], **packed)
        elif op == "pairs":
            out[form] = lambda x=x, l=l, on_dev=on_dev, packed=packed: (dev.ancestry_pair_counts_device if on_dev else dev.ancestry_pair_counts)(x, l, 1, (C0, C1), **packed)
        elif op == "ld":
            out[form] = lambda x=x, l=l, on_dev=on_dev, packed=packed: (dev.ancestry_ld_counts_device if on_dev else dev.ancestry_ld_counts)(x, l, 1, C0, C1, BAND, **packed)
        elif form != "host/2-bit":        # the association ops take numpy arrays or CUDA tensors under one name; int8 rows only on the host
            if op == "assoc":
                out[form] = lambda x=x, l=l: dev.ancestry_assoc_stats(x, l, e["y"], e["Z"], None, C0, C1, **ck)
            elif op == "traits":
                out[form] = lambda x=x, l=l: dev.ancestry_assoc_traits_stats(x, l, e["Y"], e["Z"], None, C0, C1, **ck)
            else:
                out[form] = lambda x=x, l=l: dev.ancestry_assoc_logit_fit(x, l, e["y"], e["Z"], None, C0, C1, **ck)
    gt2 = {"counts": lambda: dev.allele_counts_gt2(G, N, src, lab),
           "score": lambda: dev.ancestry_scores_gt2(G, N, src, lab, e["w"], e["eff"]),
           "pairs": lambda: dev.ancestry_pair_counts_gt2(G, N, src, lab, 1, (C0, C1)),
           "ld": lambda: dev.ancestry_ld_counts_gt2(G, N, src, lab, 1, C0, C1, BAND),
           "assoc": lambda: dev.ancestry_assoc_stats_gt2(G, N, src, lab, e["y"], e["Z"], None, C0, C1, **ck),
           "traits": lambda: dev.ancestry_assoc_traits_stats_gt2(G, N, src, lab, e["Y"], e["Z"], None, C0, C1, **ck),
           "logit": lambda: dev.ancestry_assoc_logit_fit_gt2(G, N, src, lab, e["y"], e["Z"], None, C0, C1, **ck)}
    if op in gt2:
        out["gt2"] = gt2[op]
    return out


def _host(result):
    """the fields of a returned tuple as numpy arrays (scalars as 0-d arrays), on the host"""
    return [np.asarray(v.cpu().numpy() if hasattr(v, "is_cuda") else v) for v in result]


def _same_bits(got, what):
    ref_form = sorted(got)[0]
    ref = got[ref_form]
    for form, out in got.items():
        assert len(out) == len(ref)
        for i, (a, b) in enumerate(zip(ref, out)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, ref_form, form, i, np.abs(a - b).max() if a.shape == b.shape else None)


OPS = ["counts", "dosage", "score", "pairs", "ld", "assoc", "traits", "logit"]
N_FORMS = {"counts": 5, "dosage": 4, "score": 5, "pairs": 5, "ld": 5, "assoc": 4, "traits": 4, "logit": 4}


@pytest.mark.parametrize("op", OPS)
def test_the_forms_of_an_op_agree_bit_for_bit(env, op):
    forms = _forms(env, env["lab"], op)
    assert len(forms) == N_FORMS[op]
    got = {}
    for form, call in forms.items():
        result = call()
        # tensors come back from tensors, arrays from arrays (the association blocks are numpy arrays from either)
        arrays = [v for v in result if hasattr(v, "shape") and v is not None]
        on_dev = form.startswith("cuda") and op not in ("assoc", "traits", "logit")
        assert all(hasattr(v, "is_cuda") == on_dev for v in arrays), (op, form)
        got[form] = _host(result)
    _same_bits(got, op)
    if op == "counts":
        for a, b in zip(got["host"], AE.allele_counts(env["X"], env["lab"], M, A)):
            assert np.array_equal(a, b)
    if op in ("assoc", "traits", "logit"):
        assert all(int(out[-1]) == 0 for out in got.values())      # n_bad


@pytest.mark.parametrize("op", OPS)
def test_a_label_out_of_range_gets_one_verdict_in_every_form(env, op):
    from gnomix_amd import GnxError, postprocess as pp
    bad = env["lab"].copy()
    bad[5, 2] = A
    if op in ("assoc", "traits", "logit"):       # every form has `check`
        got = {}
        for form, call in _forms(env, bad, op, check=False).items():
            got[form] = _host(call())
            assert int(got[form][-1]) == 1, (op, form)             # n_bad
        assert len(got) == N_FORMS[op]
        _same_bits(got, op)
        for form, call in _forms(env, bad, op, check=True).items():
            with pytest.raises(GnxError, match="1 labels lie outside"):
                call()
        return
    for form, call in _forms(env, bad, op).items():               # DeviceModel's forms of the other ops have none: they raise
        with pytest.raises(GnxError, match="1 labels lie outside"):
            call()
    if op in ("pairs", "ld"):                    # the host functions of postprocess have it
        ctx, X, P = env["ctx"], env["X"], env["P"]
        fn = (lambda rows, lab, **kw: pp.pair_counts(ctx, rows, lab, M, A, 1, (C0, C1), C=C, **kw)) if op == "pairs" else (
            lambda rows, lab, **kw: pp.ld_counts(ctx, rows, lab, M, A, 1, C0, C1, BAND, C=C, **kw))
        got = {"host": _host(fn(X, bad, check=False)), "host/2-bit": _host(fn(P, bad, check=False, packed=True))}
        _same_bits(got, op)
        # such a label counts for no ancestry: the tables are those of the labels with that haplotype's window given to another ancestry
        other = bad.copy()
        other[5, 2] = 0
        _same_bits({"bad": got["host"], "other": _host(fn(X, other))}, op)
        for rows, kw in ((X, {}), (P, {"packed": True})):
            with pytest.raises(GnxError, match="1 labels lie outside"):
                fn(rows, bad, check=True, **kw)


@pytest.mark.parametrize("mode_filter", [0, 3])
def test_hipgnomix_agrees_between_a_numpy_x_and_a_cuda_tensor(env, mode_filter):
    import gnomix_amd
    g = gnomix_amd.HipGnomix(env["data"], ctx=env["ctx"], mode_filter=mode_filter)
    assert g.smooth.mode_filter == mode_filter
    X, Xt = env["X"], env["Xt"]
    calls = {"allele_frequencies": lambda x: g.allele_frequencies(x),
             "ancestry_scores": lambda x: g.ancestry_scores(x, env["w"], env["eff"]),
             "ancestry_pair_counts": lambda x: g.ancestry_pair_counts(x, 1, (C0, C1)),
             "ancestry_ld": lambda x: g.ancestry_ld(x, 1, C0, C1, BAND)}
    for name, call in calls.items():
        host, cuda = call(X), call(Xt)
        assert all(isinstance(v, np.ndarray) for v in host if hasattr(v, "shape")), name
        assert all(v.is_cuda for v in cuda if hasattr(v, "shape")), name
        _same_bits({"numpy": _host(host), "cuda": _host(cuda)}, name)
    # and they are the op under the labels predict returns
    lab = g.predict(X).astype(np.int32)
    _same_bits({"method": _host(g.allele_frequencies(X)), "op": _host(g.dev.ancestry_allele_counts(X, lab))}, "allele_frequencies")
