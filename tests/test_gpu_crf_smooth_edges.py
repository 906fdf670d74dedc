"""The CRF smoother (csrc/k_smooth_crf.hip) on every kernel variant, at every chain, block and label-count edge, every forward-scale
interval and its thresholds, ties and arg-max edges — against an independent reference.

tests/test_gpu_parity.py holds the smoother to the oracle at eleven shapes and on four of its variants.  Here:
  variants   the default kernel with and without its own psi pass, with one and with four waves per block; round 3's row kernel with
             and without the psi pass; the scan (<= 8 labels) and the lanes kernel (any label count, the only one for 17..32) — one
             context each, the knobs being read once per context;
  grids      tests/crf_smooth_cases.py: label counts at every row-width and template switch, chains at every stride of every kernel
             (W = 1 .. 33), batches one below, at and one above every block size, r = max|state| + max|trans| exactly at and one
             double above 37.5 / 75 / 150 with the last window on and off the scale interval, weights 5x .. 40x a trained model's;
  ties       uniform marginals, duplicated columns (bit-identical marginals, the lower label wins), two marginals in one high
             32-bit word with either as the larger, a window whose potentials all underflow (the sum == 0 branch), one-hot and uniform B;
  reference  a log-space forward-backward in longdouble, itself checked against a sum over all paths (tests/test_crf_smooth_cases_host.py).
The bar on max|p - reference| is crf_smooth_cases.bound — first-order rounding analysis of a float64 pass — capped by the project's
existing bars (1e-11 for trained-range weights, 1e-9 for the far-range and threshold cases).  Labels are compared wherever the
reference's top-two gap exceeds twice the bound, which on every grid, threshold and far case is every window."""
import numpy as np
import pytest

import crf_smooth_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _new_context(variant):
    from gnomix_amd import _lib
    with pytest.MonkeyPatch.context() as mp:
        for k in SC.KNOBS:
            mp.delenv(k, raising=False)
        for k, v in SC.VARIANTS[variant].items():
            mp.setenv(k, v)
        return _lib.Context(0)          # the knobs are read here, once


@pytest.fixture(scope="module")
def contexts():
    """variant -> its context, made on first use and shared by the module"""
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = _new_context(variant)
        return made[variant]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module", autouse=True)
def worst():
    """kernel -> the largest max|p - reference| seen, with its bar and case; printed when the module is done"""
    w = {}
    yield w
    for k in sorted(w):
        print("\n[crf-smooth-edges] %-12s worst max|p - ref| %.3g (bar %.3g, %s); worst err / bar %.3g (%s)" % ((k,) + w[k]["abs"] + w[k]["rel"]))


def _model(ga, ctx, cid):
    N, W, A = SC.shape(cid)
    _, state, trans = SC.inputs(cid)
    d = ga.GnxModelData(C=W * 10 + 3, M=10, A=A, S=75, context=5, smooth_kind="crf", crf_state=state, crf_trans=trans)
    return ga.DeviceModel(d, ctx=ctx)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _params(ids):
    """(variant, case) for every variant and case.  Above 16 labels every variant is the lanes kernel: run once, as `lanes`.  For
    9..16 labels the scan variant is the default kernel: skipped, the reason in the id"""
    out = []
    for v in SC.VARIANTS:
        for cid in ids:
            A = SC.shape(cid)[2]
            if A > 16 and v != "lanes":
                continue
            if SC.resolves_to(v, A) != v:
                out.append(pytest.param(v, cid, id="%s-%s-is_%s_at_%d_labels" % (v, SC.name(cid), SC.resolves_to(v, A), A),
                                        marks=pytest.mark.skip(reason="scan serves up to 8 labels: this context runs the default kernel, which `ck` covers")))
            else:
                out.append(pytest.param(v, cid, id="%s-%s" % (v, SC.name(cid))))
    return out


def _check(worst, variant, dev, cid):
    """every assertion of one case -> p, labels of the full float64 call"""
    N, W, A = SC.shape(cid)
    B, state, trans = SC.inputs(cid)
    kind = cid[1] if cid[0] == "tie" else cid[0]
    p, lab = dev.smooth_predict(B)
    assert p.dtype == np.float64 and p.shape == (N, W, A) and lab.dtype == np.int32 and lab.shape == (N, W)
    assert np.all(np.isfinite(p))
    p32, lab32 = dev.smooth_predict(B, proba_dtype=np.float32)
    assert p32.dtype == np.float32 and _bits(p32) == _bits(p.astype(np.float32)) and _bits(lab32) == _bits(lab)
    if kind == "dead":                  # the sum == 0 branch, as the oracle defines it: zeros, label 0
        assert not np.any(p) and not np.any(lab)
        return p, lab
    p_ref, l_ref, _ = SC.reference(cid)
    bar = SC.bar(cid)
    err = float(np.max(np.abs(p.astype(SC.LD) - p_ref)))
    rows = float(np.max(np.abs(p.astype(SC.LD).sum(-1) - 1)))
    print("%s %s: max|p - ref| %.3g, bar %.3g, row sums off by %.3g" % (variant, SC.name(cid), err, bar, rows))
    k = SC.resolves_to(variant, A)
    w = worst.setdefault(k, {"abs": (0.0, 0.0, ""), "rel": (0.0, "")})
    if err >= w["abs"][0]:
        w["abs"] = (err, bar, SC.name(cid))
    if err / bar >= w["rel"][0]:
        w["rel"] = (err / bar, SC.name(cid))
    assert err <= bar
    ok = SC.comparable(cid)
    assert np.array_equal(lab[ok], l_ref[ok])
    assert np.all((lab >= 0) & (lab < A))
    assert rows <= A * bar
    if kind == "uniform":
        assert np.array_equal(p.view(np.uint64), np.broadcast_to(p[..., :1], p.shape).view(np.uint64)) and not np.any(lab)
    if kind == "duplicate":
        _, _, _, j, k2, _ = cid
        assert _bits(p[..., j]) == _bits(p[..., k2])
        assert np.all(lab[SC.pair_wins(cid)] == j)
    if kind == "low_word":
        _, _, _, j, k2, sign = cid
        wins = SC.pair_wins(cid)
        assert np.all(lab[wins] == (k2 if sign > 0 else j))
        same = SC.high_word(p[..., j])[wins] == SC.high_word(p[..., k2])[wins]
        assert 2 * same.sum() >= same.size        # the device's own marginals: the pair is told apart by the low words
    return p, lab


@pytest.mark.parametrize("variant,cid", _params(SC.GRID_IDS))
def test_labels_chains_and_blocks(ga, contexts, worst, variant, cid):
    _check(worst, variant, _model(ga, contexts(variant), cid), cid)


@pytest.mark.parametrize("variant,cid", _params(SC.THRESHOLD_IDS))
def test_scale_interval_thresholds(ga, contexts, worst, variant, cid):
    """r exactly at 37.5 / 75 / 150 (the longer interval) and one double above (the shorter), the last window on the interval (W = 24)
    and off it (W = 25); once with B rows that sum to 2, the slack gnx_build_crf's comment claims"""
    _check(worst, variant, _model(ga, contexts(variant), cid), cid)


@pytest.mark.parametrize("variant,cid", _params(SC.FAR_IDS))
def test_weights_far_beyond_a_trained_model(ga, contexts, worst, variant, cid):
    _check(worst, variant, _model(ga, contexts(variant), cid), cid)


@pytest.mark.parametrize("variant,cid", _params(SC.TIE_IDS))
def test_ties_and_argmax_edges(ga, contexts, worst, variant, cid):
    _check(worst, variant, _model(ga, contexts(variant), cid), cid)


@pytest.mark.parametrize("variant,cid", _params(SC.F32_IDS))
def test_float32_base_probabilities(ga, contexts, worst, variant, cid):
    assert SC.inputs(cid)[0].dtype == np.float32          # the reference is computed from the widened values
    _check(worst, variant, _model(ga, contexts(variant), cid), cid)


def _form_cases(variant):
    A = 5 if variant == "scan" else 12
    return [("chain", 5, 25, A), ("chain", 5, 7, A)]      # two segments on the default kernel's plain path, and none


@pytest.mark.parametrize("variant", list(SC.VARIANTS))
def test_output_forms(ga, contexts, worst, variant):
    """labels only, probabilities only (either width), and the device-pointer entry: the same bits as the full host call"""
    import torch
    for cid in _form_cases(variant) + ([("label", 5, 19, 20)] if variant == "lanes" else []):
        dev = _model(ga, contexts(variant), cid)
        B = SC.inputs(cid)[0]
        p, lab = _check(worst, variant, dev, cid)
        none, lab1 = dev.smooth_predict(B, want_proba=False)
        assert none is None and _bits(lab1) == _bits(lab)
        p1, none = dev.smooth_predict(B, want_labels=False)
        assert none is None and _bits(p1) == _bits(p)
        p2, none = dev.smooth_predict(B, want_labels=False, proba_dtype=np.float32)
        assert none is None and _bits(p2) == _bits(p.astype(np.float32))
        Bt = torch.from_numpy(np.array(B)).to("cuda:0")
        pt, lt = dev.smooth_predict_device(Bt, proba_dtype=torch.float64)
        assert _bits(pt.cpu().numpy()) == _bits(p) and _bits(lt.cpu().numpy()) == _bits(lab)
        none, lt = dev.smooth_predict_device(Bt, want_proba=False)
        assert none is None and _bits(lt.cpu().numpy()) == _bits(lab)
        pt, none = dev.smooth_predict_device(Bt, want_labels=False)
        assert none is None and pt.dtype == torch.float32 and _bits(pt.cpu().numpy()) == _bits(p.astype(np.float32))


@pytest.mark.parametrize("variant,cid", _params([("block",) + c for c in SC.BLOCK_CASES]))
def test_a_haplotype_alone_is_its_row_of_the_batch(ga, contexts, variant, cid):
    N, W, A = SC.shape(cid)
    dev = _model(ga, contexts(variant), cid)
    B = SC.inputs(cid)[0]
    p, lab = dev.smooth_predict(B)
    for i in sorted({0, N // 2, N - 1}):
        pi, li = dev.smooth_predict(B[i:i + 1])
        assert _bits(pi[0]) == _bits(p[i]) and _bits(li[0]) == _bits(lab[i]), i


@pytest.mark.parametrize("variant", [v for v in SC.VARIANTS if v != "scan"])      # 16 labels: the scan context runs the default kernel
def test_scratch_is_reused_across_calls(ga, worst, variant):
    """a large launch, a small one, the large one again on ONE context: the scratch (psi, parked alphas, scales) that the first left
    behind changes nothing"""
    big, small = ("label", 65, 33, 16), ("label", 3, 5, 16)
    ctx, fresh = _new_context(variant), _new_context(variant)
    try:
        dev_big, dev_small = _model(ga, ctx, big), _model(ga, ctx, small)
        p1, l1 = _check(worst, variant, dev_big, big)
        ps, ls = _check(worst, variant, dev_small, small)
        p3, l3 = dev_big.smooth_predict(SC.inputs(big)[0])
        assert _bits(p1) == _bits(p3) and _bits(l1) == _bits(l3)
        pf, lf = _model(ga, fresh, small).smooth_predict(SC.inputs(small)[0])
        assert _bits(ps) == _bits(pf) and _bits(ls) == _bits(lf)
    finally:
        ctx.close()                     # (closes its models first)
        fresh.close()
