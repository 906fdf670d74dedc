"""-m gpu: the NUMBERS of the logistic base pass (every other logistic test varies the geometry, on coefficients ~N(0, 0.05)).

Every case runs through every implementation — the float64 MFMA kernel (GNX_BASE_LR_IMPL=f64), the int8 kernels (register-staged
and LDS-direct loads), and the 2-bit kernels (slot tiles and, at 24 class columns, flat tiles) at both run lengths — and asserts
 (i)  the integer kernels are bit-identical to each other;
 (ii) every implementation is within the DERIVED bound lr_exact.bound_B of the exact reference lr_exact.proba(exact_t) (the exactly
      rounded sum on the reflect-padded X, sigmoid and normaliser in longdouble; pinned to the reference's own outputs G1 / G15 in
      tests/test_lr_exact_host.py);
 (iii) where a case says so, the integer kernels equal the arithmetic they document (lr_exact.fixed_point_t: q = rint(c 2^f_w),
      integer sum, one rounding, + b) to the few ulp of the float64 epilogue (lr_exact.epilogue_ulps) — the claim of an EXACT logit,
      which neither (i) (a fault the integer kernels share) nor a 1e-12 bar (a fault below it at |c| ~ 0.05) can see.
No bound here was tuned against a kernel.

Where 1e-12 on B stops being guaranteed (from bound_B: the quantisation term n_w xmax 2^(e_w - 54) alone reaches 5e-13, half of
1e-12 before the normaliser doubles it, at n_w xmax 2^e_w = 9007): for a window of n_w SNPs (padded width) and X values up to xmax,
B is within 1e-12 of the exact reference while  n_w * xmax * max|c| <= 8000  and |t| <= 100 — max|c| <= 20 for the 200-SNP windows of
these tests, max|c| <= 2 for the 2 000-SNP windows of chr22 at context 0.5.  Beyond it the error grows in proportion (test_dynamic_range).

Saturation: -t is capped at 708 before the exponential (gnx_exp.h), so a class with -t > 708 gets s = 1 / (1 + e^708) = 3.3e-308
instead of its (smaller) value.  bound_B carries that as its own term, 2 n_capped 3.3e-308 / sum(s): nothing (< 1e-17) while some
class of the row has s >= 1e-290 (-t <= 667), and of order 1 for rows whose every class is below that — the documented deviation,
pinned by the named tests at the end (they hold the kernels to the capped expression itself)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import lr_exact as E

pytestmark = pytest.mark.gpu

S_CAP = 1.0 / (1.0 + math.exp(708.0))      # what a capped class contributes


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


# name -> (environment read at context creation / model load, packed input?)
IMPLS = {
    "f64":    ({"GNX_BASE_LR_IMPL": "f64", "GNX_LR_DL": "0"}, False),
    "i8":     ({"GNX_BASE_LR_IMPL": "i8", "GNX_LR_DL": "0"}, False),
    "i8dl":   ({"GNX_BASE_LR_IMPL": "i8", "GNX_LR_DL": "1"}, False),
    "p2s256": ({"GNX_BASE_LR_IMPL": "i8", "GNX_LR_P2": "2", "GNX_LR_P2_FLAT": "0", "GNX_LR_P2_RUN": "256"}, True),
    "p2s512": ({"GNX_BASE_LR_IMPL": "i8", "GNX_LR_P2": "2", "GNX_LR_P2_FLAT": "0", "GNX_LR_P2_RUN": "512"}, True),
    "p2f256": ({"GNX_BASE_LR_IMPL": "i8", "GNX_LR_P2": "2", "GNX_LR_P2_FLAT": "1", "GNX_LR_P2_RUN": "256"}, True),   # flat tiles where R A = 24
    "p2f512": ({"GNX_BASE_LR_IMPL": "i8", "GNX_LR_P2": "2", "GNX_LR_P2_FLAT": "1", "GNX_LR_P2_RUN": "512"}, True),
}
ENV_KEYS = ("GNX_BASE_LR_IMPL", "GNX_LR_DL", "GNX_LR_P2", "GNX_LR_P2_FLAT", "GNX_LR_P2_RUN", "GNX_LR_FLAGS", "GNX_P2_TUNE")


def _run(ga, monkeypatch, name, d, X):
    """B (N, W, A) float64 of one implementation: a context and a model of its own (the switches are read there)"""
    import torch
    from gnomix_amd import _lib
    env, packed = IMPLS[name]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = _lib.Context(0)
    dev = ga.DeviceModel(d, ctx=ctx)
    try:
        if packed:
            P = torch.from_numpy(np.asarray(dev.pack_x(X))).cuda()
            B = dev.base_predict_packed_device(P, f64=True)
        else:
            B = dev.base_predict_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(), f64=True)
        torch.cuda.synchronize()
        return B.cpu().numpy()
    finally:
        dev.close()
        ctx.close()


def _names(d, packed=True, only=None):
    R = -(-(d.M + 2 * d.context) // d.M)
    names = [n for n in IMPLS if (packed or not IMPLS[n][1]) and (R * d.A == 24 or not n.startswith("p2f"))]
    return [n for n in names if only is None or n in only]


def _model(ga, C, M, A, ctx, seed, coef_sd=0.05, icpt_sd=0.5):
    from gnomix_amd import synth
    d = synth.synthetic_model(C=C, M=M, A=A, S=5, context=ctx, seed=seed, smooth=None, coef_sd=coef_sd, icpt_sd=icpt_sd)
    for w, (lo, n) in enumerate(E.windows(C, M, ctx)):
        d.lr_coef[w, :, n:] = 0.0            # columns past a window's width are never read
    return d


def _clamp_term(t_exact):
    """the cap's share of the bound: |ds| <= S_CAP for every class with -t > 708, so |dB| <= 2 n_capped S_CAP / sum(s)"""
    with np.errstate(over="ignore"):
        s = (E.LD(1) / (E.LD(1) + np.exp(-t_exact)))
    capped = (-t_exact > 708).sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        term = np.where(capped > 0, 2 * capped * E.LD(S_CAP) / s.sum(-1, keepdims=True), 0)
    return np.minimum(term, E.LD(2)).astype(np.float64) + np.zeros(t_exact.shape)


def _check(ga, monkeypatch, d, X, sharp, packed=True, only=None, label=""):
    """(i), (ii) and — sharp=True — (iii) of the module docstring; prints every figure before it asserts; returns the outputs"""
    C, M, ctx, A = d.C, d.M, d.context, d.A
    out = {n: _run(ga, monkeypatch, n, d, X) for n in _names(d, packed, only)}
    ints = [n for n in out if n != "f64"]
    for n in ints[1:]:
        assert np.array_equal(out[ints[0]], out[n]), (label, ints[0], n, int(np.isnan(out[ints[0]]).sum()), int(np.isnan(out[n]).sum()))
    t, Z64, absum = E.exact_t(X, M, ctx, d.lr_coef, d.lr_intercept)
    Bx = E.proba(t)
    clamp = _clamp_term(t)
    t64 = t.astype(np.float64)
    for n, B in out.items():
        skip = np.zeros(B.shape[:2], bool)
        if n == "f64":       # the float64 kernel has no cap: like the reference, 0 / 0 where every class has e^-t = inf
            assert np.all(np.isnan(B[(-t64 > 710).all(-1)])) and np.all(np.isfinite(B[(-t64 < 709).any(-1)])), (label, n)
            skip = (-t64 > 709).all(-1)                                   # (those rows: asserted just above)
            B = np.where(skip[..., None], 1.0 / A, B)
        assert np.all(np.isfinite(B)), (label, n)
        bound = E.bound_B(X, M, ctx, d.lr_coef, d.lr_intercept, "f64" if n == "f64" else "int", Z64, absum) + clamp
        err = np.abs((B.astype(E.LD) - Bx).astype(np.float64))
        ok = np.isfinite(err) & ~skip[..., None]       # (rows where the exact reference itself is 0 / 0 belong to the named tests below)
        print("%s %-6s max err %.3g  max err/bound %.3g  (largest bound %.3g)" % (label, n, err[ok].max(), (err[ok] / bound[ok]).max(), bound[ok].max()))
        assert np.all(err[ok] <= bound[ok]), (label, n)
        rows = ok.all(-1)
        assert np.all(np.abs(B.sum(-1)[rows] - 1.0) <= A * 2.0 ** -52), (label, n)
        safe = rows & (clamp.max(-1) < 1e-6) & (bound.max(-1) < 1e-9)
        top2, tt2 = np.sort(Bx, -1)[..., -2:], np.sort(t, -1)[..., -2:]       # a clear winner, or an exact tie (the first wins)
        clear = safe & ((top2[..., 1] - top2[..., 0] > 1e-6) | (tt2[..., 1] == tt2[..., 0]))
        assert np.array_equal(np.argmax(B, -1)[clear], np.argmax(Bx, -1)[clear]), (label, n)
    if sharp:
        _check_sharp(out[ints[0]], X, d, label)
    return out


def _check_sharp(B, X, d, label=""):
    """B of an integer kernel against the capped sigmoid + normaliser (longdouble) of the fixed-point logit it documents"""
    tf = E.fixed_point_t(X, d.M, d.context, d.lr_coef, d.lr_intercept)
    Bf = E.proba_clamped(tf)
    tol = E.epilogue_ulps(d.A) * E.ULP * np.abs(Bf).astype(np.float64) + 1e-300
    err = np.abs((B.astype(E.LD) - Bf).astype(np.float64))
    print("%s fixed-point image: max err %.3g = %.2f of the epilogue's %.1f ulp" % (label, err.max(), (err / tol).max(), E.epilogue_ulps(d.A)))
    assert np.all(err <= tol), label


def _rows(N, C, seed, codes=(1, 2)):
    from gnomix_amd import synth
    X = synth.synthetic_X(N, C, seed=seed, miss=0.1)
    for r, v in enumerate(codes):
        X[r, :] = v
    return X


# ---------------------------------------------------------------- 1. digit and carry edges ------------------
def _limbs(ds):
    return sum(int(dg) * 256 ** l for l, dg in enumerate(ds))


# fixed-point images q of one window's coefficients; the first entry of every list is at least 2^53 in magnitude (it sets the
# window's scale: f_w = 53 - ilogb(max |c|) puts the largest image in [2^53, 2^54)); fractions are values BETWEEN grid points.
# (An image in [2^53, 2^54) is even — c is a float64 — so the largest reachable one is 2^54 - 2, not 2^54 - 1.)
Q_PATTERNS = [
    [2 ** 54 - 2], [-(2 ** 54 - 2)], [2 ** 53], [-(2 ** 53)],
    [2 ** 53, 1, -1, 3, -3],
    [-(2 ** 53), Fraction(1, 4), Fraction(-1, 4), Fraction(1, 2), Fraction(-1, 2), Fraction(3, 8), Fraction(1, 2 ** 40)],     # all round to 0
    [2 ** 53, Fraction(3, 2), Fraction(5, 2), Fraction(-3, 2), Fraction(-5, 2), Fraction(7, 2), Fraction(255, 2), Fraction(-257, 2)],  # ties: half to even
    [_limbs([-128] * 6 + [-63])],                                         # every limb -128 (the top one as low as |q| < 2^54 lets it be)
    [2 ** 53, _limbs([127] * 6 + [31]), -_limbs([127] * 6 + [31])],       # every limb 127
    [_limbs([-128, 127, -128, 127, -128, 127, 40]), -_limbs([-128, 127, -128, 127, -128, 127, 40])],
    [2 ** 53, _limbs([127, -128, 127, -128, 127, -128, 30]), -_limbs([127, -128, 127, -128, 127, -128, 30])],
    [2 ** 53] + [dg * 256 ** l for l in range(6) for dg in (-128, 127, 128, 1, -1)],       # one non-zero limb (+128: a carry into the next)
    [-(2 ** 53)] + [dg * 256 ** 6 for dg in (-31, 31, 1, -1, 16)] + [32 * 256 ** 6 - 256],
    [2 ** 53, 128, 128 + 256 * 128, -129, 127 + 256 * 127, 32768, -32768, 32767, 2 ** 47, 2 ** 47 - 1, -(2 ** 47) - 1],   # carries that ripple
]


def _edge_model(ga, C, M, A, ctx, seed):
    """window w carries pattern w % len: its images spread over classes and over the columns [ctx, ctx + M) of the window (whose
    reflected partners hold zeros, so that folding changes nothing), scale exponent f_w varied; the special windows come last"""
    d = _model(ga, C, M, A, ctx, seed)
    d.lr_coef[:] = 0.0
    W = C // M
    rng = np.random.RandomState(seed)
    single = {}
    for w in range(W):
        pat = Q_PATTERNS[w % len(Q_PATTERNS)]
        f = 50 + (w % 7)                                   # largest |c| between 2^3 and 2^-3 .. moderate logits
        cols = ctx + rng.permutation(M)[:len(pat)]
        for k, q in enumerate(pat):
            c = float(Fraction(q) / Fraction(2) ** f)
            assert Fraction(c) * Fraction(2) ** f == Fraction(q)          # the coefficient has exactly this image
            d.lr_coef[w, (w + k) % A, cols[k]] = c
        if len(pat) == 1:
            single[w] = ((w + 0) % A, float(Fraction(pat[0]) / Fraction(2) ** f))
    # special windows
    d.lr_coef[W - 1] = 0.0                                                # all zeros
    single.pop(W - 1, None)
    d.lr_coef[W - 2] = 0.0
    d.lr_coef[W - 2, 0, ctx + 3] = -0.0
    d.lr_coef[W - 2, 1, ctx + 4] = 5e-324                                 # a denormal, the window's maximum: f_w = 53 + 1074
    d.lr_coef[W - 2, 2, ctx + 5] = -5e-324
    single.pop(W - 2, None)
    d.lr_coef[W - 3] = rng.standard_normal(d.lr_coef[W - 3].shape) * 0.05  # every ordinary weight of this window rounds to 0
    d.lr_coef[W - 3, :, E.windows(C, M, ctx)[W - 3][1]:] = 0.0
    d.lr_coef[W - 3, 0, ctx + 7] = 1e299
    d.lr_coef[W - 3, 1, ctx + 8] = -1e299
    single.pop(W - 3, None)
    d.lr_coef[W - 4] = 0.0
    d.lr_coef[W - 4, 3, ctx + 9] = 2.0 ** -1060                           # a denormal that is NOT the maximum: rounds to 0
    d.lr_coef[W - 4, 4, ctx + 9] = 1.0
    single.pop(W - 4, None)
    return d, single


@pytest.mark.parametrize("C,M,A,ctx", [(1837, 50, 7, 25), (3107, 100, 12, 50), (2401, 100, 8, 100)])
def test_digit_and_carry_edges(ga, monkeypatch, C, M, A, ctx):
    """coefficients whose fixed-point images sit at the corners of the digit split (Q_PATTERNS; -0.0, denormals, a window of zeros,
    a window whose maximum is 1e299), X all-1, all-2 and random: bit-identical integer kernels, the derived bound for all, and the
    integer kernels equal to their documented fixed-point arithmetic to the epilogue's few ulp (this is the assertion that sees a
    wrong digit: the bound of the 1e299 window, for one, is astronomically wide).  Windows with ONE non-zero coefficient and X all-1
    have B in closed form — s_a = sigmoid(b_a + c [a = a0]) —, asserted to the same few ulp."""
    d, single = _edge_model(ga, C, M, A, ctx, seed=C)
    X = _rows(6, C, seed=3)
    out = _check(ga, monkeypatch, d, X, sharp=True, label="edges")
    B = out["i8"]
    assert single
    for w, (a0, c) in single.items():
        t = d.lr_intercept[w].copy()
        t[a0] = t[a0] + c                               # the float64 addition the kernel makes; c itself is exact
        want = E.proba_clamped(t)
        err = np.abs((B[0, w].astype(E.LD) - want).astype(np.float64))
        assert np.all(err <= E.epilogue_ulps(A) * E.ULP * want.astype(np.float64)), (w, a0, c)
    W = C // M
    assert np.array_equal(B[:, W - 1], np.broadcast_to(B[0, W - 1], B[:, W - 1].shape))     # zero weights: the intercepts alone, every row
    assert np.array_equal(B[:, W - 2], B[:, W - 1] * 0 + B[0, W - 2])                       # +-5e-324 x 2 changes no logit


# ---------------------------------------------------------------- 2. dynamic range ------------------
@pytest.mark.parametrize("k", [0, 2, 4, 6, 8])
def test_dynamic_range(ga, monkeypatch, k):
    """one coefficient of 10^k in class 0 of every window (in the reflected margin of the first and last window, so that it is
    folded), the rest N(0, 0.05): one large weight coarsens the grid of every class of its window.  The derived bound (it grows
    with 10^k; for these 200-SNP windows 5.9e-14, 3.7e-12, 4.8e-10, 3.1e-8, 3.9e-6 at k = 0, 2, 4, 6, 8 — the integer kernels
    measured 1e-16, 6.5e-15, 9.2e-13, 4.1e-11, 5.6e-9 from the exact reference on an MI355X: 1e-12 ends between 1e4 and 1e6 in
    practice, at max|c| = 20 in the guarantee) and the documented fixed-point image (measured: within 0.17 of the epilogue's ulps)."""
    C, M, A, ctx = 3107, 100, 12, 50
    d = _model(ga, C, M, A, ctx, seed=k)
    W = C // M
    for w in range(W):
        d.lr_coef[w, 0, 5 + (7 * w) % (M + 2 * ctx - 10)] = 10.0 ** k
    d.lr_coef[0, 0, 3] = 10.0 ** k
    d.lr_coef[W - 1, 0, E.windows(C, M, ctx)[-1][1] - 4] = -(10.0 ** k)
    X = _rows(8, C, seed=k + 1)
    _check(ga, monkeypatch, d, X, sharp=True, label="range 1e%d" % k)


# ---------------------------------------------------------------- 3. saturation ------------------
T_SAT = [30.0, 700.0, 707.9, 708.0, 708.1, 709.7, 709.9, 745.0, 1e4, 1e300]


def _saturation_model(ga, zero_coef):
    """40 windows = 10 targets x 4 patterns, t set by the intercepts: one class dominant, two tied at the top (classes 2 and 4:
    identical rows, the first wins), every class at +T, every class at -T; and the same with one class at -T among ordinary ones"""
    C, M, A, ctx = 4037, 100, 7, 50
    d = _model(ga, C, M, A, ctx, seed=11)
    if zero_coef:
        d.lr_coef[:] = 0.0
    for w in range(C // M):
        T, pat = T_SAT[w // 4], w % 4
        if pat == 0:
            d.lr_intercept[w, 1] = T
            d.lr_intercept[w, 5] = -T
        elif pat == 1:
            d.lr_intercept[w, 2] = d.lr_intercept[w, 4] = T
            d.lr_coef[w, 4] = d.lr_coef[w, 2]
        elif pat == 2:
            d.lr_intercept[w, :] = T
        else:
            d.lr_intercept[w, :] = -T
    return d


def test_saturation(ga, monkeypatch):
    """t at +-{30, 700, 707.9, 708, 708.1, 709.7, 709.9, 745, 1e4, 1e300}; rows of zeros (t is the intercept exactly) and random
    rows (t a little off it).  Rows with a class at -t <= 708: the derived bound (with the cap's own term, see the module docstring),
    labels identical with the first maximum winning a tie, rows summing to 1 within A 2^-52 — all inside _check."""
    d = _saturation_model(ga, zero_coef=False)
    X = _rows(6, d.C, seed=5, codes=(0, 1))
    out = _check(ga, monkeypatch, d, X, sharp=True, label="saturation")
    B = out["i8"]
    for w in range(d.C // d.M):
        if w % 4 == 1:       # the tie: equal values, the label is the first of them
            assert np.array_equal(B[:, w, 2], B[:, w, 4])
            if T_SAT[w // 4] >= 30:
                assert np.all(np.argmax(B[:, w], -1) == 2)


def test_saturated_rows_follow_the_capped_expression_not_the_reference(ga, monkeypatch):
    """THE DOCUMENTED DEVIATION (gnx_exp.h): rows whose every class has -t > 708.  The reference's float64 formula
    1 / (1 + exp(-t)) / sum gives 0 / 0 = NaN there once -t passes 709.78 (shown below in numpy), and denormals without digits
    before that; the kernels give finite rows that sum to 1, equal to the same formula with -t capped at 708 — 1 / A when every
    class is capped.  Every integer implementation; the float64 MFMA kernel (GNX_BASE_LR_IMPL=f64, libm's exp, no cap) gives the
    reference's NaN."""
    d = _saturation_model(ga, zero_coef=True)
    X = _rows(3, d.C, seed=6, codes=(0, 2))
    A = d.A
    t64 = np.broadcast_to(d.lr_intercept[None], (3,) + d.lr_intercept.shape)
    all_capped = (-t64 > 708).all(-1)
    assert all_capped.sum() == 3 * 6                      # the all-negative windows of T = 708.1 ... 1e300
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = 1.0 / (1.0 + np.exp(-t64))
        ref = p / p.sum(-1, keepdims=True)
    beyond = (-t64 > 709.79).all(-1)
    assert beyond.sum() == 3 * 4 and np.all(np.isnan(ref[beyond]))          # the reference: 0 / 0
    want = E.proba_clamped(t64)
    for n in _names(d):
        B = _run(ga, monkeypatch, n, d, X)
        if n == "f64":
            assert np.all(np.isnan(B[beyond])) and np.all(np.isfinite(B[~all_capped])), n
            continue
        assert np.all(np.isfinite(B)), n
        assert np.all(np.abs(B.sum(-1) - 1.0) <= A * 2.0 ** -52), n
        err = np.abs((B.astype(E.LD) - want).astype(np.float64))
        assert np.all(err <= E.epilogue_ulps(A) * E.ULP * want.astype(np.float64) + 1e-300), (n, err.max())
        assert np.all(np.abs(B[all_capped] - 1.0 / A) <= E.epilogue_ulps(A) * E.ULP / A), n


def test_rows_of_tiny_sigmoids_are_lifted_to_the_cap(ga, monkeypatch):
    """the same deviation reaches rows that are only PARTLY beyond the cap when their largest sigmoid is itself tiny: classes at
    -t = 707.9 and 745 come out 0.52 / 0.48-like (the second lifted from e^-745 to e^-708) where exact arithmetic says 1 / 0.
    A finding of this module (the header spoke of rows whose EVERY class is beyond 708); the kernels are held to the capped
    expression, and the bound's cap term says where it matters: sum(s) below ~1e-290, i.e. every class at -t > 667."""
    C, M, A, ctx = 1237, 50, 7, 25
    d = _model(ga, C, M, A, ctx, seed=2)
    d.lr_coef[:] = 0.0
    for w in range(C // M):
        d.lr_intercept[w, :] = -745.0 - w
        d.lr_intercept[w, w % A] = -707.9 + 0.01 * w
        d.lr_intercept[w, (w + 3) % A] = -708.0
    X = _rows(2, C, seed=1, codes=(0, 1))
    t64 = np.broadcast_to(d.lr_intercept[None], (2,) + d.lr_intercept.shape)
    want = E.proba_clamped(t64)
    exact = E.proba(t64)
    assert float(np.max(np.abs((want - exact).astype(np.float64)))) > 0.3          # far from the exact value: this is the deviation
    ints = None
    for n in _names(d):
        if n == "f64":       # no cap there
            continue
        B = _run(ga, monkeypatch, n, d, X)
        err = np.abs((B.astype(E.LD) - want).astype(np.float64))
        assert np.all(err <= E.epilogue_ulps(A) * E.ULP * want.astype(np.float64) + 1e-300), (n, err.max())
        assert ints is None or np.array_equal(ints, B), n
        ints = B


# ---------------------------------------------------------------- 4. non-finite parameters ------------------
@pytest.mark.parametrize("impl", ["f64", "i8", "p2f256"])
def test_non_finite_parameters_are_refused_at_load(ga, monkeypatch, impl):
    """NaN, +Inf, -Inf in lr_coef (first and last column of a window, a reflected column, the only non-zero entry of a window) or in
    lr_intercept: gnx_model_load fails with GNX_EINVAL whichever kernels the model would run on; nothing is launched"""
    from gnomix_amd import _lib
    C, M, A, ctx = 3107, 100, 12, 50
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in IMPLS[impl][0].items():
        monkeypatch.setenv(k, v)
    c = _lib.Context(0)
    W = C // M
    last_w = E.windows(C, M, ctx)[-1][1]
    spots = [("first", 0, 0, 0), ("last", 5, 3, M + 2 * ctx - 1), ("last of the last window", W - 1, A - 1, last_w - 1),
             ("reflected", 0, 2, 7), ("reflected right", W - 1, 1, last_w - 3), ("only", 9, 4, 77)]
    for bad in (float("nan"), float("inf"), float("-inf")):
        for what, w, a, col in spots:
            d = _model(ga, C, M, A, ctx, seed=1)
            if what == "only":
                d.lr_coef[w] = 0.0
            d.lr_coef[w, a, col] = bad
            with pytest.raises(_lib.GnxError) as ei:
                ga.DeviceModel(d, ctx=c)
            assert ei.value.code == _lib.GNX_EINVAL, (bad, what)
        for w, a in ((0, 0), (W - 1, A - 1), (7, 5)):
            d = _model(ga, C, M, A, ctx, seed=1)
            d.lr_intercept[w, a] = bad
            with pytest.raises(_lib.GnxError) as ei:
                ga.DeviceModel(d, ctx=c)
            assert ei.value.code == _lib.GNX_EINVAL, (bad, w, a)
    # +Inf and -Inf in the two columns that fold into one weight (Inf - Inf), and two finite weights whose folded sum overflows
    d = _model(ga, C, M, A, ctx, seed=1)
    d.lr_coef[0, 0, 7], d.lr_coef[0, 0, 2 * ctx - 1 - 7] = float("inf"), float("-inf")
    with pytest.raises(_lib.GnxError) as ei:
        ga.DeviceModel(d, ctx=c)
    assert ei.value.code == _lib.GNX_EINVAL
    if impl != "f64":
        d = _model(ga, C, M, A, ctx, seed=1)
        d.lr_coef[0, 0, 7] = d.lr_coef[0, 0, 2 * ctx - 1 - 7] = 1.7e308
        with pytest.raises(_lib.GnxError) as ei:
            ga.DeviceModel(d, ctx=c)
        assert ei.value.code == _lib.GNX_EINVAL
    ga.DeviceModel(_model(ga, C, M, A, ctx, seed=1), ctx=c).close()        # the same model without the bad entry loads
    c.close()


# ---------------------------------------------------------------- 5. X codes ------------------
@pytest.mark.parametrize("C,M,A,ctx", [(1837, 50, 7, 25), (3107, 100, 12, 50)])
def test_x_codes(ga, monkeypatch, C, M, A, ctx):
    """rows of all 0, all 1, all 2, all 3, a row that is 3 only inside the reflected margins, random rows of 0..3 — as int8 and
    packed.  Code 3 is no code of the reference but a packed row can hold it: it enters as the number 3."""
    d = _model(ga, C, M, A, ctx, seed=C)
    X = _rows(8, C, seed=8, codes=(0, 1, 2, 3))
    X[4, :] = 0
    X[4, :ctx] = 3
    X[4, C - ctx:] = 3
    X[5] = np.random.RandomState(0).randint(0, 4, C)
    _check(ga, monkeypatch, d, X, sharp=True, label="codes")


def test_int8_values_outside_0_3(ga, monkeypatch):
    """what the entry points do with int8 values outside 0..3 (include/gnomix_hip.h): gnx_pack_x refuses them (GNX_EINVAL: two bits
    cannot hold them); the int8 entry points take the byte as the signed number it is — exact in the integer kernels (|acc| <=
    128 * 128 * K stays an int32 for windows up to 131 072 SNPs), a float64 conversion in the f64 kernel"""
    from gnomix_amd import _lib
    C, M, A, ctx = 1837, 50, 7, 25
    d = _model(ga, C, M, A, ctx, seed=5)
    X = _rows(6, C, seed=2, codes=(-1, 4, 127, -128))
    X[4] = np.random.RandomState(1).randint(-128, 128, C)
    _check(ga, monkeypatch, d, X, sharp=True, packed=False, label="int8 values")
    dev = ga.DeviceModel(d, ctx=_lib.Context(0))
    for v in (-1, 4, 127, -128):
        Xb = np.zeros((2, C), np.int8)
        Xb[1, C - 1] = v
        with pytest.raises(_lib.GnxError) as ei:
            dev.pack_x(Xb)
        assert ei.value.code == _lib.GNX_EINVAL


# ---------------------------------------------------------------- 6. wide windows ------------------
def _spans(C, M, cx, RS=256):
    """runs of RS SNPs each window spans in the 2-bit kernels' walk (gnx_build_lr: pieces end where windows end, a piece starts on a
    16-SNP boundary and is walked in whole runs; a window spans the pieces from the one its first SNP lies in to the one it ends)"""
    import bisect
    W, M_ = C // M, M + 2 * cx
    fpos = [min((i * M + M_ if i < W - 1 else C + 2 * cx) - cx, C) for i in range(W)]
    b = [0]
    for f in fpos:
        if f > b[-1]:
            b.append(f)
    pr = [0]
    for k in range(len(b) - 1):
        pr.append(pr[-1] + (b[k + 1] - (b[k] & ~15) + RS - 1) // RS)
    return [pr[bisect.bisect_left(b, fpos[i])] - pr[min(bisect.bisect_right(b, max(i * M - cx, 0)) - 1, len(b) - 2)] for i in range(W)]


Q_FOLDED = _limbs([-128] * 6 + [-31])      # windows 0 and 2: the margins fold to 2 c (which sets the scale), the bulk keeps this image
Q_PLAIN = _limbs([-128] * 6 + [-63])       # window 1, the widest span: nothing folds


def _wide_model(ga, M):
    """A = 12 at context 0.5 (24 class columns: the flat-tile kernel), W = 3; every coefficient of a window is +c (even classes) or
    -c (odd classes), c a value whose limbs 2k and 2k + 1 are both -128"""
    C, A, ctx = 3 * M + 5, 12, M // 2
    d = ga.GnxModelData(C=C, M=M, A=A, S=5, context=ctx, base_kind="logistic",
                        lr_coef=np.zeros((3, A, 2 * M + 5)), lr_intercept=np.random.RandomState(M).standard_normal((3, A)) * 0.5)
    cs = []
    for w, (lo, n) in enumerate(E.windows(C, M, ctx)):
        c = math.ldexp(float(Q_PLAIN if w == 1 else Q_FOLDED), -66)
        d.lr_coef[w, 0::2, :n] = c
        d.lr_coef[w, 1::2, :n] = -c
        cs.append((c, n))
    return d, cs


@pytest.mark.parametrize("runs,M", [(84, 8436), (86, 8692), (119, 12020), (121, 12276)])
def test_wide_windows(ga, monkeypatch, runs, M):
    """windows that span 84, 86, 119 and 121 runs of the 2-bit walk, every limb pair of every weight (-128, -128), X all-3, all-2,
    all-1: the largest sums the accumulators and the flat kernel's int32 limb PAIRS can meet.  A pair holds 257 * 128 * x * K:
    with x = 3 below 2^31 only while K < 21 760 SNPs = 85 runs, so the flat kernel takes windows up to 84 runs and declines wider
    ones (the rows are widened and the int8 kernels run); at 119 runs (K = 24 040) a pair WOULD wrap.  B is known in closed form
    from Python integers — t_a = fl(fl(+-x n c) + b_a), c on the window's grid — and asserted to the epilogue's few ulp.  At the
    widest model every implementation runs (windows of 24 557 SNPs), at the others the flat-tile route."""
    d, cs = _wide_model(ga, M)
    C, A, ctx = d.C, d.A, d.context
    assert max(_spans(C, M, ctx)) == runs
    X = np.zeros((3, C), np.int8)
    X[0], X[1], X[2] = 3, 2, 1
    t = np.zeros((3, 3, A))
    for w, (c, n) in enumerate(cs):
        for r, x in enumerate((3, 2, 1)):
            z = float(Fraction(c) * x * n)                      # correctly rounded: the one rounding of combine()
            t[r, w, 0::2] = z + d.lr_intercept[w, 0::2]
            t[r, w, 1::2] = -z + d.lr_intercept[w, 1::2]
    if runs == 84:           # the closed form is the fixed-point arithmetic (no coefficient is off the grid, the folded ones included)
        assert np.array_equal(t, E.fixed_point_t(X, M, ctx, d.lr_coef, d.lr_intercept))
    want = E.proba_clamped(t)
    tol = E.epilogue_ulps(A) * E.ULP * want.astype(np.float64)
    names = _names(d) if runs == 121 else ["p2f256"]
    ints = None
    for n in names:
        B = _run(ga, monkeypatch, n, d, X)
        err = np.abs((B.astype(E.LD) - want).astype(np.float64))
        print("wide %d runs %-6s max err %.3g (%.2f of the tolerance)" % (runs, n, err.max(), (err / tol).max()))
        if n == "f64":       # the float64 kernel: its dot-product bound n 2^-53 sum |c x| = n 2^-53 |Z| on t, doubled by the normaliser
            nmax = max(nn for _, nn in cs)
            assert np.all(err <= 2 * (nmax + 1) * E.ULP * np.abs(t).max() + 8 * E.ULP), n
            continue
        assert np.all(err <= tol), (runs, n, err.max())
        assert ints is None or np.array_equal(ints, B), n
        ints = B
