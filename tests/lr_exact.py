"""An exact host reference of the logistic base pass, and the error bounds the kernels are held to.  Plain Python: no GPU, no oracle.

What the reference computes (src/Base/base.py:41-44 `Base.pad`, :146-180 `predict_proba_vectorized`; src/Base/models.py:12-21, i.e.
sklearn's one-vs-rest `LogisticRegression.predict_proba`): reflect-pad X by `ctx` SNPs, window i = padded columns [i M, i M + M + 2 ctx)
(the last window runs to the end), t = X_w . c + b per class, s = 1 / (1 + e^-t), B = s / sum_a s.  Restated here twice:

 * `exact_t`: the logit as the EXACTLY rounded sum (math.fsum over the terms c_k x_k and b; a term is made exact by entering x bit by
   bit, c 2^b is a power-of-two multiple), kept to ~100 bits as t64 + residual in numpy.longdouble.  The reflection is done on X.
 * `fixed_point_t`: the arithmetic the integer kernels DOCUMENT (k_base_logistic_i8.hip:1-18, gnx_model_build.hip `gnx_build_lr`):
   reflections folded into the weights in float64, q = rint(c 2^f_w) with f_w = 53 - ilogb(max |c| of the window), the integer sum
   in Python integers, ONE rounding to float64, then the float64 addition of the intercept.  The kernels claim exactly this t.

`proba` is the sigmoid and row normaliser in numpy.longdouble (64-bit mantissa on x86).  `bound_B` derives how far a kernel's B may be
from `proba(exact_t)`.
"""
import math

import numpy as np

LD = np.longdouble
ULP = 2.0 ** -53          # unit roundoff of float64


def pad(X, ctx):
    """Base.pad (base.py:41-44)"""
    X = np.asarray(X)
    return np.concatenate([X[:, :ctx][:, ::-1], X, X[:, X.shape[1] - ctx:][:, ::-1]], axis=1) if ctx else X


def windows(C, M, ctx):
    """[(first padded column, width)] per window (base.py:157-164): W = C // M windows, the last one takes the remainder"""
    W, M_ = C // M, M + 2 * ctx
    rem = C - M * W
    return [(i * M, M_) for i in range(W - 1)] + [(C + 2 * ctx - (M_ + rem), M_ + rem)]


def _exact_terms(Xw, c):
    """(N, n) integers and (n,) float64 -> (N, n * bits) float64 whose sum is sum_k c_k x_k and whose every element is exact:
    x = sign * sum_b 2^b enters as the terms sign * c * 2^b (x = 3: 2c and c)"""
    Xw = Xw.astype(np.int64)
    mag, sgn = np.abs(Xw), np.sign(Xw).astype(np.float64)
    out = []
    for b in range(8):
        m = (mag >> b) & 1
        if m.any():
            out.append(m * sgn * (c * float(1 << b))[None, :])
    return np.concatenate(out, axis=1) if out else np.zeros((Xw.shape[0], 1))


def exact_t(X, M, ctx, coef, intercept):
    """-> t (N, W, A) longdouble: sum_k c_k x_k + b to ~2^-100 relative; Z64 (N, W, A): the sum without b, rounded once;
    absum (N, W, A): sum_k |c_k x_k| (float64, for the dot-product bound)"""
    X = np.asarray(X)
    N, C = X.shape
    W, A = intercept.shape
    Xp = pad(X, ctx)
    t = np.zeros((N, W, A), LD)
    Z64 = np.zeros((N, W, A))
    absum = np.zeros((N, W, A))
    for w, (lo, n) in enumerate(windows(C, M, ctx)):
        Xw = Xp[:, lo:lo + n]
        for a in range(A):
            c = np.asarray(coef[w, a, :n], np.float64)
            T = _exact_terms(Xw, c)
            absum[:, w, a] = np.abs(T).sum(axis=1)
            b = float(intercept[w, a])
            for r in range(N):
                terms = T[r].tolist()
                Z64[r, w, a] = math.fsum(terms)
                hi = math.fsum(terms + [b])
                t[r, w, a] = LD(hi) + LD(math.fsum(terms + [b, -hi]))
    return t, Z64, absum


def proba(t):
    """s = 1 / (1 + e^-t), B = s / sum s (sklearn's _predict_proba_lr) in longdouble; NaN where every class underflows, as there"""
    t = np.asarray(t, LD)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = LD(1) / (LD(1) + np.exp(-t))
        return s / s.sum(axis=-1, keepdims=True)


def proba_clamped(t, cap=708.0):
    """the kernels' documented expression (gnx_exp.h): -t capped at 708 before the exponential, in longdouble"""
    t = np.asarray(t, LD)
    s = LD(1) / (LD(1) + np.exp(np.minimum(-t, LD(cap))))
    return s / s.sum(axis=-1, keepdims=True)


def folded_weights(C, M, ctx, coef):
    """per window: (first real SNP j0, Wf (A, nj) float64, nfold): the weights of the real SNPs [j0, j0 + nj) with the reflected
    columns added in, in float64 and in the order gnx_build_lr adds them (left reflection, direct, right reflection = ascending
    padded column), and how many of them are sums of more than one column"""
    out = []
    for w, (lo, n) in enumerate(windows(C, M, ctx)):
        p = np.arange(lo, lo + n)
        j = np.where(p < ctx, ctx - 1 - p, np.where(p >= C + ctx, 2 * C + ctx - 1 - p, p - ctx))
        j0, j1 = int(j.min()), int(j.max()) + 1
        A = coef.shape[1]
        Wf = np.zeros((A, j1 - j0))
        cnt = np.zeros(j1 - j0, np.int64)
        for k in range(n):               # ascending padded column: the same order of float64 additions as the model build
            Wf[:, j[k] - j0] += coef[w, :, k]
            cnt[j[k] - j0] += 1
        out.append((j0, Wf, int((cnt > 1).sum())))
    return out


def window_exponent(Wf):
    """e_w = ilogb(max |folded weight|) of a window (None: every weight is zero)"""
    m = float(np.max(np.abs(Wf))) if Wf.size else 0.0
    return None if m == 0.0 else math.frexp(m)[1] - 1


def quantise(Wf):
    """-> (q: object array of Python integers = rint(c 2^f_w), half to even; f_w).  c 2^f_w is exact (a scaling by a power of two
    of a value that stays a normal number or becomes one below 1/2 ulp of the grid), numpy's rint rounds half to even like llrint."""
    e = window_exponent(Wf)
    f = 0 if e is None else 53 - e
    q = np.rint(np.ldexp(Wf, f))
    return np.vectorize(int, otypes=[object])(q) if q.size else q.astype(object), f


def fixed_point_t(X, M, ctx, coef, intercept):
    """t (N, W, A) float64 exactly as the integer kernels define it: fl(fl(S 2^-f_w) + b), S = sum_j x_j q_j an integer"""
    X = np.asarray(X)
    N, C = X.shape
    W, A = intercept.shape
    t = np.zeros((N, W, A))
    for w, (j0, Wf, _) in enumerate(folded_weights(C, M, ctx, coef)):
        q, f = quantise(Wf)
        S = X[:, j0:j0 + Wf.shape[1]].astype(object) @ q.T          # (N, A) Python integers
        for r in range(N):
            for a in range(A):
                t[r, w, a] = math.ldexp(float(S[r, a]), -f) + float(intercept[w, a])
    return t


def bound_B(X, M, ctx, coef, intercept, kind, Z64=None, absum=None):
    """How far a kernel's B may be from proba(exact_t(...)): an array (N, W, A), derived, not measured.

    Let t be the exact logit and t' a kernel's, |t' - t| <= delta.  s = 1 / (1 + e^-t) has ds/dt = s (1 - s), so |ds| <= s delta to
    first order (all deltas here are << 1), and for p_a = s_a / sum s:  |dp_a| <= p_a (delta_a + max_b delta_b) <= 2 max delta.
    The epilogue after t (exp within 2 ulp — tests/test_exp_sc_host.py —, 1 + e, two reciprocals within 1 ulp each, the A-term sum,
    one product) adds relative errors of a few ulp to p <= 1: 8 ulp is allowed, as the issue of this test module sets it.  So

        |dB| <= 2 max_a delta(n, w, a) + 8 * 2^-53.

    delta for the INTEGER kernels (kind "int"), e_w = ilogb(max |folded weight| of the window), xmax = max |x|:
        n_w xmax 2^(e_w - 54)      quantisation: |c - q 2^-f_w| <= half a grid step 2^-f_w = 2^(e_w - 53), over n_w SNPs
      + n_fold xmax 2^(e_w - 53)   the float64 addition that folds a reflected column into a weight |c| < 2^(e_w + 1): 1/2 ulp each
      + |Z| 2^-53                  the single rounding of combine()
      + |t| 2^-53                  the float64 addition of the intercept
    (the last term is not in the issue's formula, which stops at Z: at |t| ~ 700 it is 8e-14, the largest term of the saturation
    cases; the exact reference carries t to 2^-100, so the kernel's own rounding of Z + b has to be allowed for).
    delta for the FLOAT64 MFMA kernel (kind "f64"): the dot product of n_w terms in any order, n_w 2^-53 sum |c_k x_k| (Higham,
    Accuracy and Stability, 3.1, gamma_n ~ n u), the same folding term and the same last term.
    """
    X = np.asarray(X)
    N, C = X.shape
    W, A = intercept.shape
    xmax = float(np.max(np.abs(X.astype(np.int64)))) if X.size else 0.0
    if Z64 is None or absum is None:
        _, Z64, absum = exact_t(X, M, ctx, coef, intercept)
    tabs = np.abs(Z64 + intercept[None])
    delta = np.zeros((N, W, A))
    for w, (j0, Wf, nfold) in enumerate(folded_weights(C, M, ctx, coef)):
        e = window_exponent(Wf)
        g = 0.0 if e is None else math.ldexp(1.0, e - 53)     # one grid step of the window = 1 ulp of its largest weight
        n_w = Wf.shape[1]
        fold = nfold * xmax * g
        if kind == "ref":      # the reference itself: BLAS dot product on the padded X (nothing folded) + the intercept
            delta[:, w, :] = n_w * ULP * absum[:, w, :] + tabs[:, w, :] * ULP
        elif kind == "int":
            delta[:, w, :] = n_w * xmax * g / 2 + fold + np.abs(Z64[:, w, :]) * ULP + tabs[:, w, :] * ULP
        else:
            delta[:, w, :] = n_w * ULP * absum[:, w, :] + fold + tabs[:, w, :] * ULP
    return 2.0 * delta.max(axis=-1, keepdims=True) + 8 * ULP + np.zeros((N, W, A))


def epilogue_ulps(A):
    """relative error of B against proba(t) for a kernel that has t EXACTLY, in units of u = 2^-53 (a result "within k ulp" is within
    2 k u in relative terms, a correctly rounded operation within u): exp within 2 ulp (4.5e-16, tests/test_exp_sc_host.py) 4.05,
    1 + e 1, reciprocal within 1 ulp 2 -> 7.05 per s; the sum of A of them 7.05 + (A - 1); its reciprocal 2; the product 1; and
    one more for the second-order terms:  18.1 + A"""
    return 7.05 + 7.05 + (A - 1) + 2 + 1 + 1 + 1
