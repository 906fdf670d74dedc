"""tests/lr_exact.py (the exact host reference of the logistic base pass that tests/test_gpu_lr_numerics.py measures the kernels
against) pinned to the REFERENCE's own Base.predict_proba outputs, G1 and G15 — that is how the helper itself is shown to be right —
and its two restatements (exact sum on the padded X; the kernels' fixed-point arithmetic on folded weights) held to the derived
quantisation bound against each other.  No GPU."""
import numpy as np

from conftest import load_golden
import lr_exact as E


def _golden(name):
    g = load_golden(name)
    return g, int(g["C"]), int(g["M"]), int(g["ctx"])


def test_exact_reference_reproduces_the_references_own_output_G1_G15():
    """allowed difference: the float64 dot-product bound n 2^-53 sum |c_k x_k| plus the rounding of + b on the logit (the reference
    computes X_w @ coef.T + b in float64), doubled by the normaliser, plus 8 ulp for its float64 epilogue (lr_exact.bound_B, "ref")"""
    for name in ("G1_lr.npz", "G15_lr_binary.npz"):
        g, C, M, ctx = _golden(name)
        t, Z64, absum = E.exact_t(g["X"], M, ctx, g["coef"], g["intercept"])
        B = E.proba(t)
        bound = E.bound_B(g["X"], M, ctx, g["coef"], g["intercept"], "ref", Z64, absum)
        err = np.abs((B - g["B"].astype(E.LD)).astype(np.float64))
        print(name, "max err %.3g, max bound %.3g, max err/bound %.3g" % (err.max(), bound.max(), (err / bound).max()))
        assert B.shape == g["B"].shape and np.all(err <= bound)
        assert np.array_equal(np.argmax(B, -1), np.argmax(g["B"], -1))
        assert np.max(np.abs((B.sum(-1) - 1).astype(np.float64))) < 1e-18 * 64


def test_fixed_point_restatement_is_within_the_quantisation_bound_of_the_exact_sum():
    """the arithmetic the integer kernels document (folded float64 weights, q = rint(c 2^f_w), integer sum, one rounding, + b) against
    the exact sum on the reflect-padded X: within delta of lr_exact.bound_B — on a model with a large coefficient in one class, where
    the bound is far above the rounding noise of a float64 dot product (so that a wrong fold, window slice or scale would show)"""
    from gnomix_amd import synth
    C, M, A, ctx = 1237, 100, 5, 70
    d = synth.synthetic_model(C=C, M=M, A=A, S=5, context=ctx, seed=4, smooth=None)
    d.lr_coef[:, 0, 3] = 1000.0
    X = synth.synthetic_X(6, C, seed=1, miss=0.1)
    X[0, :] = 3
    X[1, :] = 0
    t, Z64, absum = E.exact_t(X, M, ctx, d.lr_coef, d.lr_intercept)
    tf = E.fixed_point_t(X, M, ctx, d.lr_coef, d.lr_intercept)
    bound = E.bound_B(X, M, ctx, d.lr_coef, d.lr_intercept, "int", Z64, absum)
    delta = (bound - 8 * E.ULP) / 2
    err = np.abs((tf.astype(E.LD) - t).astype(np.float64))
    assert np.all(err <= delta), (err.max(), delta.max())
    assert np.all(tf[1] == d.lr_intercept)            # a row of zeros: the intercepts, exactly
    # and a fold that is wrong by ONE column is far outside it (the check has teeth)
    coef2 = d.lr_coef.copy()
    coef2[0, :, :ctx] = np.roll(coef2[0, :, :ctx], 1, axis=-1)
    err2 = np.abs((E.fixed_point_t(X, M, ctx, coef2, d.lr_intercept).astype(E.LD) - t).astype(np.float64))
    assert np.any(err2[:, 0] > delta[:, 0])


def test_quantise_rounds_half_to_even_and_keeps_the_window_scale():
    Wf = np.array([[2.0 ** 53, 0.5, 1.5, 2.5, -0.5, -1.5, 0.25, 0.75, -(2.0 ** 54 - 2), 0.0, -0.0, 5e-324]])
    q, f = E.quantise(Wf)
    assert f == 0 and [int(v) for v in q[0]] == [2 ** 53, 0, 2, 2, 0, -2, 0, 1, -(2 ** 54 - 2), 0, 0, 0]
    q, f = E.quantise(Wf * 2.0 ** -70)
    assert f == 70 and int(q[0, 2]) == 2
    q, f = E.quantise(np.zeros((2, 3)))
    assert f == 0 and not q.any()
