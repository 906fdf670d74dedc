"""Inputs, the shape grid and the oracle-side arithmetic of the CRF trainer's edge tests (tests/test_train_crf_cases_host.py,
tests/test_gpu_train_crf_edges.py).  Not a test.

The sizes the grid is chosen by (csrc/k_train_crf.hip): k_crf_eval<KP> holds KP = 1 / 4 / 16 (attribute, label) and (from, to)
pairs per lane for A * A <= 64 / <= 256 / <= 1024, i.e. A <= 8 / <= 16 / <= 32; a block is 4 waves = 4 sequences (the waves past N
alias sequence N - 1); the potential and score loops stride W by the 64 lanes; the backward pass prefetches the operands of window
t - 2; k_crf_reduce1 sums chunks of 32 sequences."""
import numpy as np

# (N, W, A)
KP_CASES = [(9, 7, 8), (9, 7, 9), (9, 7, 16), (9, 7, 17), (9, 7, 32), (5, 6, 2)]                    # <1> <4> <4> <16> <16> <1>
CHAIN_CASES = [(6, 1, 3), (6, 1, 17), (6, 2, 9), (6, 3, 9), (5, 64, 4), (5, 65, 4), (3, 130, 20)]   # <1> <16> <4> <4> <1> <1> <16>
BLOCK_CASES = [(1, 5, 3), (3, 5, 3), (4, 5, 3), (5, 5, 3), (32, 4, 5), (33, 4, 5), (65, 4, 17)]     # <1> x 6, <16>
GRID = KP_CASES + CHAIN_CASES + BLOCK_CASES
F32_CASES = [(9, 7, 17), (33, 4, 5), (6, 1, 3)]                                                     # <16> <1> <1>
C2_CASES = [(9, 7, 9), (9, 7, 17)]                                                                  # <4> <16>
C2S = (1e-6, 0.01, 10.0)
FAR_CASES = [(7, 400, 5), (7, 133, 12)]                                                             # <1> <4>
FAR_SCALES = (5.0, 20.0)
LABEL_CASES = [(12, 7, 5), (12, 7, 17)]                                                             # <1> <16>
LABEL_KINDS = ("label_absent", "constant_sequence", "constant_set", "b_onehot", "b_uniform")


def kp(A):
    """pairs per lane of the k_crf_eval instantiation that A selects"""
    return 1 if A * A <= 64 else 4 if A * A <= 256 else 16


def tracts(rng, N, W, A, noise=0.6):
    """tests/test_train_crf.py's _tracts restated: label tracts with a 12 % switch rate per window, the first sequences constant
    (one label each, so that labels occur), B = Dirichlet noise plus a uniform bump on the label's attribute, renormalised.
    _tracts makes the first A sequences constant and needs N >= A; here it is the first min(A, N // 2), which is the same set
    wherever N >= 2 A and leaves sequences that change label in the cases with fewer sequences than labels."""
    y = np.empty((N, W), np.int32)
    for i in range(N):
        a = rng.randint(A)
        for w in range(W):
            if rng.rand() < 0.12:
                a = rng.randint(A)
            y[i, w] = a
    k = min(A, N // 2)
    y[:k, :] = np.arange(k)[:, None]
    B = rng.dirichlet(np.ones(A) * noise, size=(N, W))
    B[np.arange(N)[:, None], np.arange(W)[None, :], y] += rng.random_sample((N, W))
    return B / B.sum(-1, keepdims=True), y


def case(N, W, A, dtype=np.float64, kind=None):
    """-> B (N, W, A) dtype, y (N, W) int32, state0, trans0 ~ N(0, 0.5) (A, A) float64; one fixed seed per (N, W, A).
    kind (LABEL_KINDS): label_absent — label 2 never occurs (its windows get label 3); constant_sequence — every sequence keeps its
    first label; constant_set — every label is 1; b_onehot — B is exactly 1.0 at its largest attribute and 0.0 elsewhere, as a forest
    base emits it; b_uniform — B is 1 / A everywhere"""
    rng = np.random.RandomState(100000 * N + 100 * W + A)
    B, y = tracts(rng, N, W, A)
    st0, tr0 = rng.normal(0, 0.5, (A, A)), rng.normal(0, 0.5, (A, A))
    if kind == "label_absent":
        y[y == 2] = 3
    elif kind == "constant_sequence":
        y[:, :] = y[:, :1]
    elif kind == "constant_set":
        y[:, :] = 1
    elif kind == "b_onehot":
        B = (np.arange(A)[None, None, :] == np.argmax(B, -1)[:, :, None]).astype(np.float64)
    elif kind == "b_uniform":
        B = np.full((N, W, A), 1.0 / A)
    elif kind is not None:
        raise ValueError(kind)
    return np.ascontiguousarray(B.astype(dtype)), np.ascontiguousarray(y), st0, tr0


def far_start(N, W, A, s):
    """weights far beyond a trained model's O(3): state0, trans0 ~ N(0, 1) * s"""
    rng = np.random.RandomState(7 + 100000 * N + 100 * W + A)
    return rng.normal(0, 1.0, (A, A)) * s, rng.normal(0, 1.0, (A, A)) * s


def unit(gs, gt):
    """the gradient as one unit vector over the 2 A^2 entries, state then trans"""
    g = np.concatenate([np.asarray(gs).ravel(), np.asarray(gt).ravel()])
    return g / np.sqrt(np.sum(g * g))


def mutations(gs, gt):
    """what an indexing slip in the kernel would return instead of (gs, gt): (attribute, label) as (label, attribute), (from, to) as
    (to, from), the two halves exchanged -> {name: unit vector}"""
    return {"state_transposed": unit(gs.T, gt), "trans_transposed": unit(gs, gt.T), "halves_swapped": unit(gt, gs)}


def direction_bound(w0, w1):
    """the bar on max|u - v|, u = (w0 - w1) / |w0 - w1|: the gradient's 1e-9 plus the rounding of w1 = w0 + step d and of w0 - w1
    (a few ulp of the larger weight, relative to the length of the step; zero at w0 = 0)"""
    return 1e-9 + 4.0 * 2.0 ** -53 * np.max(np.abs(w0)) / np.sqrt(np.sum((w0 - w1) ** 2))


def crf_objective_longdouble(B, y, state, trans, c2):
    """oracle.crf_objective's log-space recursion restated in np.longdouble (x87 extended: 64-bit significand): the arbiter where
    float64 results disagree -> f, g_state, g_trans (longdouble)"""
    L = np.longdouble

    def lse(a, axis):
        m = np.max(a, axis=axis, keepdims=True)
        return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))
    X = np.asarray(B, dtype=np.float64).astype(L)
    y = np.asarray(y).astype(np.int64)
    state, trans, c2 = np.asarray(state, dtype=np.float64).astype(L), np.asarray(trans, dtype=np.float64).astype(L), L(c2)
    N, W, A = X.shape
    s = np.einsum("nta,al->ntl", X, state)          # matmul of longdouble goes through object loops in some numpy builds
    la, lb = np.empty_like(s), np.zeros_like(s)
    la[:, 0] = s[:, 0]
    for t in range(1, W):
        la[:, t] = s[:, t] + lse(la[:, t - 1][:, :, None] + trans[None], 1)
    for t in range(W - 2, -1, -1):
        lb[:, t] = lse(trans[None] + (s[:, t + 1] + lb[:, t + 1])[:, None, :], 2)
    logz = lse(la[:, W - 1], 1)
    score = np.take_along_axis(s, y[:, :, None], axis=2)[:, :, 0].sum(1) + trans[y[:, :-1], y[:, 1:]].sum(1)
    onehot = (np.arange(A)[None, None, :] == y[:, :, None]).astype(L)
    g_state = np.einsum("nta,ntl->al", X, np.exp(la + lb - logz[:, None, None]) - onehot)
    g_trans = np.zeros((A, A), L)
    for t in range(1, W):
        g_trans += np.exp(la[:, t - 1][:, :, None] + trans[None] + (s[:, t] + lb[:, t])[:, None, :] - logz[:, None, None]).sum(0)
    np.subtract.at(g_trans, (y[:, :-1].ravel(), y[:, 1:].ravel()), L(1))
    f = np.sum(logz - score) + c2 * (np.sum(state * state) + np.sum(trans * trans))
    return f, g_state + 2 * c2 * state, g_trans + 2 * c2 * trans
