"""Inputs, grids, references and the bound of the CRF smoother's edge tests (tests/test_crf_smooth_cases_host.py,
tests/test_gpu_crf_smooth_edges.py).  Not a test.

The sizes the grids are chosen by (csrc/k_smooth_crf.hip): up to 16 labels a haplotype is one 16-lane DPP row whose label vector is
padded to 8, 12 or 16 (switches at 8 | 9, 12 | 13, 16 | 17); k_crf_psi is instantiated exactly for 2..8, 12 and 16 labels and
generically below 16, 24 and 32; k_smooth_crf_lanes packs 64 / A haplotypes into a wave (4, 3, 2 for 16, 17..21, 22..32 labels).  The
default kernel (k_smooth_crf_ck) works in segments of 8 windows, of which the ones with 0 < t0 and t0 + 8 < W take a path of their own;
k_smooth_crf_row16 pipelines by 8 windows, the lanes kernel by 4, k_crf_scan by chunks of 4 through a three-slot ring.  A block is 4
haplotypes (default), 16 (four-wave blocks, row16), 64 (scan) or 4 * (64 / A) (lanes).  gnx_build_crf picks the default kernel's
forward-scale interval 8 / 4 / 2 / 1 from r = max|state| + max|trans| at 37.5 / 75 / 150."""
import functools

import numpy as np

LD = np.longdouble

# ---- the kernel variants: environment knobs of a context -------------------------------------------------------------------------
KNOBS = ("GNX_CRF_FLAGS", "GNX_CRF_NWB", "GNX_CRF_IMPL")
VARIANTS = {
    "ck": {},
    "ck_psi": {"GNX_CRF_FLAGS": "4"},
    "ck_nwb4": {"GNX_CRF_NWB": "4"},
    "ck_psi_nwb4": {"GNX_CRF_FLAGS": "4", "GNX_CRF_NWB": "4"},
    "row": {"GNX_CRF_FLAGS": "2"},
    "row_fused": {"GNX_CRF_FLAGS": "1"},
    "scan": {"GNX_CRF_IMPL": "scan"},
    "lanes": {"GNX_CRF_IMPL": "lanes"},
}


def resolves_to(variant, A):
    """the kernel gnx_launch_smooth_crf runs for a context of `variant` at A labels"""
    if A > 16:
        return "lanes"
    if variant == "scan" and A > 8:
        return "ck"
    return variant


# ---- grids: (N, W, A) ------------------------------------------------------------------------------------------------------------
LABEL_CASES = [(5, 19, A) for A in (2, 3, 7, 8, 9, 12, 13, 15, 16, 17, 20, 24, 25, 32)]
CHAIN_CASES = [(5, W, A) for A in (5, 12) for W in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33)]
BLOCK_CASES = [(1, 9, 12), (3, 9, 12), (4, 9, 12), (5, 9, 12), (15, 9, 12), (16, 9, 12), (17, 9, 12), (63, 9, 4), (64, 9, 4), (65, 9, 4),
               (11, 9, 20), (12, 9, 20), (13, 9, 20), (35, 9, 7), (36, 9, 7), (37, 9, 7)]
THRESHOLDS = (37.5, 75.0, 150.0)
# (N, W, A, target r, just above it, B rows sum to 2)
THRESHOLD_CASES = [(6, W, A, r, above, False) for A in (5, 12) for W in (24, 25) for r in THRESHOLDS for above in (False, True)]
THRESHOLD_CASES.append((6, 25, 12, 37.5, False, True))
FAR_SCALES = (5.0, 20.0, 40.0)
FAR_CASES = [(7, 61, 5, s) for s in FAR_SCALES] + [(7, 133, 12, s) for s in FAR_SCALES]
F32_CASES = [(5, 19, 7), (5, 19, 12), (5, 19, 20), (5, 8, 5), (5, 8, 12), (5, 17, 5), (5, 17, 12)]
ENUM_CASES = [(3, 9, 2), (3, 5, 3), (3, 4, 4)]          # (A, W) = (2, 9), (3, 5), (4, 4): at most 512 paths
TIE_N, TIE_W = 5, 19
EPS = 1e-9
# (kind, A, j, k, sign): j, k the two columns of `duplicate` / `low_word`
TIE_CASES = ([("uniform", A, 0, 0, 0) for A in (2, 7, 12, 16, 20)]
             + [("duplicate", 12, 0, 1, 0), ("duplicate", 12, 3, 9, 0), ("duplicate", 12, 10, 11, 0), ("duplicate", 20, 17, 19, 0)]
             + [("low_word", A, j, k, s) for (A, j, k) in ((7, 2, 5), (12, 3, 9), (20, 17, 19)) for s in (+1, -1)]
             + [(kind, A, 0, 0, 0) for kind in ("dead", "b_onehot", "b_uniform") for A in (5, 12, 20)])
DEAD_ROW = -800.0
PAIR_BONUS = 3.0

# the cases as ids: ("label" | "chain" | "block" | "f32", N, W, A), ("thr", N, W, A, r, above, two), ("far", N, W, A, s),
# ("tie", kind, A, j, k, sign)
GRID_IDS = ([("label",) + c for c in LABEL_CASES] + [("chain",) + c for c in CHAIN_CASES] + [("block",) + c for c in BLOCK_CASES])
THRESHOLD_IDS = [("thr",) + c for c in THRESHOLD_CASES]
FAR_IDS = [("far",) + c for c in FAR_CASES]
F32_IDS = [("f32",) + c for c in F32_CASES]
TIE_IDS = [("tie",) + c for c in TIE_CASES]
ALL_IDS = GRID_IDS + THRESHOLD_IDS + FAR_IDS + F32_IDS + TIE_IDS


def name(cid):
    return "-".join(("%g" % v) if isinstance(v, float) else str(int(v)) if isinstance(v, (bool, np.bool_)) else str(v) for v in cid)


def shape(cid):
    """-> N, W, A"""
    if cid[0] == "tie":
        return TIE_N, TIE_W, cid[2]
    return cid[1], cid[2], cid[3]


def trained_weights(rng, A):
    """tests/test_gpu_parity.py's weights: the range of a trained model"""
    return rng.standard_normal((A, A)) * 2 + 4 * np.eye(A), rng.standard_normal((A, A)) * 0.5 + 3 * np.eye(A)


def _seed(tag, N, W, A):
    return (tag * 7919 + 100003 * N + 1009 * W + A) % (2 ** 31)


def set_r(state, trans, r, above):
    """state and trans rescaled so that max|state| + max|trans|, summed as gnx_build_crf sums them, is exactly r, or the next double
    above it: both maxima are put at r / 2 (an exact halving), then the transition maximum is raised by the one step"""
    half = r / 2
    state, trans = state * (half / np.max(np.abs(state))), trans * (half / np.max(np.abs(trans)))
    i, j = np.unravel_index(np.argmax(np.abs(state)), state.shape), np.unravel_index(np.argmax(np.abs(trans)), trans.shape)
    state[i] = np.copysign(half, state[i])
    want = np.nextafter(r, np.inf) if above else r
    trans[j] = np.copysign(want - half, trans[j])
    state, trans = np.clip(state, -half, half), np.clip(trans, -abs(trans[j]), abs(trans[j]))
    assert builder_r(state, trans) == want
    return state, trans


def builder_r(state, trans):
    """r as gnx_build_crf computes it: the two running maxima of fabs, added in float64"""
    smax = tmax = 0.0
    for v in np.asarray(state, np.float64).ravel():
        smax = max(smax, abs(float(v)))
    for v in np.asarray(trans, np.float64).ravel():
        tmax = max(tmax, abs(float(v)))
    return smax + tmax


def norm_mask(state, trans):
    """gnx_build_crf's choice: windows between two forward scales of the default kernel, minus one"""
    r = builder_r(state, trans)
    return 0 if not r <= 150.0 else 7 if r <= 37.5 else 3 if r <= 75.0 else 1


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """-> B (N, W, A), state, trans (A, A) float64 (B float32 for the "f32" cases), read-only; one fixed seed per case"""
    kind = cid[0]
    N, W, A = shape(cid)
    if kind in ("label", "chain", "block", "f32"):
        rng = np.random.RandomState(_seed(1, N, W, A))
        B = rng.dirichlet(np.ones(A) * 0.5, size=(N, W))
        state, trans = trained_weights(rng, A)
        if kind == "f32":
            B = B.astype(np.float32)
    elif kind == "thr":
        _, _, _, _, r, above, two = cid
        rng = np.random.RandomState(_seed(2 + int(r) + int(above), N, W, A))
        B = rng.dirichlet(np.ones(A) * 0.5, size=(N, W))
        if two:
            B = B * 2.0
        state, trans = set_r(rng.standard_normal((A, A)), rng.standard_normal((A, A)), r, above)
    elif kind == "far":
        s = cid[4]
        rng = np.random.RandomState(_seed(3 + int(s), N, W, A))
        B = rng.dirichlet(np.ones(A) * 0.5, size=(N, W))
        state, trans = rng.standard_normal((A, A)) * s, rng.standard_normal((A, A)) * s
    elif kind == "tie":
        B, state, trans = _tie_inputs(*cid[1:])
    else:
        raise ValueError(cid)
    out = (np.ascontiguousarray(B), np.ascontiguousarray(state, dtype=np.float64), np.ascontiguousarray(trans, dtype=np.float64))
    for a in out:
        a.setflags(write=False)
    return out


def dead_windows(N, W):
    """the one window per haplotype at which the `dead` case's potentials all underflow: mid-chain, on both sides of a segment edge"""
    return W // 2 - 1 + np.arange(N) % 3


def _tie_inputs(kind, A, j, k, sign):
    N, W = TIE_N, TIE_W
    rng = np.random.RandomState(_seed(11 + 3 * j + k + (sign < 0), N, W, A))
    B = rng.dirichlet(np.ones(A) * 0.5, size=(N, W))
    state, trans = trained_weights(rng, A)
    if kind == "uniform":
        state, trans = np.zeros((A, A)), np.zeros((A, A))
    elif kind in ("duplicate", "low_word"):
        trans = np.zeros((A, A))
        state[:, j] += PAIR_BONUS
        state[:, k] = state[:, j] + (sign * EPS if kind == "low_word" else 0.0)
    elif kind == "dead":
        a0 = A // 2
        state[a0, :] = DEAD_ROW
        a = rng.randint(A - 1, size=(N, W))
        a[a >= a0] += 1                                   # any attribute but a0 ...
        a[np.arange(N), dead_windows(N, W)] = a0          # ... except at the haplotype's dead window
        B = (np.arange(A)[None, None, :] == a[:, :, None]).astype(np.float64)
    elif kind == "b_onehot":
        B = (np.arange(A)[None, None, :] == np.argmax(B, -1)[:, :, None]).astype(np.float64)
    elif kind == "b_uniform":
        B = np.full((N, W, A), 1.0 / A)
    else:
        raise ValueError(kind)
    return B, state, trans


# ---- references ------------------------------------------------------------------------------------------------------------------
def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def marginals_longdouble(B, state, trans):
    """The arbiter: forward-backward in log space in np.longdouble (x87 extended, 64-bit significand), nothing scaled and nothing
    exponentiated before the end -> marginals (N, W, A) longdouble, labels (N, W) int64 (first maximum)"""
    X = np.asarray(B).astype(np.float64).astype(LD)       # float32 inputs: the widened values, as the kernels read them
    state, trans = np.asarray(state, dtype=np.float64).astype(LD), np.asarray(trans, dtype=np.float64).astype(LD)
    N, W, A = X.shape
    s = np.einsum("nta,al->ntl", X, state)                # matmul of longdouble goes through object loops in some numpy builds
    la, lb = np.empty_like(s), np.zeros_like(s)
    la[:, 0] = s[:, 0]
    for t in range(1, W):
        la[:, t] = s[:, t] + _lse(la[:, t - 1][:, :, None] + trans[None], 1)
    for t in range(W - 2, -1, -1):
        lb[:, t] = _lse(trans[None] + (s[:, t + 1] + lb[:, t + 1])[:, None, :], 2)
    logz = _lse(la[:, W - 1], 1)
    p = np.exp(la + lb - logz[:, None, None])
    return p, np.argmax(p, -1).astype(np.int64)


def marginals_enumerated(B, state, trans):
    """Marginals by brute force: exp(score) summed over all A^W label paths, in 60-digit arithmetic.  Shares no recurrence with
    anything else; for the tiny chains only -> (N, W, A) longdouble"""
    import itertools

    import mpmath
    B, state, trans = np.asarray(B, np.float64), np.asarray(state, np.float64), np.asarray(trans, np.float64)
    N, W, A = B.shape
    assert A ** W <= 1024
    out = np.empty((N, W, A), LD)
    with mpmath.workdps(60):
        th = [[mpmath.mpf(float(state[a, y])) for y in range(A)] for a in range(A)]
        ta = [[mpmath.mpf(float(trans[x, y])) for y in range(A)] for x in range(A)]
        for n in range(N):
            s = [[mpmath.fsum(th[a][y] * mpmath.mpf(float(B[n, t, a])) for a in range(A)) for y in range(A)] for t in range(W)]
            z = mpmath.mpf(0)
            m = [[mpmath.mpf(0)] * A for _ in range(W)]
            for path in itertools.product(range(A), repeat=W):
                sc = mpmath.fsum([s[t][path[t]] for t in range(W)] + [ta[path[t - 1]][path[t]] for t in range(1, W)])
                e = mpmath.exp(sc)
                z += e
                for t in range(W):
                    m[t][path[t]] = m[t][path[t]] + e
            for t in range(W):
                for y in range(A):
                    # 60 digits -> longdouble through two float64 halves (numpy takes no mpf)
                    q = m[t][y] / z
                    hi = float(q)
                    out[n, t, y] = LD(hi) + LD(float(q - mpmath.mpf(hi)))
    return out


def bound(W, A, state, trans):
    """First-order bound on max|p - true marginal| of a float64 scaled forward-backward pass, u = 2^-53:
        2 W (A (1 + r) + 4) u,   r = max|state| + max|trans|.
    Per window and direction the recurrence rounds at most A + 4 times (the A products and partial sums of a label's row product, the
    product with psi, the row sum, its reciprocal and the scaling); psi_t(y) = exp(theta' B) carries the absolute error of the dot
    product, at most A r u for B on the simplex, which exp turns into a relative error of the same size.  Relative errors add up
    linearly over the W windows of each of the two sweeps (first order), the marginal is their product, and marginals are <= 1, so the
    relative error is also the absolute one."""
    r = float(np.max(np.abs(state)) + np.max(np.abs(trans)))
    return 2.0 * W * (A * (1.0 + r) + 4.0) * 2.0 ** -53


def bar(cid):
    """the GPU tests' bar on max|p - reference|: the bound under the project's existing bars, 1e-11 for weights in a trained model's
    range and 1e-9 for the far-range and threshold cases"""
    _, W, A = shape(cid)
    _, state, trans = inputs(cid)
    return min(bound(W, A, state, trans), 1e-9 if cid[0] in ("thr", "far") else 1e-11)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """-> marginals (longdouble), labels, top-two gap (N, W) of the arbiter; computed once per case, shared, read-only"""
    B, state, trans = inputs(cid)
    p, lab = marginals_longdouble(B, state, trans)
    top = np.sort(p, -1)
    gap = (top[..., -1] - top[..., -2]).astype(np.float64)
    for a in (p, lab, gap):
        a.setflags(write=False)
    return p, lab, gap


def comparable(cid):
    """the label comparison rule: windows whose top-two gap in the reference exceeds twice the bound -> (N, W) bool"""
    _, W, A = shape(cid)
    _, state, trans = inputs(cid)
    return reference(cid)[2] > 2.0 * bound(W, A, state, trans)


def pair_wins(cid):
    """`duplicate` / `low_word`: the windows where column j or k holds the reference's maximum, clear of every other label by the
    comparison rule's margin -> (N, W) bool"""
    _, _, A, j, k, _ = cid
    _, W, _ = shape(cid)
    _, state, trans = inputs(cid)
    p = reference(cid)[0]
    others = np.delete(p, [j, k], axis=-1).max(-1)
    return (np.maximum(p[..., j], p[..., k]) - others).astype(np.float64) > 2.0 * bound(W, A, state, trans)


def high_word(x):
    return (np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)
