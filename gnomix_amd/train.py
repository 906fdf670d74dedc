"""Training on the device.

Tree smoother: `Smoother.train` of `XGB_Smoother` (reference src/Smooth/smooth.py:28-38, src/Smooth/models.py:14-20, called
from Gnomix.train, src/model.py:117) — gnx_train_gbt, histogram gradient boosting with fixed-point sums (k_train_gbt.hip).

Logistic base: the device side of `Base.train` for
`LogisticRegressionBase` (reference src/Base/base.py:104-127, src/Base/models.py:12-21, called from Gnomix.train,
src/model.py:113 and :155).  gnx_train_logistic minimises liblinear's L2-regularised logistic objective for all
W windows x A one-vs-rest problems at once (k_train_lr.hip); this module is the ctypes call and the glue that turns the
result into a GnxModelData / a fresh device model."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .model import GnxModelData


def train_logistic_arrays(X, y, M, context, A, C_reg=3.0, tol=1e-9, max_iter=1000, ctx=None, device=0):
    """X (N, C) int8 {0,1,2}, y (N, W) window labels -> (lr_coef (W, A, ldc) f64, lr_intercept (W, A) f64, info dict).
    Defaults are the reference's (C=3., max_iter=1000); tol is OUR stopping rule |grad| <= tol |grad(0)| (the reference's
    liblinear stops near 1e-4: the default here converges to the optimum it approximates)."""
    ctx = ctx or _lib.default_context(device)
    from . import resident
    on_dev = resident.all_on_device([X, y], "train_logistic_arrays: (X, y)")
    if on_dev:
        # X / y already in HBM (a CUDA int8 tensor with any row stride, int32 labels): gnx_train_logistic_dev reads them in place
        N, Cn = X.shape
        W = Cn // int(M)
        X, y = resident.check_x(X, Cn, ctx.device), resident.check_y(y, N, W, ctx.device)
        lo, hi = (int(v) for v in y.aminmax()) if N else (0, 0)
    else:
        X = np.ascontiguousarray(X, dtype=np.int8)
        N, Cn = X.shape
        W = Cn // int(M)
        y = np.ascontiguousarray(y, dtype=np.int32)
        if y.shape != (N, W):
            raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
        lo, hi = y.min(), y.max()
    if lo < 0 or hi >= A:
        raise ValueError("labels must lie in [0, A)")
    ldc = int(M) + 2 * int(context) + (Cn - int(M) * W)
    coef = np.zeros((W, int(A), ldc), np.float64)
    icpt = np.zeros((W, int(A)), np.float64)
    info = _lib.TrainInfo()
    if on_dev:
        with resident.torch_stream(ctx):
            ctx.check(ctx.lib.gnx_train_logistic_dev(ctx.h, X.data_ptr(), N, resident.row_stride(X), y.data_ptr(), Cn, int(M), int(context),
                                                     int(A), float(C_reg), float(tol), int(max_iter), coef.ctypes.data, ldc,
                                                     icpt.ctypes.data, C.byref(info)))
    else:
        ctx.check(ctx.lib.gnx_train_logistic(ctx.h, X.ctypes.data, N, X.shape[1], y.ctypes.data, Cn, int(M), int(context), int(A),
                                             float(C_reg), float(tol), int(max_iter), coef.ctypes.data, ldc, icpt.ctypes.data, C.byref(info)))
    out = dict(newton_iterations=info.newton_iterations, cg_iterations=info.cg_iterations, n_problems=info.n_problems,
               worst_rel_gradient=info.worst_rel_gradient, objective_sum=info.objective_sum)
    # the library bounds the Newton steps (at most 200 whatever max_iter says: include/gnomix_hip.h) and returns what it has: a
    # window that did not get near liblinear's own stopping level (1e-4) must not pass as a trained model silently
    if info.worst_rel_gradient > max(float(tol), 1e-4):
        import warnings
        warnings.warn("gnx_train_logistic stopped after %d Newton steps with |grad| / |grad(0)| = %.3g on its worst window "
                      "(tol %.3g): the logistic base is not converged" % (info.newton_iterations, info.worst_rel_gradient, tol),
                      RuntimeWarning, stacklevel=2)
    return coef, icpt, out


def train_logistic_base(data: GnxModelData, X, y, **kw) -> dict:
    """fit the logistic base of `data` in place (lr_coef / lr_intercept) -> info"""
    coef, icpt, info = train_logistic_arrays(X, y, data.M, data.context, data.A, **kw)
    data.base_kind, data.lr_coef, data.lr_intercept = "logistic", coef, icpt
    return info


def lr_objective(coef_row, intercept, Xw, ypm, C_reg=3.0):
    """liblinear's primal objective of ONE binary problem: 1/2 (|w|^2 + b^2) + C sum log(1 + exp(-y (w.x + b))) — numpy, for
    tests and for judging a fit against the reference's (the bias is a regularised feature: intercept_scaling = 1)"""
    z = Xw.astype(np.float64) @ coef_row + intercept
    return 0.5 * (float(coef_row @ coef_row) + float(intercept) ** 2) + C_reg * float(np.sum(np.logaddexp(0.0, -ypm * z)))


def train_gbt_arrays(B, y, S, n_rounds=100, max_depth=4, learning_rate=0.1, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0,
                     max_bin=256, base_score=0.5, tree_method="hist", ctx=None, device=0):
    """B (N, W, A) base probabilities of the smoother's training haplotypes (float32 / float64; a CUDA tensor stays on the
    device), y (N, W) labels -> (dict of tree arrays as GnxModelData takes them, losses (n_rounds + 1,)).  Defaults are the
    reference's XGBClassifier arguments (src/Smooth/models.py:14-20).  tree_method: "hist" (max_bin quantile bins per class column) or
    "exact" (xgboost's exact greedy enumeration: a candidate between every two distinct values of a node's rows; slower, and like the
    histogram form not pinned to xgboost's own floating-point trajectory)."""
    if tree_method not in ("hist", "exact"):
        raise ValueError("tree_method is 'hist' or 'exact'")
    ctx = ctx or _lib.default_context(device)
    on_dev = hasattr(B, "is_cuda") and B.is_cuda
    if on_dev:
        import torch
        assert B.is_contiguous() and B.dtype in (torch.float32, torch.float64)
        N, W, A = B.shape
        is64 = B.dtype == torch.float64
        y = y if (hasattr(y, "is_cuda") and y.is_cuda) else torch.as_tensor(np.ascontiguousarray(y, dtype=np.int32), device=B.device)
        assert y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (N, W)
        b_ptr, y_ptr, fn = B.data_ptr(), y.data_ptr(), ctx.lib.gnx_train_gbt_dev
        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    else:
        B = np.ascontiguousarray(B)
        if B.dtype != np.float64:
            B = np.ascontiguousarray(B, dtype=np.float32)
        N, W, A = B.shape
        is64 = B.dtype == np.float64
        y = np.ascontiguousarray(y, dtype=np.int32)
        if y.shape != (N, W):
            raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
        b_ptr, y_ptr, fn = B.ctypes.data, y.ctypes.data, ctx.lib.gnx_train_gbt
    T = int(n_rounds) * int(A)
    # a complete tree of that depth (the library rejects depths outside 1..5 itself: include/gnomix_hip.h, gnx_gbt_params)
    per_tree = 2 ** (min(max(int(max_depth), 1), 5) + 1) - 1
    tree_off = np.zeros(T + 1, np.int32); tree_class = np.zeros(T, np.int32)
    left = np.zeros(T * per_tree, np.int32); right = np.zeros(T * per_tree, np.int32); feat = np.zeros(T * per_tree, np.int32)
    cond = np.zeros(T * per_tree, np.float32); loss = np.zeros(int(n_rounds) + 1, np.float64)
    nn = C.c_int64(0)
    P = _lib.GbtParams(int(n_rounds), int(max_depth), int(max_bin), 1 if tree_method == "exact" else 0, float(learning_rate), float(reg_lambda), float(gamma),
                       float(min_child_weight), float(base_score))
    ctx.check(fn(ctx.h, b_ptr, int(is64), y_ptr, int(N), int(W), int(A), int(S), C.byref(P), tree_off.ctypes.data, tree_class.ctypes.data,
                 left.ctypes.data, right.ctypes.data, feat.ctypes.data, cond.ctypes.data, C.addressof(nn), loss.ctypes.data))
    n = nn.value
    trees = dict(tree_off=tree_off, left=left[:n].copy(), right=right[:n].copy(), feat=feat[:n].copy(), cond=cond[:n].copy(),
                 tree_class=tree_class)
    return trees, loss


def train_gbt_smoother(data: GnxModelData, B, y, **kw) -> np.ndarray:
    """fit the tree smoother of `data` in place (smooth_kind "xgb", tree arrays, base_score) -> losses per round"""
    trees, loss = train_gbt_arrays(B, y, data.S, **kw)
    data.smooth_kind = "xgb"
    for k, v in trees.items():
        setattr(data, k, v)
    data.base_score = float(kw.get("base_score", 0.5))
    return loss


def train_forest_arrays(X, y, M, context, A, n_rounds=20, max_depth=4, learning_rate=0.1, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0,
                        base_score=0.5, ctx=None, device=0):
    """XGBBase's per-window XGBClassifier(n_estimators=20, max_depth=4, learning_rate=0.1, reg_lambda=1, missing=2).fit on the device,
    all windows at once (gnx_train_gbt_base; the algorithm is stated in forest/k_train_gbt_base.hip, NOT pinned to xgboost's own trees).
    X (N, C) int8 codes {0, 1, 2 = missing} — a numpy array, or a CUDA int8 tensor that stays on the device — y (N, W) labels ->
    (dict of fb_* arrays as GnxModelData takes them, losses (n_rounds + 1,))."""
    ctx = ctx or _lib.default_context(device)
    on_dev = hasattr(X, "is_cuda") and X.is_cuda
    if on_dev:
        import torch
        assert X.dtype == torch.int8 and X.dim() == 2 and X.stride(1) == 1
        N, Cn = X.shape
        ldx = X.stride(0) if N > 1 else Cn
        W = Cn // int(M)
        y = y if (hasattr(y, "is_cuda") and y.is_cuda) else torch.as_tensor(np.ascontiguousarray(y, dtype=np.int32), device=X.device)
        assert y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (N, W)
        x_ptr, y_ptr, fn = X.data_ptr(), y.data_ptr(), ctx.lib.gnx_train_gbt_base_dev
        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    else:
        X = np.ascontiguousarray(X, dtype=np.int8)
        N, Cn = X.shape
        ldx = Cn
        W = Cn // int(M)
        y = np.ascontiguousarray(y, dtype=np.int32)
        if y.shape != (N, W):
            raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
        x_ptr, y_ptr, fn = X.ctypes.data, y.ctypes.data, ctx.lib.gnx_train_gbt_base
    T = W * int(n_rounds) * (1 if int(A) == 2 else int(A))
    # a complete tree of that depth (the library rejects depths outside 1..5 itself: include/gnomix_hip.h)
    cap = max(T, 1) * (2 ** (min(max(int(max_depth), 1), 5) + 1) - 1)
    wt0 = np.zeros(W + 1, np.int32); tree_off = np.zeros(max(T, 0) + 1, np.int32); tree_class = np.zeros(max(T, 1), np.int32)
    left = np.zeros(cap, np.int32); right = np.zeros(cap, np.int32); feat = np.zeros(cap, np.int32)
    cond = np.zeros(cap, np.float32); dleft = np.zeros(cap, np.uint8); loss = np.zeros(max(int(n_rounds), 0) + 1, np.float64)
    nn = C.c_int64(0)
    P = _lib.GbtParams(int(n_rounds), int(max_depth), 256, 0, float(learning_rate), float(reg_lambda), float(gamma), float(min_child_weight),
                       float(base_score))
    ctx.check(fn(ctx.h, x_ptr, int(N), int(ldx), y_ptr, int(Cn), int(M), int(context), int(A), C.byref(P), wt0.ctypes.data, tree_off.ctypes.data,
                 left.ctypes.data, right.ctypes.data, feat.ctypes.data, cond.ctypes.data, dleft.ctypes.data, tree_class.ctypes.data,
                 C.addressof(nn), loss.ctypes.data))
    n = nn.value
    trees = dict(fb_win_tree0=wt0, fb_tree_off=tree_off, fb_left=left[:n].copy(), fb_right=right[:n].copy(), fb_feat=feat[:n].copy(),
                 fb_cond=cond[:n].copy(), fb_default_left=dleft[:n].copy(), fb_tree_class=tree_class[:T].copy())
    return trees, loss


def train_forest_base(data: GnxModelData, X, y, **kw) -> np.ndarray:
    """fit the boosted-tree base of `data` in place (base_kind "forest", fb_* arrays, fb_missing = 2, fb_base_score) -> losses per round"""
    trees, loss = train_forest_arrays(X, y, data.M, data.context, data.A, **kw)
    data.base_kind, data.fb_missing = "forest", 2
    data.fb_base_score = float(kw.get("base_score", 0.5))
    for k, v in trees.items():
        setattr(data, k, v)
    return loss


def forest_placeholder(W, A):
    """one stump per window and class (a split on the window's first SNP, two zero leaves): every class gets probability 1 / A"""
    K = 1 if A == 2 else A
    T = W * K
    return dict(fb_win_tree0=(np.arange(W + 1) * K).astype(np.int32), fb_tree_off=(3 * np.arange(T + 1)).astype(np.int32),
                fb_left=np.tile(np.array([1, -1, -1], np.int32), T), fb_right=np.tile(np.array([2, -1, -1], np.int32), T),
                fb_feat=np.zeros(3 * T, np.int32), fb_cond=np.tile(np.array([0.5, 0.0, 0.0], np.float32), T),
                fb_default_left=np.zeros(3 * T, np.uint8), fb_tree_class=(np.arange(T) % K).astype(np.int32))


def cnn_init(A, S, seed=None):
    """nn.Conv1d(A, A, S)'s default initialisation (torch.nn.modules.conv._ConvNd.reset_parameters): kaiming_uniform_(a = sqrt 5)
    on the weight and uniform(+-1/sqrt(fan_in)) on the bias are both uniform(+-1/sqrt(A * S)); numpy's generator, not torch's"""
    rng = np.random.RandomState(seed)
    bound = 1.0 / np.sqrt(A * S)
    return (rng.uniform(-bound, bound, size=(A, A, S)).astype(np.float32), rng.uniform(-bound, bound, size=A).astype(np.float32))


def train_cnn_arrays(B, y, S, weight=None, bias=None, max_ep=250, batch_size=128, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, log_eps=1e-8,
                     shuffle=True, seed=None, order=None, ctx=None, device=0):
    """CNN.fit (src/Smooth/cnn.py:104-118) on the device: B (N, W, A) base probabilities, y (N, W) labels -> (weight (A, A, S),
    bias (A,), per-epoch mean batch loss).  `weight` / `bias` = initial parameters (default: cnn_init(A, S, seed));
    `order` (max_ep, N) = the rows' order in every epoch (default: a fresh permutation per epoch when `shuffle`, as the
    reference's DataLoader(shuffle=True), drawn from numpy's RandomState(seed))."""
    ctx = ctx or _lib.default_context(device)
    B = np.ascontiguousarray(B)
    if B.dtype != np.float64:
        B = np.ascontiguousarray(B, dtype=np.float32)
    N, W, A = B.shape
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.shape != (N, W):
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
    if weight is None or bias is None:
        weight, bias = cnn_init(A, S, seed)
    weight = np.array(weight, dtype=np.float32, order="C")
    bias = np.array(bias, dtype=np.float32, order="C")
    if weight.shape != (A, A, S) or bias.shape != (A,):
        raise ValueError(f"weight / bias must be ({A}, {A}, {S}) / ({A},), got {weight.shape} / {bias.shape}")
    if order is None and shuffle:
        rng = np.random.RandomState(None if seed is None else seed + 1)
        order = np.stack([rng.permutation(N) for _ in range(int(max_ep))]) if max_ep > 0 else np.zeros((0, N), np.int64)
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int64)
        if order.shape != (int(max_ep), N):
            raise ValueError(f"order must be (max_ep, N) = ({int(max_ep)}, {N}), got {order.shape}")
    loss = np.zeros(max(int(max_ep), 1), np.float64)
    P = _lib.CnnParams(int(max_ep), int(batch_size), float(lr), float(betas[0]), float(betas[1]), float(eps), float(log_eps))
    ctx.check(ctx.lib.gnx_train_cnn(ctx.h, B.ctypes.data, int(B.dtype == np.float64), y.ctypes.data, int(N), int(W), int(A), int(S), C.byref(P),
                                    order.ctypes.data if order is not None else None, weight.ctypes.data, bias.ctypes.data, loss.ctypes.data))
    return weight, bias, loss[:int(max_ep)]


def train_cnn_smoother(data: GnxModelData, B, y, **kw) -> np.ndarray:
    """fit the convolutional smoother of `data` in place (smooth_kind "cnn", cnn_weight / cnn_bias) -> losses per epoch"""
    w, b, loss = train_cnn_arrays(B, y, data.S if data.S % 2 else data.S - 1, **kw)
    data.smooth_kind, data.cnn_weight, data.cnn_bias = "cnn", w, b
    return loss


def train_crf_arrays(B, y, c2=1.0, epsilon=1e-8, max_iterations=10000, memory=10, state0=None, trans0=None, ctx=None, device=0):
    """CRF.fit (src/Smooth/crf.py:51-58) on the device: B (N, W, A) base probabilities (the attributes' values), y (N, W) labels ->
    (state (A, A) [attribute][label], trans (A, A) [from][to], info dict).  Minimises CRFsuite's L2-regularised negative
    log-likelihood (c1 = 0, c2 = 1 as sklearn_crfsuite.CRF's defaults) from zeros, like CRFsuite, to a tighter tolerance."""
    ctx = ctx or _lib.default_context(device)
    B = np.ascontiguousarray(B)
    if B.dtype != np.float64:
        B = np.ascontiguousarray(B, dtype=np.float32)
    N, W, A = B.shape
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.shape != (N, W):
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
    state = np.zeros((A, A), np.float64) if state0 is None else np.array(state0, dtype=np.float64, order="C")
    trans = np.zeros((A, A), np.float64) if trans0 is None else np.array(trans0, dtype=np.float64, order="C")
    if state.shape != (A, A) or trans.shape != (A, A):
        raise ValueError(f"state0 / trans0 must be ({A}, {A})")
    P = _lib.CrfParams(0.0, float(c2), float(epsilon), int(max_iterations), int(memory))
    info = _lib.CrfInfo()
    ctx.check(ctx.lib.gnx_train_crf(ctx.h, B.ctypes.data, int(B.dtype == np.float64), y.ctypes.data, int(N), int(W), int(A), C.byref(P),
                                    state.ctypes.data, trans.ctypes.data, C.byref(info)))
    return state, trans, {"iterations": info.iterations, "evaluations": info.evaluations, "objective": info.objective,
                          "grad_norm": info.grad_norm, "converged": bool(info.converged)}


def train_crf_smoother(data: GnxModelData, B, y, **kw) -> dict:
    """fit the CRF smoother of `data` in place (smooth_kind "crf", crf_state / crf_trans) -> info"""
    st, tr, info = train_crf_arrays(B, y, **kw)
    data.smooth_kind, data.crf_state, data.crf_trans = "crf", st, tr
    return info


# ---- the CovRSK SVC base (mode "best") ---------------------------------------------------------------------------------------
SVC_SEED_HIGH = int(np.iinfo("i").max)          # BaseLibSVM.fit: seed = rnd.randint(np.iinfo("i").max)
SVC_KERNEL_KINDS = {"CovRSK": 0, "string_kernel": 2}   # GNX_SVC_KERNEL_SUBSTRINGS (CovSample lengths), GNX_SVC_KERNEL_ALL_LENGTHS
SVC_TRAIN_KINDS = dict(SVC_KERNEL_KINDS, rbf=3, poly_kernel=1)   # + GNX_SVC_KERNEL_RBF (SVMBase), GNX_SVC_KERNEL_POLY (PolynomialStringKernelBase): what train_svc_arrays accepts
SVC_UNCHAINED_KERNELS = ("rbf", "string_kernel", "poly_kernel")  # kernels that leave numpy's global generator alone: one drawn seed per window


def svc_rng_after_kernel(width):
    """numpy's global generator where one CovRSK kernel call on a window of `width` SNPs leaves it: CovSample
    (string_kernel.py:80-89) runs np.random.seed(37), then width - 1 draws"""
    np.random.seed(37)
    if int(width) > 1:
        np.random.rand(int(width) - 1)


def svc_seed_chain(widths, first_seed):
    """libsvm seeds of the reference's sequential window fits (CovRSKBase.train): window 0 uses `first_seed`, drawn from the global
    generator before any kernel call (BaseLibSVM.fit draws it before _compute_kernel); window w >= 1 draws from the state that window
    w-1's kernel call left, RandomState(37) after width_{w-1} - 1 draws -> uint32 (W,)"""
    seeds, memo = [int(first_seed)], {}
    for w in range(1, len(widths)):
        pw = int(widths[w - 1])
        if pw not in memo:
            rs = np.random.RandomState(37)
            if pw > 1:
                rs.random_sample(pw - 1)
            memo[pw] = int(rs.randint(SVC_SEED_HIGH))
        seeds.append(memo[pw])
    return np.asarray(seeds, dtype=np.uint32)


def svc_fold_permutation(seed, l):
    """the Platt fold permutation libsvm draws for an l-row class pair fitted with `seed` (gnx_svc_fold_permutation)"""
    perm = np.empty(max(int(l), 1), np.int32)
    rc = _lib.load().gnx_svc_fold_permutation(int(seed), int(l), perm.ctypes.data)
    if rc != _lib.GNX_OK:
        raise _lib.GnxError(rc, "gnx_svc_fold_permutation: bad length")
    return perm[:int(l)]


def window_columns(C, M, context, w):
    """columns of X that window w reads, in order: base.py's reflect padding (base.py:41-44) and window slicing (:146-164)"""
    W, rem = C // M, C - M * (C // M)
    width = M + 2 * context + (rem if w == W - 1 else 0)
    p = w * M + np.arange(width)
    return np.where(p < context, context - 1 - p, np.where(p < context + C, p - context, C - 1 - (p - context - C)))


def svc_seeds_unchained(W):
    """libsvm seeds for SVMBase's window fits: the reference fits them in spawned workers with unseeded generators
    (base_multithread = True), so there is nothing to reproduce; one seed per window from numpy's global generator, in window
    order, as BaseLibSVM.fit draws it -> uint32 (W,).  StringKernelBase and PolynomialStringKernelBase fit sequentially
    (base_multithread = False) and their kernels never touch the global generator, so these ARE the seeds the reference's fits draw:
    the first W values of RandomState(k).randint(SVC_SEED_HIGH) after np.random.seed(k)."""
    return np.asarray([np.random.randint(SVC_SEED_HIGH) for _ in range(int(W))], dtype=np.uint32)


def train_svc_arrays(X, y, M, context, A, seeds, kernel="CovRSK", ctx=None, device=0, gamma=0.001, C=None, p=1.2):
    """SVC(kernel=<kernel>, probability=True).fit of every window on the device (gnx_train_svc2).  kernel "rbf" is SVMBase's
    SVC(C=100., gamma=0.001) (C defaults to 100 for "rbf" and to sklearn's 1 for the string kernels); "poly_kernel" is
    PolynomialStringKernelBase's poly_kernel(X, Y, p) (gnx_train_svc_poly, with the run values of convert.poly_run_values).
    X (N, C) int8 {0,1,2}, y (N, W)
    labels, seeds (W,) libsvm seeds -> dict of (W, ...) arrays in sklearn's layout (support / dual_coef padded to N columns, n_sv
    valid) and an info dict"""
    import ctypes as ct   # (the libsvm cost parameter of this function is named C, as sklearn's)
    if kernel not in SVC_TRAIN_KINDS:
        raise ValueError(f"kernel must be one of {sorted(SVC_TRAIN_KINDS)}")
    ctx = ctx or _lib.default_context(device)
    X = np.ascontiguousarray(X, dtype=np.int8)
    N, Cn = X.shape
    W = Cn // int(M)
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.shape != (N, W):
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    if seeds.shape != (W,):
        raise ValueError(f"seeds must be (W,) = ({W},), got {seeds.shape}")
    A, P = int(A), int(A) * (int(A) - 1) // 2
    out = dict(n_sv=np.zeros(W, np.int32), n_support=np.zeros((W, A), np.int32), support=np.zeros((W, N), np.int32),
               dual_coef=np.zeros((W, A - 1, N), np.float64), intercept=np.zeros((W, P), np.float64),
               prob_a=np.zeros((W, P), np.float64), prob_b=np.zeros((W, P), np.float64))
    info = _lib.SvcTrainInfo()
    prm = _lib.SvcParams(SVC_TRAIN_KINDS[kernel], 0, float((100.0 if kernel == "rbf" else 1.0) if C is None else C), float(gamma))
    outs = [out[k].ctypes.data for k in ("n_sv", "n_support", "support", "dual_coef", "intercept", "prob_a", "prob_b")]
    if kernel == "poly_kernel":
        from .convert import poly_run_values
        rv = np.ascontiguousarray(poly_run_values(int(M) + 2 * int(context) + Cn % int(M), p)["run_value"], dtype=np.float64)
        ctx.check(ctx.lib.gnx_train_svc_poly(ctx.h, X.ctypes.data, N, Cn, y.ctypes.data, Cn, int(M), int(context), A, ct.byref(prm),
                                            float(p), rv.ctypes.data, len(rv), seeds.ctypes.data, *outs, ct.byref(info)))
    else:
        ctx.check(ctx.lib.gnx_train_svc2(ctx.h, X.ctypes.data, N, Cn, y.ctypes.data, Cn, int(M), int(context), A, ct.byref(prm),
                                        seeds.ctypes.data, *outs, ct.byref(info)))
    return out, dict(smo_iterations=info.smo_iterations, n_solves=info.n_solves, n_guarded=info.n_guarded, gram_ms=info.gram_ms,
                     smo_ms=info.smo_ms, platt_ms=info.platt_ms)


def svc_gram(X, M, context, kernel="CovRSK", p=1.2, w0=0, w1=None, ctx=None, device=0):
    """the float Gram matrices K(Xw, Xw) of windows [w0, w1) as the string-kernel trainers compute them (gnx_svc_gram) ->
    (w1 - w0, N, N) float32.  kernel: "CovRSK", "string_kernel" or "poly_kernel" (with exponent p)"""
    if kernel not in SVC_TRAIN_KINDS or kernel == "rbf":
        raise ValueError("kernel must be \"CovRSK\", \"string_kernel\" or \"poly_kernel\"")
    ctx = ctx or _lib.default_context(device)
    X = np.ascontiguousarray(X, dtype=np.int8)
    N, Cn = X.shape
    w1 = Cn // int(M) if w1 is None else int(w1)
    rv = None
    if kernel == "poly_kernel":
        from .convert import poly_run_values
        rv = np.ascontiguousarray(poly_run_values(int(M) + 2 * int(context) + Cn % int(M), p)["run_value"], dtype=np.float64)
    G = np.zeros((max(w1 - int(w0), 0), N, N), np.float32)
    ctx.check(ctx.lib.gnx_svc_gram(ctx.h, X.ctypes.data, N, Cn, Cn, int(M), int(context), SVC_TRAIN_KINDS[kernel], float(p),
                                  None if rv is None else rv.ctypes.data, 0 if rv is None else len(rv), int(w0), w1, G.ctypes.data))
    return G


def svc_window_kernel(w) -> str:
    """the kernel of a per-window SVC dict, by its tag: "rbf" (SVMBase), "string_kernel" (StringKernelBase), "poly_kernel"
    (PolynomialStringKernelBase); no tag (a converted pickle, an older .gnx) = "CovRSK", whatever lengths it carries"""
    k = str(np.asarray(w["kernel"])) if "kernel" in w else "CovRSK"
    if k not in SVC_TRAIN_KINDS:
        raise ValueError(f"unknown SVC window kernel tag {k!r}")
    return k


def train_svc_base(data: GnxModelData, X, y, ctx=None, seeds=None, kernel="CovRSK", **kw) -> dict:
    """fit the SVC base of `data` in place (data.svc, base_kind "covrsk") -> info: the CovRSK string kernel, or kernel="rbf"
    (SVMBase; gamma=0.001, C=100.0 unless given), kernel="string_kernel" (StringKernelBase: every length) or kernel="poly_kernel"
    (PolynomialStringKernelBase; p=1.2 unless given); the windows of the last three carry the tag `kernel` and one seed per window
    drawn from numpy's global generator when `seeds` is None.  Each window keeps only its support
    rows as `xfit` (support = arange(n_sv)): the full training window would put N x width bytes per window into the .gnx.  The
    sklearn-order support_ indices (rows of X) are info["support"]."""
    from .convert import string_kernel_lengths
    W = data.W
    rbf = kernel == "rbf"
    if seeds is None:
        seeds = (svc_seeds_unchained(W) if kernel in SVC_UNCHAINED_KERNELS else
                 svc_seed_chain([data.window_width(w) for w in range(W)], np.random.randint(SVC_SEED_HIGH)))
    X = np.ascontiguousarray(X, dtype=np.int8)
    res, info = train_svc_arrays(X, y, data.M, data.context, data.A, seeds, kernel=kernel, ctx=ctx, **kw)
    from .convert import poly_run_values

    def extras(width):   # what a window carries besides the fitted arrays: the kernel's tag and parameters
        if rbf:
            return dict(kernel=np.array("rbf"), gamma=np.float64(kw.get("gamma", 0.001)))
        if kernel == "poly_kernel":
            return dict(kernel=np.array("poly_kernel"), **poly_run_values(width, kw.get("p", 1.2)))
        if kernel == "string_kernel":
            return dict(kernel=np.array("string_kernel"), ms=string_kernel_lengths(width, kernel))
        return dict(ms=string_kernel_lengths(width, kernel))
    svc, sup_raw = [], []
    for w in range(W):
        n = int(res["n_sv"][w])
        sup = res["support"][w, :n].copy()
        cols = window_columns(data.C, data.M, data.context, w)
        svc.append(dict(xfit=np.ascontiguousarray(X[sup][:, cols]), support=np.arange(n, dtype=np.int32),
                        dual_coef=np.ascontiguousarray(res["dual_coef"][w, :, :n]), intercept=res["intercept"][w].copy(),
                        prob_a=res["prob_a"][w].copy(), prob_b=res["prob_b"][w].copy(), n_support=res["n_support"][w].copy(),
                        **extras(len(cols))))
        sup_raw.append(sup)
    data.base_kind, data.svc = "covrsk", svc
    info["support"] = sup_raw
    info["seeds"] = np.asarray(seeds, dtype=np.uint32)
    return info


# ---- the 1-nearest-neighbour base (KNNBase) ------------------------------------------------------------------------------------
def train_knn_base(data: GnxModelData, X, y, ctx=None) -> dict:
    """fit the 1-NN base of `data` in place (base_kind "knn") -> info.  KNeighborsClassifier(n_neighbors=1).fit stores its
    training set, so fitting is storing: no training kernel exists or is needed.  Every window's fit rows are the same
    haplotypes, so the model keeps X (n_fit, C) and y (n_fit, W) once (the shared form) and windows are cut when the model is
    loaded.  X must hold the codes 0..2, y labels in [0, A)."""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != data.C or X.shape[0] < 1:
        raise ValueError(f"X must be (N >= 1, C={data.C}), got {X.shape}")
    if X.dtype.kind == "f" and np.any(X != np.rint(X)):
        raise ValueError("X must hold whole numbers (the SNP codes 0, 1, 2)")
    if X.min() < 0 or X.max() > 2:
        raise ValueError("X must hold the SNP codes 0, 1, 2 (2 = missing)")
    y = np.asarray(y)
    if y.shape != (X.shape[0], data.W):
        raise ValueError(f"y must be (N, W) = ({X.shape[0]}, {data.W}), got {y.shape}")
    if y.min() < 0 or y.max() >= data.A:
        raise ValueError(f"y must hold labels in 0..{data.A - 1}")
    data.base_kind, data.knn = "knn", None
    data.knn_X, data.knn_y = np.ascontiguousarray(X, dtype=np.int8), np.ascontiguousarray(y, dtype=np.int32)
    return {"n_fit": int(X.shape[0])}


# ---- the three Naive-Bayes bases (NBBernoulliBase, NBMultinomialBase, NBGaussianBase) -------------------------------------------
NB_TRAIN_KINDS = ("bernoulli", "multinomial", "gaussian")


def nb_counts(X, y, M, context, A, ctx=None, device=0):
    """the integer counts every Naive-Bayes closed form needs, on the device (gnx_train_nb_counts): X (N, C) int8 codes 0..2, y (N, W)
    labels in [0, A) -> n1, n2 (W, A, ldw) int32 (rows of class c whose SNP at window position p is 1 / 2; positions past a window's
    width hold 0) and class_count (W, A) int32"""
    ctx = ctx or _lib.default_context(device)
    X = np.ascontiguousarray(X, dtype=np.int8)
    N, Cn = X.shape
    W = Cn // int(M)
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.shape != (N, W):
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
    ldw = int(M) + 2 * int(context) + Cn - int(M) * W
    n1, n2, cc = np.zeros((W, int(A), ldw), np.int32), np.zeros((W, int(A), ldw), np.int32), np.zeros((W, int(A)), np.int32)
    ctx.check(ctx.lib.gnx_train_nb_counts(ctx.h, X.ctypes.data, N, Cn, y.ctypes.data, Cn, int(M), int(context), int(A), n1.ctypes.data,
                                          n2.ctypes.data, cc.ctypes.data))
    return n1, n2, cc


def nb_fit_from_counts(kind, n1, n2, cc, alpha=1e-10, var_smoothing=1e-9):
    """ONE window's fitted attributes from its counts, by scikit-learn's own expressions (so they come out equal to scikit-learn's):
    n1, n2 (A, width) and cc (A,) integers -> dict with classes_ (the classes that have rows) and, per kind,
      bernoulli:    fc = n1 + n2;    feature_log_prob_ = log(fc + alpha) - log((cc + 2 alpha)[:, None])
      multinomial:  fc = n1 + 2 n2;  sf = fc + alpha;  feature_log_prob_ = log(sf) - log(sf.sum(axis=1)[:, None])
      both:         class_log_prior_ = log(cc) - log(cc.sum())
      gaussian:     theta_ = (n1 + 2 n2) / cc;  var_ = (n0 theta^2 + n1 (1 - theta)^2 + n2 (2 - theta)^2) / cc + eps,
                    eps = var_smoothing * (largest whole-window variance over positions, from the pooled counts);
                    class_prior_ = cc / cc.sum()"""
    n1, n2, cc = np.asarray(n1, dtype=np.int64), np.asarray(n2, dtype=np.int64), np.asarray(cc, dtype=np.int64)
    present = np.flatnonzero(cc > 0)
    n1, n2, cc = n1[present], n2[present], cc[present].astype(np.float64)
    out = {"classes_": present.astype(np.int64)}
    if kind == "bernoulli":
        fc = (n1 + n2).astype(np.float64)
        out["feature_log_prob_"] = np.log(fc + alpha) - np.log((cc + alpha * 2).reshape(-1, 1))
        out["class_log_prior_"] = np.log(cc) - np.log(cc.sum())
    elif kind == "multinomial":
        sf = (n1 + 2 * n2).astype(np.float64) + alpha
        out["feature_log_prob_"] = np.log(sf) - np.log(sf.sum(axis=1).reshape(-1, 1))
        out["class_log_prior_"] = np.log(cc) - np.log(cc.sum())
    elif kind == "gaussian":
        n = cc.sum()
        s1, s2 = (n1 + 2 * n2).sum(axis=0).astype(np.float64), (n1 + 4 * n2).sum(axis=0).astype(np.float64)
        mu = s1 / n
        n0a, n1a, n2a = n - (n1 + n2).sum(axis=0), n1.sum(axis=0).astype(np.float64), n2.sum(axis=0).astype(np.float64)
        pooled = (n0a * mu ** 2 + n1a * (1.0 - mu) ** 2 + n2a * (2.0 - mu) ** 2) / n
        eps = var_smoothing * pooled.max()
        theta = (n1 + 2 * n2).astype(np.float64) / cc[:, None]
        n0 = cc[:, None] - (n1 + n2)
        var = (n0 * theta ** 2 + n1 * (1.0 - theta) ** 2 + n2 * (2.0 - theta) ** 2) / cc[:, None]
        out["theta_"], out["var_"], out["class_prior_"] = theta, var + eps, cc / n
    else:
        raise ValueError(f"kind must be one of {NB_TRAIN_KINDS}, got {kind!r}")
    return out


def train_nb_base(data: GnxModelData, X, y, kind, alpha=1e-10, var_smoothing=1e-9, ctx=None) -> dict:
    """fit a Naive-Bayes base of `data` in place (base_kind "nb", nb_kind, nb_table, nb_bias) -> info.  The device counts
    (gnx_train_nb_counts: exact integers), the closed forms finish in numpy (nb_fit_from_counts), the converter's nb_tables builds the
    tables.  alpha = 1e-10 is a decision: the reference asks for alpha=0, which the scikit-learn it pins (1.0.1) raises to 1e-10;
    newer scikit-learn keeps a true 0 and returns NaN on real genotype data.  A class with no rows in a window becomes an absent
    class of that window.  X must hold the codes 0..2, y labels in [0, A)."""
    from .convert import nb_tables
    if kind not in NB_TRAIN_KINDS:
        raise ValueError(f"kind must be one of {NB_TRAIN_KINDS}, got {kind!r}")
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != data.C or X.shape[0] < 1:
        raise ValueError(f"X must be (N >= 1, C={data.C}), got {X.shape}")
    if X.dtype.kind == "f" and np.any(X != np.rint(X)):
        raise ValueError("X must hold whole numbers (the SNP codes 0, 1, 2)")
    if X.min() < 0 or X.max() > 2:
        raise ValueError("X must hold the SNP codes 0, 1, 2 (2 = missing)")
    y = np.asarray(y)
    if y.shape != (X.shape[0], data.W):
        raise ValueError(f"y must be (N, W) = ({X.shape[0]}, {data.W}), got {y.shape}")
    if y.min() < 0 or y.max() >= data.A:
        raise ValueError(f"y must hold labels in 0..{data.A - 1}")
    n1, n2, cc = nb_counts(X, y, data.M, data.context, data.A, ctx=ctx)
    W, A = data.W, data.A
    table, bias = np.zeros((W, data.M_ + data.rem, 4, A)), np.zeros((W, A))
    fits = []
    for w in range(W):
        width = data.window_width(w)
        fit = nb_fit_from_counts(kind, n1[w, :, :width], n2[w, :, :width], cc[w], alpha=alpha, var_smoothing=var_smoothing)
        try:
            t, b = nb_tables(kind, fit, A)
        except ValueError as e:
            raise ValueError(f"window {w}: {e}") from e
        table[w, :width], bias[w] = t, b
        fits.append(fit)
    data.base_kind, data.nb_kind, data.nb_table, data.nb_bias = "nb", kind, table, bias
    return {"n_fit": int(X.shape[0]), "fits": fits, "n1": n1, "n2": n2, "class_count": cc}


# ---- the LDA base (LDABase) --------------------------------------------------------------------------------------------------------
def lda_gram(X, y, M, context, A, w0, w1, ctx=None, device=0):
    """the exact integers the LDA fit needs for the windows [w0, w1), on the device (gnx_train_lda_gram): X (N, C) int8 codes 0..2, y
    (N, W) labels in [0, A) -> G (w1 - w0, ldw, ldw) int32 (Xw^T Xw, full symmetric), S (w1 - w0, A, ldw) int32 (class sums) and
    n (w1 - w0, A) int32 (class counts); ldw = the widest window, positions past a window's width hold 0"""
    ctx = ctx or _lib.default_context(device)
    X = np.ascontiguousarray(X, dtype=np.int8)
    N, Cn = X.shape
    W = Cn // int(M)
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.shape != (N, W):
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
    ldw, nw = int(M) + 2 * int(context) + Cn - int(M) * W, int(w1) - int(w0)
    if not 0 <= int(w0) < int(w1) <= W:
        raise ValueError(f"the window range [{w0}, {w1}) is not inside [0, {W})")
    G, S, n = np.zeros((nw, ldw, ldw), np.int32), np.zeros((nw, int(A), ldw), np.int32), np.zeros((nw, int(A)), np.int32)
    ctx.check(ctx.lib.gnx_train_lda_gram(ctx.h, X.ctypes.data, N, Cn, y.ctypes.data, Cn, int(M), int(context), int(A), int(w0), int(w1),
                                         G.ctypes.data, S.ctypes.data, n.ctypes.data))
    return G, S, n


def lda_finish(G, S, n, N, tol=1e-4):
    """ONE window's LinearDiscriminantAnalysis(solver="svd", tol) fit from its integers -> (coef (A or 1, width), intercept (A or 1,),
    info).  G (width, width) = Xw^T Xw, S (A, width) class sums, n (A,) class counts, N rows; priors are the class frequencies.
    scikit-learn's _solve_svd, step by step, with the one SVD of the (N, width) scaled, class-centred data replaced by the
    eigen-decomposition of its Gram matrix, which the integers give exactly:
      scatter = G - sum_k S_k S_k^T / n_k;  std = sqrt(diag(scatter) / N), 1 where a column is constant within every class;
      fac / (std std^T) * scatter = V diag(s^2) V^T  (numpy.linalg.eigh), s descending;  rank = #(s > tol);
      scalings = (V[:, :rank] / std[:, None]) / s[:rank];
      the (A, rank) between-class matrix sqrt(N priors / (A - 1)) (means - xbar) @ scalings goes through a real SVD, rank2 =
      #(s2 > tol s2[0]); coef_ and intercept_ follow as in scikit-learn; for A == 2 row 1 minus row 0 is kept.
    A column is constant within every class exactly when its scatter is 0; a column that is not has scatter >= 1/2 (integer codes),
    and the float64 evaluation of the scatter is exact for the former, so the test is scatter < 1/4.
    info: rank, rank2, sv (all width values of s), sv2.  ValueError: a class without rows, N - A < 1."""
    G, S, n = np.asarray(G, dtype=np.float64), np.asarray(S, dtype=np.float64), np.asarray(n, dtype=np.float64)
    A, width = S.shape
    if np.any(n < 1):
        raise ValueError("class %d has no row" % int(np.flatnonzero(n < 1)[0]))
    if N - A < 1:
        raise ValueError(f"N - A = {N - A} < 1: the pooled covariance needs more rows than classes")
    priors = n / float(N)
    means = S / n[:, None]
    xbar = priors @ means
    scatter = G - (S / n[:, None]).T @ S
    diag = np.diagonal(scatter).copy()
    const = diag < 0.25
    std = np.sqrt(np.where(const, 0.0, diag) / float(N))
    std[const] = 1.0
    fac = 1.0 / (N - A)
    scaled = fac * (scatter / std[:, None] / std[None, :])
    scaled[const, :] = 0.0
    scaled[:, const] = 0.0
    lam, V = np.linalg.eigh(0.5 * (scaled + scaled.T))
    lam, V = lam[::-1], V[:, ::-1]
    sv = np.sqrt(np.maximum(lam, 0.0))
    rank = int(np.sum(sv > tol))
    scalings = (V[:, :rank] / std[:, None]) / sv[:rank]
    fac2 = 1.0 if A == 1 else 1.0 / (A - 1)
    Xb = (np.sqrt((N * priors) * fac2) * (means - xbar).T).T @ scalings
    _, sv2, Vt2 = np.linalg.svd(Xb, full_matrices=False)
    rank2 = int(np.sum(sv2 > tol * sv2[0])) if len(sv2) else 0
    scalings = scalings @ Vt2.T[:, :rank2]
    coef = (means - xbar) @ scalings
    intercept = -0.5 * np.sum(coef ** 2, axis=1) + np.log(priors)
    coef = coef @ scalings.T
    intercept -= xbar @ coef.T
    if A == 2:
        coef, intercept = coef[1:2] - coef[0:1], intercept[1:2] - intercept[0:1]
    return coef, intercept, {"rank": rank, "rank2": rank2, "sv": sv, "sv2": sv2}


# ---- the random-forest base (RFBase) ---------------------------------------------------------------------------------------------
RF_SEED_HIGH = 2 ** 31 - 1                      # sklearn.ensemble._base._set_random_states: randint(np.iinfo(np.int32).max)


def rforest_seeds_unchained(W):
    """forest seeds for RFBase's window fits: the reference fits them in spawned workers with unseeded generators, so there is no
    stream to reproduce; one seed per window from numpy's global generator, in window order, in one call -> int64 (W,)"""
    return np.random.randint(RF_SEED_HIGH, size=int(W)).astype(np.int64)


def rforest_bootstrap(seeds, n_trees, N):
    """what numpy's generator decides in RandomForestClassifier(n_estimators=n_trees, random_state=seed).fit on N rows, per window
    seed: the tree seeds RandomState(seed).randint(2**31 - 1) in order; per tree the bootstrap rows RandomState(ts).randint(0, N, N,
    dtype=int32) as row weights (bincount) and the splitter's state, the first randint(0, 2**31 - 1) of a FRESH RandomState(ts)
    -> (weight (W, n_trees, N) int64, state (W, n_trees) uint32)"""
    seeds = np.asarray(seeds).reshape(-1)
    W, T, N = len(seeds), int(n_trees), int(N)
    weight, state = np.zeros((W, T, N), np.int64), np.zeros((W, T), np.uint32)
    for w in range(W):
        rs = np.random.RandomState(int(seeds[w]))
        for t in range(T):
            ts = rs.randint(RF_SEED_HIGH)
            weight[w, t] = np.bincount(np.random.RandomState(ts).randint(0, N, N, dtype=np.int32), minlength=N)
            state[w, t] = np.random.RandomState(ts).randint(0, RF_SEED_HIGH)
    return weight, state


def train_rforest_arrays(X, y, M, context, A, seeds, n_trees=20, max_depth=4, ctx=None, device=0):
    """RFBase's per-window RandomForestClassifier(n_estimators=n_trees, max_depth=max_depth, random_state=seeds[w]).fit on the device,
    the same trees as scikit-learn 1.7.2 builds (gnx_train_rforest; the chain is stated in forest/k_train_rforest.hip).  X (N, C) int8
    codes {0, 1, 2} — a numpy array, or a CUDA int8 tensor that stays on the device — y (N, W) labels, seeds (W,) -> dict of rf_* arrays
    as GnxModelData takes them (convert.rforest_from_sklearn's layout).  The bootstrap is drawn here with numpy (rforest_bootstrap)."""
    ctx = ctx or _lib.default_context(device)
    on_dev = hasattr(X, "is_cuda") and X.is_cuda
    A, T, D = int(A), int(n_trees), int(max_depth)
    N, Cn = X.shape
    W = Cn // int(M)
    seeds = np.asarray(seeds).reshape(-1)
    if seeds.shape != (W,):
        raise ValueError(f"seeds must be (W,) = ({W},), got {seeds.shape}")
    if T < 1 or not 1 <= D <= 5:
        raise ValueError("n_trees >= 1 and 1 <= max_depth <= 5")
    weight, state = rforest_bootstrap(seeds, T, N)
    if weight.max() > 127:
        raise _lib.GnxError(_lib.GNX_EINVAL, "train_rforest: a bootstrap weight above 127")
    weight = weight.astype(np.uint8)
    keep = []
    if on_dev:
        import torch
        assert X.dtype == torch.int8 and X.dim() == 2 and X.stride(1) == 1
        ldx = X.stride(0) if N > 1 else Cn
        y = y if (hasattr(y, "is_cuda") and y.is_cuda) else torch.as_tensor(np.ascontiguousarray(y, dtype=np.int32), device=X.device)
        assert y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (N, W)
        dw, ds = torch.as_tensor(weight, device=X.device), torch.as_tensor(state.view(np.int32), device=X.device)
        keep = [dw, ds]
        x_ptr, y_ptr, w_ptr, s_ptr, fn = X.data_ptr(), y.data_ptr(), dw.data_ptr(), ds.data_ptr(), ctx.lib.gnx_train_rforest_dev
        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
        torch.cuda.current_stream(ctx.device).synchronize()
    else:
        X = np.ascontiguousarray(X, dtype=np.int8)
        ldx = Cn
        y = np.ascontiguousarray(y, dtype=np.int32)
        if y.shape != (N, W):
            raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
        x_ptr, y_ptr, w_ptr, s_ptr, fn = X.ctypes.data, y.ctypes.data, weight.ctypes.data, state.ctypes.data, ctx.lib.gnx_train_rforest
    cap = max(W * T, 1) * (2 ** (D + 1) - 1)
    wt0, tree_off = np.zeros(W + 1, np.int32), np.zeros(W * T + 1, np.int32)
    left, right, feat = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    thr, value = np.zeros(cap, np.float64), np.zeros((cap, A), np.float64)
    nn = C.c_int64(0)
    ctx.check(fn(ctx.h, x_ptr, int(N), int(ldx), y_ptr, int(Cn), int(M), int(context), A, T, D, w_ptr, s_ptr, wt0.ctypes.data,
                 tree_off.ctypes.data, left.ctypes.data, right.ctypes.data, feat.ctypes.data, thr.ctypes.data, value.ctypes.data,
                 C.addressof(nn)))
    del keep
    n = nn.value
    return dict(rf_win_tree0=wt0, rf_tree_off=tree_off, rf_left=left[:n].copy(), rf_right=right[:n].copy(), rf_feat=feat[:n].copy(),
                rf_thr=thr[:n].copy(), rf_value=value[:n].copy())


def rforest_placeholder(W, A):
    """one single-leaf tree per window: every class gets probability 1 / A"""
    return dict(rf_win_tree0=np.arange(W + 1, dtype=np.int32), rf_tree_off=np.arange(W + 1, dtype=np.int32),
                rf_left=np.full(W, -1, np.int32), rf_right=np.full(W, -1, np.int32), rf_feat=np.zeros(W, np.int32),
                rf_thr=np.full(W, -2.0, np.float64), rf_value=np.full((W, A), 1.0 / A, np.float64))


def train_rforest_base(data: GnxModelData, X, y, seeds=None, ctx=None) -> dict:
    """fit the random-forest base of `data` in place (base_kind "rforest", rf_* arrays) -> info.  Hyper-parameters are data.rf_train
    (n_trees, max_depth; RFBase's 20 and 4 when absent).  seeds (W,): one forest seed per window; by default drawn from numpy's global
    generator in window order (rforest_seeds_unchained).  ValueError (naming the window): a class of range(A) without rows in a window
    (scikit-learn would fit fewer classes and the reference's predict_proba_vectorized cannot stack such a model).  X must hold the
    codes 0..2, y labels in [0, A)."""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != data.C or X.shape[0] < 1:
        raise ValueError(f"X must be (N >= 1, C={data.C}), got {X.shape}")
    if X.dtype.kind == "f" and np.any(X != np.rint(X)):
        raise ValueError("X must hold whole numbers (the SNP codes 0, 1, 2)")
    if X.min() < 0 or X.max() > 2:
        raise ValueError("X must hold the SNP codes 0, 1, 2 (2 = missing)")
    y = np.asarray(y)
    N, W, A = X.shape[0], data.W, data.A
    if y.shape != (N, W):
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
    if y.min() < 0 or y.max() >= A:
        raise ValueError(f"y must hold labels in 0..{A - 1}")
    y32 = np.ascontiguousarray(y, dtype=np.int32)
    for w in range(W):
        cc = np.bincount(y32[:, w], minlength=A)
        if np.any(cc < 1):
            raise ValueError("window %d: class %d has no row" % (w, int(np.flatnonzero(cc < 1)[0])))
    hp = {"n_trees": 20, "max_depth": 4, **(getattr(data, "rf_train", None) or {})}
    if seeds is None:
        seeds = rforest_seeds_unchained(W)
    trees = train_rforest_arrays(np.ascontiguousarray(X, dtype=np.int8), y32, data.M, data.context, A, seeds, n_trees=hp["n_trees"],
                                 max_depth=hp["max_depth"], ctx=ctx)
    data.base_kind = "rforest"
    for k, v in trees.items():
        setattr(data, k, v)
    return {"n_fit": int(N), "seeds": np.asarray(seeds, dtype=np.int64), "n_nodes": int(len(trees["rf_left"])), **hp}


def host_threads():
    """the CPUs this process may use: OMP_NUM_THREADS when it is set (a job's allowance), else the scheduler's affinity mask"""
    import os
    try:
        v = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        v = 0
    return max(1, v if v > 0 else len(os.sched_getaffinity(0)))


def train_lda_base(data: GnxModelData, X, y, ctx=None, tol=1e-4, windows_per_call=None) -> dict:
    """fit the LDA base of `data` in place (base_kind "lda", lda_coef, lda_intercept) -> info.  The device computes every window's exact
    Gram matrix, class sums and counts (lda_gram, windows_per_call windows at a time: by default as many as keep G under 1 GiB); the
    host finishes each window in float64 (lda_finish), the windows of a call in parallel over the allowed host threads.
    ValueError (naming the window): a class of range(A) without rows in a window (the reference's predict_proba_vectorized cannot
    stack such a model either), N - A < 1.  X must hold the codes 0..2, y labels in [0, A)."""
    from concurrent.futures import ThreadPoolExecutor
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != data.C or X.shape[0] < 1:
        raise ValueError(f"X must be (N >= 1, C={data.C}), got {X.shape}")
    if X.dtype.kind == "f" and np.any(X != np.rint(X)):
        raise ValueError("X must hold whole numbers (the SNP codes 0, 1, 2)")
    if X.min() < 0 or X.max() > 2:
        raise ValueError("X must hold the SNP codes 0, 1, 2 (2 = missing)")
    y = np.asarray(y)
    N, W, A = X.shape[0], data.W, data.A
    if y.shape != (N, W):
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {y.shape}")
    if y.min() < 0 or y.max() >= A:
        raise ValueError(f"y must hold labels in 0..{A - 1}")
    if N - A < 1:
        raise ValueError(f"N - A = {N - A} < 1: the pooled covariance needs more rows than classes")
    ldw, R = data.M_ + data.rem, (1 if A == 2 else A)
    per_call = int(windows_per_call) if windows_per_call else max(1, min(W, (1 << 30) // (4 * ldw * ldw)))
    if per_call < 1:
        raise ValueError("windows_per_call must be at least 1")
    coef, icpt = np.zeros((W, R, ldw)), np.zeros((W, R))
    ranks = np.zeros((W, 2), np.int64)
    X8, y32 = np.ascontiguousarray(X, dtype=np.int8), np.ascontiguousarray(y, dtype=np.int32)
    workers = min(host_threads(), per_call)

    def one(w, G, S, n):
        width = data.window_width(w)
        try:
            c, b, info = lda_finish(G[:width, :width], S[:, :width], n, N, tol)
        except ValueError as e:
            raise ValueError(f"window {w}: {e}") from e
        coef[w, :, :width], icpt[w] = c, b
        ranks[w] = info["rank"], info["rank2"]

    with ThreadPoolExecutor(max_workers=workers) as pool:
        for w0 in range(0, W, per_call):
            w1 = min(W, w0 + per_call)
            G, S, n = lda_gram(X8, y32, data.M, data.context, A, w0, w1, ctx=ctx)
            for f in [pool.submit(one, w, G[w - w0], S[w - w0], n[w - w0]) for w in range(w0, w1)]:
                f.result()
    data.base_kind, data.lda_coef, data.lda_intercept = "lda", coef, icpt
    return {"n_fit": int(N), "ranks": ranks, "windows_per_call": per_call}


def untrained_model(C, M, A, S, context, mode, seed=None, meta=None, base=None):
    """an untrained model of a mode's kinds (the reference's config model.inference: "default", "fast", "large", "best"), ready to
    be loaded and then trained in place: zero logistic weights or, for "best", one placeholder SVC per window (A zero rows, zero
    coefficients), or with base="rf" (RFBase: the random forest) one single-leaf tree per window with value 1 / A and
    rf_train = dict(n_trees=20, max_depth=4) (the hyper-parameters HipBase.train fits with; kept in memory, not in the .gnx), or with base="xgb" one zero-valued stump per window and class, or with base="knn" one fit row of zeros with label 0
    per window, or with base="nb_bernoulli" / "nb_multinomial" / "nb_gaussian" zero Naive-Bayes tables and zero bias (every class
    gets 1 / A), or with base="string_kernel" / "poly_string_kernel" (StringKernelBase / PolynomialStringKernelBase) placeholder SVC
    windows tagged with the kernel and carrying its parameters, or with base="lda_svd" (LDABase: LinearDiscriminantAnalysis with its default svd solver; the bare name "lda" stays refused, as it
    was before the base existed) zero LDA coefficients and intercepts (every class gets 1 / A); the smoother's starting point:
    one placeholder tree, zero CRF weights, Conv1d's default initialisation.
    meta: optional dict with snp_pos, snp_ref, snp_alt, pop_order (the simulation's metadata)"""
    from . import synth
    from .convert import cov_sample
    if mode not in ("default", "fast", "large", "best"):
        raise ValueError("unknown model mode %r" % (mode,))
    W = C // M
    kw = {}
    if meta is not None:
        kw = dict(snp_pos=np.asarray(meta["snp_pos"]), snp_ref=np.asarray(meta["snp_ref"]), snp_alt=np.asarray(meta["snp_alt"]),
                  population_order=list(meta["pop_order"]))
    d = GnxModelData(C=C, M=M, A=A, S=S, context=context, **kw)
    nb_names = {"nb_" + k: k for k in NB_TRAIN_KINDS}
    if base not in (None, "svm", "xgb", "rf", "knn", "lda_svd", "string_kernel", "poly_string_kernel") and base not in nb_names:
        raise ValueError("base must be None (the mode's own base), \"svm\" (SVMBase: the RBF SVC), \"xgb\" (XGBBase: boosted trees), "
                         "\"rf\" (RFBase: the random forest), \"knn\" (KNNBase: 1-nearest neighbour), \"nb_bernoulli\" / \"nb_multinomial\" / \"nb_gaussian\" (the "
                         "Naive-Bayes bases), \"lda_svd\" (LDABase: linear discriminant analysis, svd solver), \"string_kernel\" (StringKernelBase: the plain "
                         "string-kernel SVC) or \"poly_string_kernel\" (PolynomialStringKernelBase: the polynomial string-kernel SVC), got %r" % (base,))
    if base == "lda_svd":   # LDABase (src/Base/models.py:83-94) in place of the mode's base; the smoother stays the mode's
        d.base_kind = "lda"
        d.lda_coef, d.lda_intercept = np.zeros((W, 1 if A == 2 else A, M + 2 * context + C - M * W)), np.zeros((W, 1 if A == 2 else A))
    elif base in nb_names:   # NB*Base (src/Base/models.py:96-132) in place of the mode's base; the smoother stays the mode's
        d.base_kind, d.nb_kind = "nb", nb_names[base]
        d.nb_table, d.nb_bias = np.zeros((W, M + 2 * context + C - M * W, 4, A)), np.zeros((W, A))
    elif base == "knn":   # KNNBase (src/Base/models.py:135-146) in place of the mode's base; the smoother stays the mode's
        d.base_kind, d.knn_X, d.knn_y = "knn", np.zeros((1, C), np.int8), np.zeros((1, W), np.int32)
    elif base == "rf":   # RFBase (src/Base/models.py:54-66) in place of the mode's base; the smoother stays the mode's
        d.base_kind, d.rf_train = "rforest", dict(n_trees=20, max_depth=4)
        for k, v in rforest_placeholder(W, A).items():
            setattr(d, k, v)
    elif base == "xgb":   # XGBBase (src/Base/models.py:24-35) in place of the mode's base; the smoother stays the mode's
        d.base_kind, d.fb_missing, d.fb_base_score = "forest", 2, 0.5
        for k, v in forest_placeholder(W, A).items():
            setattr(d, k, v)
    elif base == "svm":   # SVMBase (src/Base/models.py:148-159) in place of the mode's base; the smoother stays the mode's
        P = A * (A - 1) // 2
        d.base_kind, d.svc = "covrsk", []
        for w in range(W):
            d.svc.append(dict(xfit=np.zeros((A, d.window_width(w)), np.int8), support=np.arange(A, dtype=np.int32),
                              dual_coef=np.zeros((A - 1, A)), intercept=np.zeros(P), prob_a=np.zeros(P), prob_b=np.zeros(P),
                              n_support=np.ones(A, np.int32), kernel=np.array("rbf"), gamma=np.float64(0.001)))
    elif base in ("string_kernel", "poly_string_kernel"):
        # StringKernelBase / PolynomialStringKernelBase (src/Base/models.py:161-193) in place of the mode's base: placeholder windows
        # with the kernel's tag and parameters (every length / p = 1.2 and its run values); the smoother stays the mode's
        from .convert import poly_run_values, string_kernel_lengths
        P = A * (A - 1) // 2
        d.base_kind, d.svc = "covrsk", []
        for w in range(W):
            width = d.window_width(w)
            par = (dict(kernel=np.array("string_kernel"), ms=string_kernel_lengths(width, "string_kernel")) if base == "string_kernel" else
                   dict(kernel=np.array("poly_kernel"), **poly_run_values(width)))
            d.svc.append(dict(xfit=np.zeros((A, width), np.int8), support=np.arange(A, dtype=np.int32),
                              dual_coef=np.zeros((A - 1, A)), intercept=np.zeros(P), prob_a=np.zeros(P), prob_b=np.zeros(P),
                              n_support=np.ones(A, np.int32), **par))
    elif mode == "best":
        P = A * (A - 1) // 2
        d.base_kind, d.svc = "covrsk", []
        for w in range(W):
            width = d.window_width(w)
            d.svc.append(dict(xfit=np.zeros((A, width), np.int8), support=np.arange(A, dtype=np.int32),
                              dual_coef=np.zeros((A - 1, A)), intercept=np.zeros(P), prob_a=np.zeros(P), prob_b=np.zeros(P),
                              n_support=np.ones(A, np.int32), ms=cov_sample(width)))
    else:
        d.base_kind, d.lr_coef, d.lr_intercept = "logistic", np.zeros((W, A, M + 2 * context + C - M * W)), np.zeros((W, A))
    if mode == "fast":
        d.smooth_kind, d.crf_state, d.crf_trans = "crf", np.zeros((A, A)), np.zeros((A, A))
    elif mode == "large":
        d.smooth_kind = "cnn"
        d.cnn_weight, d.cnn_bias = cnn_init(A, S if S % 2 else S - 1, seed=seed)
    else:
        d.smooth_kind = "xgb"
        for k, v in synth.synthetic_trees(1, A, (S if S % 2 else S - 1) * A, seed=seed).items():
            setattr(d, k, v)
    return d
