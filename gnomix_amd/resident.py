"""Training from device-resident splits: what HipGnomix.train, HipBase and HipSmoother share when their inputs are CUDA tensors
(SplitPlan.materialise_dev's) instead of numpy arrays — recognising them, binding the library's stream to torch's for the duration,
and the confusion counts of a split that was predicted in HBM (gnx_confusion_dev, csrc/score/k_confusion.hip).

The host-array paths never import torch; nothing here does either until a tensor has been seen."""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager

import numpy as np

from . import _lib

PRED_LABELS_I32, PRED_PROBA_F64, PRED_PROBA_F32 = 0, 1, 2   # GNX_PRED_* of include/gnomix_hip.h
CONFUSION_MAX_A = 32                                        # GNX_CONFUSION_MAX_A


def is_cuda(a) -> bool:
    """a CUDA torch tensor (anything else, numpy arrays and CPU tensors included, is host data)"""
    return bool(getattr(a, "is_cuda", False))


def all_on_device(arrays, what="data") -> bool:
    """True when every array that is not None is a CUDA tensor, False when none is; a mixture is a TypeError"""
    flags = [is_cuda(a) for a in arrays if a is not None]
    if any(flags) and not all(flags):
        raise TypeError("%s mixes host arrays and CUDA tensors: pass every split (X and y) either as numpy arrays or as CUDA "
                        "tensors on the model's device" % what)
    return bool(flags) and all(flags)


def check_x(X, Cn, device):
    """X as the resident path takes it: (N, C) torch.int8 on the context's device, rows contiguous (any row stride)"""
    import torch
    if X.dtype != torch.int8 or X.dim() != 2 or X.shape[1] != Cn or (X.shape[0] > 0 and X.stride(1) != 1):
        raise TypeError(f"a device-resident X must be a torch.int8 (N, C={Cn}) tensor with contiguous rows, got {X.dtype} {tuple(X.shape)} "
                        f"strides {tuple(X.stride())}")
    if X.device.index != device:
        raise TypeError(f"X lives on {X.device}, the model on cuda:{device}")
    return X


def check_y(y, N, W, device):
    """y as the resident path takes it: torch.int32 on the context's device, (N, W) -> contiguous"""
    import torch
    if not is_cuda(y) or y.dtype != torch.int32 or y.device.index != device:
        raise TypeError(f"with a device-resident X, y must be a torch.int32 tensor on cuda:{device}")
    y = y.reshape(N, -1)
    if y.shape[1] != W:
        raise ValueError(f"y must be (N, W) = ({N}, {W}), got {tuple(y.shape)}")
    return y.contiguous()


def row_stride(X):
    """bytes between two rows of an int8 (N, C) tensor (a one-row tensor's stride is arbitrary)"""
    return int(X.stride(0)) if X.shape[0] > 1 else int(X.shape[1])


def adjacent_rows(parts):
    """One view over all the rows of `parts` when they are consecutive row ranges of one allocation, in this order and with one row
    stride (what SimPlan.as_splits cuts from the simulated matrix) — no bytes move; None otherwise (the caller concatenates)."""
    first = parts[0]
    if any(p.dim() != 2 or p.shape[0] < 1 or p.shape[1] != first.shape[1] or p.dtype != first.dtype or p.device != first.device
           or p.stride() != first.stride() or p.stride(1) != 1
           or p.untyped_storage().data_ptr() != first.untyped_storage().data_ptr() for p in parts):
        return None
    row_bytes = first.stride(0) * first.element_size()
    if first.stride(0) < first.shape[1]:
        return None
    end = first.data_ptr()
    for p in parts:
        if p.data_ptr() != end:
            return None
        end += p.shape[0] * row_bytes
    return first.as_strided((sum(p.shape[0] for p in parts), first.shape[1]), first.stride())


@contextmanager
def torch_stream(ctx):
    """the library context works on torch's current stream inside the block and on the stream it had before after it"""
    import torch
    prev = ctx.bound_stream
    ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    try:
        yield
    finally:
        if prev is _lib.OWN_STREAM:
            ctx.reset_stream()
        else:
            ctx.set_stream(prev)


def to_host(a):
    """a CUDA tensor as a numpy array (None stays None)"""
    return None if a is None else a.cpu().numpy()


def confusion_counts(ctx, y, pred, A, debug_flush_every=0, want_flushes=False):
    """(A, A) int64 counts  cm[t, p] = #{y == t and prediction == p}  of device-resident labels against device-resident predictions
    (gnx_confusion_dev): `pred` is an int32 label tensor of y's size, or float64 / float32 probabilities (..., A) whose first-maximum
    argmax the kernel takes itself (np.argmax(B, -1) of Base.evaluate).  A label outside [0, A) raises GnxError(GNX_EINVAL).
    want_flushes: -> (counts, how often a workgroup added its table to the counts)"""
    import torch
    y = y.reshape(-1)
    n = y.numel()
    if not is_cuda(y) or y.dtype != torch.int32 or not is_cuda(pred):
        raise TypeError("confusion_counts: y must be a torch.int32 CUDA tensor and pred a CUDA tensor")
    y = y.contiguous()
    if pred.dtype == torch.int32:
        kind, ok = PRED_LABELS_I32, pred.numel() == n
    elif pred.dtype in (torch.float64, torch.float32):
        kind, ok = (PRED_PROBA_F64 if pred.dtype == torch.float64 else PRED_PROBA_F32), pred.numel() == n * int(A)
    else:
        raise TypeError(f"confusion_counts: pred must be int32 labels or float32 / float64 probabilities, got {pred.dtype}")
    if not ok:
        raise ValueError(f"confusion_counts: pred {tuple(pred.shape)} does not match {n} labels and A = {A}")
    pred = pred.contiguous()
    cm = torch.zeros((max(int(A), 1) ** 2,), dtype=torch.int64, device=y.device)
    nfl = C.c_int64(0)
    with torch_stream(ctx):
        ctx.check(ctx.lib.gnx_confusion_dev(ctx.h, y.data_ptr(), pred.data_ptr(), kind, n, int(A), cm.data_ptr(), int(debug_flush_every),
                                            C.byref(nfl)))
        counts = cm.cpu().numpy().reshape(int(A), int(A))
    return (counts, int(nfl.value)) if want_flushes else counts


def confusion_counts_host(ctx, y, pred, A, debug_flush_every=0):
    """the same for numpy arrays (gnx_confusion stages them): y int32, pred int32 labels or float32 / float64 probabilities"""
    y = np.ascontiguousarray(y, dtype=np.int32).reshape(-1)
    pred = np.ascontiguousarray(pred)
    if pred.dtype not in (np.float32, np.float64):
        pred = np.ascontiguousarray(pred, dtype=np.int32)
    kind = {np.dtype(np.int32): PRED_LABELS_I32, np.dtype(np.float64): PRED_PROBA_F64, np.dtype(np.float32): PRED_PROBA_F32}[pred.dtype]
    if pred.size != y.size * (1 if kind == PRED_LABELS_I32 else int(A)):
        raise ValueError(f"confusion_counts_host: pred {pred.shape} does not match {y.size} labels and A = {A}")
    cm = np.zeros((max(int(A), 1), max(int(A), 1)), np.int64)
    ctx.check(ctx.lib.gnx_confusion(ctx.h, y.ctypes.data, pred.ctypes.data, kind, y.size, int(A), cm.ctypes.data, int(debug_flush_every),
                                    None))
    return cm
