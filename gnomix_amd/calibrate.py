"""Fitting the calibrator: `Calibrator.fit` (reference src/Smooth/Calibration.py:43-55) = one
sklearn IsotonicRegression(out_of_bounds="clip") per class on (proba[:, i], y == class i), called from
`Smoother.train_calibrator` (src/Smooth/smooth.py:81-92) on the smoother's probabilities of a 5 % sample of the haplotypes.
The isotonic fit itself is gnx_fit_isotonic_f32 / gnx_fit_isotonic_f64 (host arithmetic in the library: sort, merge, pool adjacent
violators), chosen by the dtype of the probabilities as scikit-learn chooses its arithmetic: the tree and the CNN smoother return
float32 (src/Smooth/cnn.py:148-151), the CRF smoother float64."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def fit_isotonic(x, y):
    """x, y (n,) -> (X_thresholds_, y_thresholds_), as IsotonicRegression(out_of_bounds="clip").fit(x, y): float64 x is fitted in
    float64 (y is cast to x's type, as scikit-learn does), anything else in float32"""
    f64 = np.asarray(x).dtype == np.float64
    dt = np.float64 if f64 else np.float32
    x = np.ascontiguousarray(x, dtype=dt).reshape(-1)
    y = np.ascontiguousarray(y, dtype=dt).reshape(-1)
    if x.shape != y.shape or x.size == 0:
        raise ValueError("fit_isotonic: x and y must be non-empty and of one length")
    xt, yt = np.empty_like(x), np.empty_like(x)
    n = C.c_int64(0)
    name = "gnx_fit_isotonic_f64" if f64 else "gnx_fit_isotonic_f32"
    rc = getattr(_lib.load(), name)(x.ctypes.data, y.ctypes.data, x.size, xt.ctypes.data, yt.ctypes.data, C.addressof(n))
    if rc != 0:
        raise _lib.GnxError(rc, name + " failed")
    return xt[:n.value].copy(), yt[:n.value].copy()


def fit_calibrator(proba, y, n_classes):
    """proba (R, A) smoother probabilities in the dtype the smoother returns them (float64: the CRF smoother, fitted in float64 with
    calib_is_f32 False; anything else is cast to float32 like the tree and CNN smoothers'), y (R,) labels -> the calib_* fields of
    GnxModelData.  Column i is fitted against the i-th class of sorted(unique(y)) (OneHotEncoder's order, Calibration.py:51-52);
    every class must occur."""
    f64 = np.asarray(proba).dtype == np.float64
    dt = np.float64 if f64 else np.float32
    proba = np.asarray(proba, dtype=dt).reshape(-1, n_classes)
    y = np.asarray(y).reshape(-1)
    classes = np.unique(y)
    if len(classes) != n_classes:
        raise ValueError("calibrator training data does not include all populations")
    off, xs, ys = [0], [], []
    for i in range(n_classes):
        xt, yt = fit_isotonic(np.ascontiguousarray(proba[:, i]), (y == classes[i]).astype(dt))
        xs.append(xt.astype(np.float64)); ys.append(yt.astype(np.float64))
        off.append(off[-1] + len(xt))
    return dict(calib_off=np.array(off, np.int32), calib_x=np.concatenate(xs), calib_y=np.concatenate(ys), calib_is_f32=not f64)
