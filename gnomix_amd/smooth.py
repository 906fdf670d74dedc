"""HipSmoother — the reference's Smoother plugin interface (src/Smooth/smooth.py:7-65) served by the
HIP kernels.  `.model.predict_proba(rows)` is kept because Gnofix calls it (gnofix.py:157)."""
from __future__ import annotations

from time import time

import numpy as np


class _RowModel:
    """stands where XGBClassifier stands: predict_proba on explicit (R, S*A) rows"""

    def __init__(self, dev):
        self.dev = dev

    def predict_proba(self, rows):
        rows = np.asarray(rows)
        return self.dev.smooth_rows(rows.reshape(rows.shape[0], -1))


class HipSmoother:

    def __init__(self, device_model, calibrate=None, mode_filter=0, n_jobs=None, seed=None, verbose=False):
        d = device_model.data
        self._calibrate = None
        self.dev = device_model
        self.W = d.C // d.M
        self.A = d.A
        self.S = d.S if d.S % 2 else d.S - 1   # smooth.py:14
        self._calibrate = None
        self.calibrator = d.calib_off is not None or None   # truthy when the model carries fitted isotonic maps
        self.calibrate = calibrate
        self.mode_filter = mode_filter
        self.n_jobs = n_jobs
        self.seed = seed
        self.verbose = verbose
        self.gnofix = d.smooth_kind == "xgb"   # only XGB_Smoother sets it (Smooth/models.py:12)
        self.model = _RowModel(device_model) if d.smooth_kind == "xgb" else None
        self.time = {}

    @property
    def dev(self):
        return self._dev

    @dev.setter
    def dev(self, m):
        """every (re)binding of the device model — training builds fresh ones — carries the calibrate switch over: a new
        gnx_model starts with calibration off (the reference keeps calibrating after Gnomix.train's base retrain, model.py:119-167)"""
        self._dev = m
        m.set_calibrate(bool(self._calibrate))

    @property
    def calibrate(self):
        return self._calibrate

    @calibrate.setter
    def calibrate(self, on):  # gnomix.py:367 pokes this attribute after loading the model
        self._calibrate = on
        self.dev.set_calibrate(bool(on))

    def train(self, B, y, **kw):
        """Smoother.train (smooth.py:28-38) for the tree smoother: gradient boosting on the device with the reference's
        XGBClassifier arguments (Smooth/models.py:14-20), then the device model is swapped for the freshly trained one.
        B (N, W, A) base probabilities of the smoother's training haplotypes, y (N, W) labels."""
        from .train import train_gbt_smoother, train_cnn_smoother, train_crf_smoother
        from .model import DeviceModel
        from . import resident
        if resident.all_on_device([B, y], "HipSmoother.train: (B, y)"):
            if self.dev.data.smooth_kind in ("cnn", "crf"):
                # CUDA tensors: the tree smoother fits them in place (gnx_train_gbt_dev); the CNN and CRF trainers take host arrays
                import warnings
                warnings.warn("HipSmoother.train: the %s smoother has no device-resident training path; B and y are copied to the host "
                              "once and the host-array path runs" % self.dev.data.smooth_kind, RuntimeWarning, stacklevel=2)
                B, y = resident.to_host(B), resident.to_host(y)
            else:
                return self._train_resident(B, y, **kw)
        y = np.asarray(y)
        assert len(np.unique(y)) == self.A, "Smoother training data does not include all populations"   # smooth.py:30
        if self.dev.data.smooth_kind == "cnn":   # CNN_Smoother: CNN.fit (Smooth/cnn.py:104-118) on the device
            t = time()
            self.train_loss = train_cnn_smoother(self.dev.data, B, y.reshape(np.asarray(B).shape[0], -1), ctx=self.dev.ctx, **kw)
            self.dev = DeviceModel(self.dev.data, ctx=self.dev.ctx)
            self.time["train"] = time() - t
            return self
        if self.dev.data.smooth_kind == "crf":   # CRF_Smoother: CRFsuite's objective, L-BFGS with device evaluations
            t = time()
            self.train_info = train_crf_smoother(self.dev.data, B, y.reshape(np.asarray(B).shape[0], -1), ctx=self.dev.ctx, **kw)
            if not self.train_info.get("converged", True):   # as the logistic base does: a fit that stopped early must not pass silently
                import warnings
                warnings.warn("gnx_train_crf stopped after %s iterations without reaching its gradient tolerance: the CRF smoother is not "
                              "converged" % self.train_info.get("iterations", "?"), RuntimeWarning, stacklevel=2)
            self.dev = DeviceModel(self.dev.data, ctx=self.dev.ctx)
            self.time["train"] = time() - t
            return self
        t = time()
        self.train_loss = train_gbt_smoother(self.dev.data, B, y.reshape(B.shape[0], -1), ctx=self.dev.ctx, **kw)
        self.dev = DeviceModel(self.dev.data, ctx=self.dev.ctx)   # (a HipGnomix re-binds base and fused path: HipGnomix.train_smoother)
        self.gnofix = True
        self.model = _RowModel(self.dev)
        self.time["train"] = time() - t
        return self

    def _train_resident(self, B, y, **kw):
        """train() of the tree smoother on CUDA tensors: B (N, W, A) float32 / float64, y (N, W) int32, both read in place"""
        import torch
        from .train import train_gbt_smoother
        from .model import DeviceModel
        ctx = self.dev.ctx
        N = B.shape[0]
        from .resident import check_y
        y = check_y(y, N, self.W, ctx.device)
        assert len(torch.unique(y)) == self.A, "Smoother training data does not include all populations"   # smooth.py:30
        t = time()
        from .resident import torch_stream
        with torch_stream(ctx):
            self.train_loss = train_gbt_smoother(self.dev.data, B.contiguous(), y, ctx=ctx, **kw)
            self.dev = DeviceModel(self.dev.data, ctx=ctx)
        self.gnofix = True
        self.model = _RowModel(self.dev)
        self.time["train"] = time() - t
        return self

    def train_calibrator(self, B, y, frac=0.05):
        """Smoother.train_calibrator (smooth.py:81-92): uncalibrated probabilities of a random `frac` of the haplotypes (numpy's
        global generator, as the reference), one isotonic map per class (gnomix_amd.calibrate), device model re-loaded with them.
        The fit follows the dtype the smoother returns: float32 for the tree and the CNN smoother, float64 for the CRF smoother."""
        from .calibrate import fit_calibrator
        from .model import DeviceModel
        from . import resident
        on_dev = resident.all_on_device([B, y], "HipSmoother.train_calibrator: (B, y)")
        if not on_dev:
            B = np.asarray(B)
            y = np.asarray(y)
        calibrate = self.calibrate
        self.calibrate = False
        idxs = np.random.choice(len(B), int(frac * len(B)), replace=False)
        if on_dev:
            # the same draw; the rows are gathered and smoothed in HBM, only the drawn rows' probabilities and labels come to the host
            import torch
            with resident.torch_stream(self.dev.ctx):
                rows = torch.from_numpy(idxs.astype(np.int64)).to(B.device)
                proba = self.predict_proba(B.index_select(0, rows)).reshape(-1, self.A).cpu().numpy()
                y_sel = y.reshape(len(B), -1).index_select(0, rows).reshape(-1).cpu().numpy()
        else:
            proba = self.predict_proba(B[idxs]).reshape(-1, self.A)
            y_sel = y[idxs].reshape(-1)
        for k, v in fit_calibrator(proba, y_sel, self.A).items():
            setattr(self.dev.data, k, v)
        self.dev = DeviceModel(self.dev.data, ctx=self.dev.ctx)   # (a HipGnomix re-binds: HipGnomix.train)
        if self.model is not None:
            self.model.dev = self.dev
        self.calibrator = True
        self.calibrate = calibrate
        return self

    def evaluate(self, B=None, y=None, y_pred=None):
        """(accuracy %, balanced accuracy %) rounded to two decimals (smooth.py:67-79)"""
        from .metrics import accuracy_pair, accuracy_pair_from_counts
        from . import resident
        if B is not None:
            y_pred = self.predict(B)
        elif y_pred is None:
            raise ValueError("Need either Base probabilities or y predictions.")
        if resident.all_on_device([y, y_pred], "HipSmoother.evaluate: (y, y_pred)"):
            import torch
            return accuracy_pair_from_counts(resident.confusion_counts(self.dev.ctx, y, y_pred.to(torch.int32), self.A))
        return accuracy_pair(y, y_pred)

    def predict_proba(self, B):
        """B (N, W, A) -> (N, W, A): float32 for the xgb smoother, float64 for crf (smooth.py:40-56)."""
        from . import resident
        t = time()
        if self.calibrate:
            if self.calibrator is None:
                print("No calibrator found, returning original probabilities.")  # smooth.py:49-50
        if resident.is_cuda(B):   # CUDA in, CUDA out, the dtype the numpy form returns
            import torch
            pd = torch.float64 if self.dev.proba_dtype() == np.float64 else torch.float32
            with resident.torch_stream(self.dev.ctx):
                proba, _ = self.dev.smooth_predict_device(self._b_dev(B), want_proba=True, want_labels=False, proba_dtype=pd)
        else:
            proba, _ = self.dev.smooth_predict(B, want_proba=True, want_labels=False)
        self.time["inference"] = time() - t
        return proba.reshape(-1, self.W, self.A)

    def _b_dev(self, B):
        """B as the device entry takes it: (N, W, A) float32 / float64, contiguous"""
        import torch
        if B.dim() != 3 or tuple(B.shape[1:]) != (self.W, self.A):
            raise ValueError(f"B must be (N, W={self.W}, A={self.A}), got {tuple(B.shape)}")
        if B.dtype not in (torch.float32, torch.float64):
            B = B.to(torch.float64)
        return B.contiguous()

    def predict(self, B):
        """argmax labels (N, W) int64, first max wins; with mode_filter = k, each label but the first and last k // 2 of a row
        becomes the unambiguous mode of the k labels around it (smooth.py:58-65, Smooth/utils.py:31-46; k_mode_filter)."""
        from . import resident
        if resident.is_cuda(B):   # CUDA in, CUDA out (int64, as the numpy form)
            import torch
            with resident.torch_stream(self.dev.ctx):
                _, lab = self.dev.smooth_predict_device(self._b_dev(B), want_proba=False, want_labels=True)
                if self.mode_filter:
                    lab = self.dev.mode_filter_device(lab, self.mode_filter)
                return lab.to(torch.int64)
        _, lab = self.dev.smooth_predict(B, want_proba=False, want_labels=True)
        if self.mode_filter:
            lab = self.dev.mode_filter(lab, self.mode_filter)
        return lab.astype(np.int64)
