"""HipBase — the reference's Base plugin interface (src/Base/base.py:8-27, 129-180, 214-216) served
by the HIP kernels.  Same attribute names (C, M, W, A, context, n_jobs, vectorize, time) and the
same method contracts, so run_inference()/Gnomix.predict read unchanged (gnomix.py:55)."""
from __future__ import annotations

from time import time

import numpy as np


class HipBase:

    def __init__(self, device_model, n_jobs=None, verbose=False):
        d = device_model.data
        self.dev = device_model
        self.C = d.C
        self.M = d.M
        self.W = d.C // d.M
        self.A = d.A
        self.context = d.context
        self.missing_encoding = 2
        self.n_jobs = n_jobs
        self.verbose = verbose
        self.vectorize = True          # poked by gnomix.py:370; the device path is always "vectorized"
        self.base_multithread = False
        self.log_inference = False
        self.time = {}

    def train(self, X, y, verbose=False):
        """Base.train (base.py:104-127) on the device, X (N, C) int8, y (N, W) window labels; swaps the device model for the freshly
        trained one.  Logistic base: every window's LogisticRegression.  CovRSK base: every window's SVC(kernel=CovRSK,
        probability=True), seeded as the reference's sequential fits are (window 0 from numpy's global generator, like
        BaseLibSVM.fit; later windows from the state each CovRSK kernel call leaves), and the global generator is left where the
        reference leaves it.  RBF windows (SVMBase): every window's SVC(C=100, gamma, probability=True), one seed per window drawn
        from numpy's global generator in window order.  Windows tagged "string_kernel" / "poly_kernel" (StringKernelBase /
        PolynomialStringKernelBase): every window's SVC(kernel=<that kernel>, probability=True) with the window's own lengths / exponent,
        seeded likewise (the reference fits them sequentially and their kernels draw nothing), the generator left there; untagged
        string-kernel windows are fitted as CovRSK.  Forest base (XGBBase): every window's 20 rounds of depth-4 boosted
        trees (train.train_forest_base).  1-NN base (KNNBase): the rows are stored (train.train_knn_base; there is nothing to fit).
        Naive-Bayes bases (NB*Base): counts on the device, closed forms on the host (train.train_nb_base; alpha = 1e-10).
        LDA base (LDABase): the exact Gram matrix, class sums and counts on the device, scikit-learn's svd solver restated on them in
        float64 on the host (train.train_lda_base).  Random-forest base (RFBase) of a model made by untrained_model(base="rf"): every window's
        20 depth-4 trees as scikit-learn builds them (train.train_rforest_base); an rforest model without rf_train (a converted pickle,
        a loaded .gnx) has no hyper-parameters and is refused."""
        from .train import train_logistic_base, train_svc_base, svc_seed_chain, svc_rng_after_kernel, svc_window_kernel, SVC_SEED_HIGH
        from .model import DeviceModel, svc_window_is_rbf
        from . import resident
        d = self.dev.data
        if resident.all_on_device([X, y], "HipBase.train: (X, y)") and d.base_kind not in (None, "logistic"):
            # CUDA tensors: the logistic base fits them in place (gnx_train_logistic_dev); every other base takes the host path
            import warnings
            warnings.warn("HipBase.train: the %s base has no device-resident training path; X and y are copied to the host once and "
                          "the host-array path runs" % d.base_kind, RuntimeWarning, stacklevel=2)
            X, y = resident.to_host(X), resident.to_host(y)
        if d.base_kind == "rforest" and not getattr(d, "rf_train", None):
            # a converted pickle, a synthetic model or a loaded .gnx carries no hyper-parameters to fit with
            raise NotImplementedError("on-device training is not built for the random-forest base (RFBase: scikit-learn's bootstrap "
                                      "stream); the logistic, SVC (CovRSK, RBF), boosted-tree (XGBBase), 1-NN (KNNBase), Naive-Bayes and LDA bases are")
        if d.base_kind not in (None, "logistic", "covrsk", "forest", "rforest", "knn", "nb", "lda"):
            raise NotImplementedError("on-device training is built for the logistic, the SVC (CovRSK, RBF), the boosted-tree, the 1-NN, the "
                                      "Naive-Bayes and the LDA bases")
        t = time()
        if d.base_kind == "rforest":
            # RFBase: every window's RandomForestClassifier(n_estimators=20, max_depth=4), scikit-learn's own trees; one forest seed per
            # window from numpy's global generator, in window order (the reference's workers fit with unseeded generators)
            from .train import train_rforest_base
            self.train_info = train_rforest_base(d, X, y, ctx=self.dev.ctx)
        elif d.base_kind == "lda":
            from .train import train_lda_base
            self.train_info = train_lda_base(d, X, y, ctx=self.dev.ctx)
        elif d.base_kind == "nb":
            # NB*Base: integer counts on the device, scikit-learn's closed forms on the host (train.train_nb_base)
            from .train import train_nb_base
            self.train_info = train_nb_base(d, X, y, d.nb_kind, ctx=self.dev.ctx)
        elif d.base_kind == "knn":
            from .train import train_knn_base
            self.train_info = train_knn_base(d, X, y, ctx=self.dev.ctx)
        elif d.base_kind == "forest":
            # XGBBase: every window's XGBClassifier(n_estimators=20, max_depth=4) (the algorithm, not xgboost's own trajectory)
            from .train import train_forest_base
            self.train_info = {"loss": train_forest_base(d, X, y, ctx=self.dev.ctx)}
        elif d.base_kind == "covrsk" and d.svc and svc_window_is_rbf(d.svc[0]):
            # SVMBase: the reference's workers fit with unseeded generators; one seed per window from the global generator, in order
            self.train_info = train_svc_base(d, X, y, ctx=self.dev.ctx, kernel="rbf", gamma=float(d.svc[0]["gamma"]))
        elif d.base_kind == "covrsk" and d.svc and svc_window_kernel(d.svc[0]) in ("string_kernel", "poly_kernel"):
            # StringKernelBase / PolynomialStringKernelBase (windows tagged by train_svc_base / untrained_model): sequential fits whose
            # kernels leave numpy's global generator alone, so window w's seed is the w-th value drawn from it; no CovRSK seed chain
            kernel = svc_window_kernel(d.svc[0])
            kw = dict(p=float(d.svc[0]["poly_p"])) if kernel == "poly_kernel" else {}
            self.train_info = train_svc_base(d, X, y, ctx=self.dev.ctx, kernel=kernel, **kw)
        elif d.base_kind == "covrsk":
            widths = [d.window_width(w) for w in range(d.W)]
            seeds = svc_seed_chain(widths, np.random.randint(SVC_SEED_HIGH))
            self.train_info = train_svc_base(d, X, y, ctx=self.dev.ctx, seeds=seeds)
            svc_rng_after_kernel(widths[-1])
        else:
            self.train_info = train_logistic_base(d, X, y, ctx=self.dev.ctx)
        self.dev = DeviceModel(d, ctx=self.dev.ctx)   # (a HipGnomix re-binds its smoother: HipGnomix.train_base)
        self.time["train"] = time() - t
        return self

    def evaluate(self, X=None, y=None, B=None):
        """(accuracy %, balanced accuracy %) rounded to two decimals, from SNPs or from base probabilities (base.py:214-228)"""
        from .metrics import accuracy_pair, accuracy_pair_from_counts
        from . import resident
        if resident.all_on_device([X, y, B], "HipBase.evaluate: (X, y, B)"):
            # device-resident: the kernel takes the argmax of the probabilities itself and only the A x A counts come back
            if X is None and B is None:
                raise ValueError("Need either SNP input or estimated probabilities to evaluate.")
            B = self.predict_proba(X) if X is not None else B
            return accuracy_pair_from_counts(resident.confusion_counts(self.dev.ctx, y, B, self.A))
        if X is not None:
            y_pred = self.predict(X)
        elif B is not None:
            y_pred = np.argmax(B, axis=-1)
        else:
            raise ValueError("Need either SNP input or estimated probabilities to evaluate.")
        return accuracy_pair(y, y_pred)

    def predict_proba(self, X):
        """X (N, C) int8-like -> B (N, W, A) float64, as Base.predict_proba (base.py:129-180).  A CUDA int8 tensor (rows contiguous,
        any row stride) gives a CUDA float64 tensor and nothing crosses the host link."""
        from . import resident
        t = time()
        if resident.is_cuda(X):
            with resident.torch_stream(self.dev.ctx):
                B = self.dev.base_predict_device(resident.check_x(X, self.C, self.dev.ctx.device), f64=True)
        else:
            _, B = self.dev.base_predict(X, want_f32=False, want_f64=True)
        self.time["inference"] = time() - t
        return B

    def predict_proba_f32(self, X):
        """float32(B): what the XGB smoother actually consumes (Smooth/utils.py:20)."""
        b32, _ = self.dev.base_predict(X, want_f32=True, want_f64=False)
        return b32

    def predict(self, X):
        B = self.predict_proba(X)
        return B.argmax(dim=-1) if hasattr(B, "is_cuda") else np.argmax(B, axis=-1)  # base.py:214-216 (both: first maximum)
