"""HipGnomix — the inference surface of the reference's model object (src/model.py:12-214):
predict / predict_proba / phase and the attributes run_inference() and the writers read
(C, M, A, S, W, context, snp_pos, snp_ref, snp_alt, population_order, gen_map_df, base, smooth)."""
from __future__ import annotations

import sys
from contextlib import contextmanager

import numpy as np

from . import resident
from .base import HipBase
from .model import DeviceModel, GnxModelData
from .smooth import HipSmoother


class HipGnomix:

    def __init__(self, data: GnxModelData, device: int = 0, ctx=None, calibrate=False, verbose=False, prepared=None, mode_filter=None):
        """mode_filter: Gnomix(..., mode_filter=k) (src/model.py:18, 80); None takes the model's own (GnxModelData.mode_filter, what a
        converted model.pkl or a .gnx carries), 0 / False switches it off"""
        self.data = data
        self.dev = DeviceModel(data, ctx=ctx, device=device, prepared=prepared)
        self.C, self.M, self.A, self.S = data.C, data.M, data.A, data.S
        self.W = self.C // self.M
        self.context = data.context
        self.snp_pos, self.snp_ref, self.snp_alt = data.snp_pos, data.snp_ref, data.snp_alt
        self.population_order = data.population_order
        self.calibrate = calibrate
        self.n_cores = None
        self.verbose = verbose
        self.gen_map_df = {}
        if data.gen_map_pos is not None:
            try:
                import pandas as pd
                self.gen_map_df = pd.DataFrame({"pos": data.gen_map_pos, "pos_cm": data.gen_map_cm})
            except ImportError:
                self.gen_map_df = {"pos": data.gen_map_pos, "pos_cm": data.gen_map_cm}
        self.base = HipBase(self.dev, verbose=verbose)
        self.smooth = HipSmoother(self.dev, calibrate=calibrate, mode_filter=(data.mode_filter if mode_filter is None else mode_filter) or 0,
                                  verbose=verbose)
        self.time = {}

    @classmethod
    def load(cls, path, **kw):
        return cls(GnxModelData.load(path), **kw)

    def save(self, path):
        """write the model (base, smoother, calibrator, metadata) as a .gnx archive: what Gnomix.save pickles (src/model.py:100-102)"""
        self.dev.data.save(path)
        return path

    def train_base(self, X, y):
        """the base half of Gnomix.train (src/model.py:113, 155): fit the base (logistic, SVC or boosted trees) on the device, then re-bind base,
        smoother and the fused path to the freshly loaded model"""
        self.base.train(X, y)
        self.dev = self.base.dev
        self.smooth.dev = self.dev
        if self.smooth.model is not None:
            self.smooth.model.dev = self.dev
        return self

    def train_smoother(self, B, y, **kw):
        """the smoother half of Gnomix.train (src/model.py:116-117): fit the tree smoother on the device, re-bind everything"""
        self.smooth.train(B, y, **kw)
        self.dev = self.smooth.dev
        self.base.dev = self.dev
        return self

    def conf_matrix(self, y, y_pred):
        from .metrics import confusion
        return confusion(y, y_pred)

    def _score_splits(self, splits):
        """The bookkeeping half of Gnomix.train (src/model.py:127-151), one split at a time.  The reference scores the base on a
        split's own haplotypes and the smoother on labels predicted from base probabilities: for "train" those are two different
        sets (base: train1; smoother: train2, whose probabilities `train` already holds), for "val" one.  Keys as the reference
        stores them: <base|smooth>_<split>_acc[_bal] in `accuracies`, the split's name in `Confusion_Matrices`."""
        from .metrics import accuracy_pair_from_counts, confusion_from_counts
        acc, cms = {}, {}
        for name, parts in splits.items():
            if parts is None:
                continue
            (X, y), smoother_part = parts
            B = self.base.predict_proba(X)
            labels = self.smooth.predict(B)
            B_s, y_s = smoother_part if smoother_part is not None else (B, y)
            labels_s = labels if smoother_part is None else self.smooth.predict(B_s)
            if resident.is_cuda(X):
                # the split was predicted in HBM: three passes of gnx_confusion_dev, 3 A^2 integers to the host, the same formulas
                import torch
                ctx = self.dev.ctx
                counts = resident.confusion_counts(ctx, y, labels.to(torch.int32), self.A)
                acc["base_%s_acc" % name], acc["base_%s_acc_bal" % name] = accuracy_pair_from_counts(resident.confusion_counts(ctx, y, B, self.A))
                acc["smooth_%s_acc" % name], acc["smooth_%s_acc_bal" % name] = accuracy_pair_from_counts(
                    counts if smoother_part is None else resident.confusion_counts(ctx, y_s, labels_s.to(torch.int32), self.A))
                cms[name] = confusion_from_counts(counts)
                continue
            acc["base_%s_acc" % name], acc["base_%s_acc_bal" % name] = self.base.evaluate(X=None, y=y, B=B)
            acc["smooth_%s_acc" % name], acc["smooth_%s_acc_bal" % name] = self.smooth.evaluate(B=None, y=y_s, y_pred=labels_s)
            cms[name] = self.conf_matrix(y=y, y_pred=labels)
        return acc, cms

    def _resident_mode(self):
        """the reference's mode name of this model's base / smoother pair, for messages"""
        d = self.dev.data
        return {("logistic", "xgb"): "default", ("logistic", "crf"): "fast", ("logistic", "cnn"): "large",
                ("covrsk", "xgb"): "best"}.get((d.base_kind, d.smooth_kind), "%s base, %s smoother" % (d.base_kind, d.smooth_kind))

    def _train_resident(self, data, retrain_base, evaluate, **smoother_kw):
        """train() on CUDA tensors, logistic base and tree smoother: the reference's steps in the reference's order with X, the base
        probabilities and the labels in HBM throughout.  The host receives the fitted arrays, the calibrator's 5 % sample and the
        A x A counts of the scored splits."""
        import torch
        (X_t1, y_t1), (X_t2, y_t2), (X_v, y_v) = data
        with resident.torch_stream(self.dev.ctx):
            self.train_base(X_t1, y_t1)
            B_t2 = self.base.predict_proba(X_t2)
            self.train_smoother(B_t2, y_t2, **smoother_kw)
            if self.calibrate:   # src/model.py:119-124
                self.smooth.train_calibrator(self.base.predict_proba(X_t1), y_t1)
                self.dev = self.smooth.dev
                self.base.dev = self.dev
            if evaluate:
                self.accuracies, self.Confusion_Matrices = self._score_splits(
                    {"train": ((X_t1, y_t1), (B_t2, y_t2)), "val": None if X_v is None else ((X_v, y_v), None)})
            del B_t2
            if retrain_base:
                parts = [(X_t1, y_t1), (X_t2, y_t2)] + ([(X_v, y_v)] if X_v is not None else [])
                X_all = resident.adjacent_rows([p[0] for p in parts])
                y_all = resident.adjacent_rows([p[1] for p in parts])
                if X_all is None:   # not one allocation's consecutive rows: concatenated in HBM
                    X_all = torch.cat([p[0] for p in parts])
                if y_all is None:
                    y_all = torch.cat([p[1] for p in parts])
                self.train_base(X_all, y_all)
        return self

    def train(self, data, retrain_base=True, evaluate=True, verbose=False, **smoother_kw):
        """Gnomix.train (src/model.py:104-167) on the device: base on train1, smoother on the base's probabilities of train2,
        the reference's accuracies / confusion matrices, base again on all the data.
        data = ((X_t1, y_t1), (X_t2, y_t2), (X_v, y_v)) with X_v possibly None.  Numpy arrays are staged through the device call
        by call; CUDA tensors (X torch.int8 with contiguous rows and any row stride, y torch.int32, as SimPlan.materialise_dev
        returns them) stay in HBM for the logistic base with the tree smoother, and are copied to the host once, with a warning,
        for every other pair.  A mixture of the two is a TypeError."""
        from time import time
        t0 = time()
        (X_t1, y_t1), (X_t2, y_t2), (X_v, y_v) = data
        if resident.all_on_device([X_t1, y_t1, X_t2, y_t2, X_v, y_v], "HipGnomix.train: data"):
            d = self.dev.data
            if d.base_kind in (None, "logistic") and d.smooth_kind in (None, "xgb"):
                self._train_resident(data, retrain_base, evaluate, **smoother_kw)
                self.time["training"] = round(time() - t0, 2)
                return self
            import warnings
            warnings.warn('HipGnomix.train: mode "%s" has no device-resident training path (the logistic base with the tree smoother, '
                          'mode "default", has); the splits are copied to the host once and the host-array path runs'
                          % self._resident_mode(), RuntimeWarning, stacklevel=2)
            (X_t1, y_t1), (X_t2, y_t2), (X_v, y_v) = [(resident.to_host(X), resident.to_host(y)) for X, y in data]
        self.train_base(X_t1, y_t1)
        B_t2 = self.base.predict_proba(X_t2)
        self.train_smoother(B_t2, y_t2, **smoother_kw)
        if self.calibrate:   # src/model.py:119-124: balanced w.r.t. the train1 class distribution
            self.smooth.train_calibrator(self.base.predict_proba(X_t1), y_t1)
            self.dev = self.smooth.dev
            self.base.dev = self.dev
        if evaluate:
            self.accuracies, self.Confusion_Matrices = self._score_splits(
                {"train": ((X_t1, y_t1), (B_t2, y_t2)), "val": None if X_v is None else ((X_v, y_v), None)})
        if retrain_base:
            from .train import svc_window_kernel
            if self.dev.data.base_kind == "covrsk" and svc_window_kernel(self.dev.data.svc[0]) == "CovRSK":
                # the reference's kernel calls between the two fits (its base predictions of train2 / val) leave numpy's global
                # generator where a CovRSK kernel call on the last window leaves it; this build's predictions do not touch it
                # (the RBF, plain and polynomial string kernels draw nothing: their models leave the generator alone)
                from .train import svc_rng_after_kernel
                svc_rng_after_kernel(self.data.window_width(self.W - 1))
            parts = [(X_t1, y_t1), (X_t2, y_t2)] + ([(X_v, y_v)] if X_v is not None else [])
            self.train_base(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        self.time["training"] = round(time() - t0, 2)
        return self

    def predict(self, X):
        """labels (N, W) — base + smoother fused on the device, B never leaves HBM (model.py:169-173); the smoother's mode_filter
        acts on them as in Smoother.predict"""
        mf = self.smooth.mode_filter
        if resident.is_cuda(X):   # CUDA in, CUDA out (int64, as the numpy form)
            import torch
            with resident.torch_stream(self.dev.ctx):
                _, lab = self.dev.infer_device(resident.check_x(X, self.C, self.dev.ctx.device), want_proba=False, want_labels=True)
                if mf:
                    lab = self.dev.mode_filter_device(lab, mf)
                return lab.to(torch.int64)
        _, lab = self.dev.infer(X, want_proba=False, want_labels=True)
        if mf:
            lab = self.dev.mode_filter(lab, mf)
        return lab.astype(np.int64)

    def predict_proba(self, X):
        """probabilities (N, W, A) (model.py:175-179)"""
        if resident.is_cuda(X):   # CUDA in, CUDA out, the dtype the numpy form returns
            import torch
            pd = torch.float64 if self.dev.proba_dtype() == np.float64 else torch.float32
            with resident.torch_stream(self.dev.ctx):
                p, _ = self.dev.infer_device(resident.check_x(X, self.C, self.dev.ctx.device), want_proba=True, want_labels=False,
                                             proba_dtype=pd)
            return p
        p, _ = self.dev.infer(X, want_proba=True, want_labels=False)
        return p

    def global_ancestry(self, X, weights=None, soft=False):
        """global ancestry proportions per individual, (N / 2, A) float64: the mean of the two haplotype rows of the weighted share
        of each ancestry (weights (W,), e.g. postprocess.window_weights(meta, "cM"); None = every window counts the same).  Hard
        calls come from the labels predict returns (mode_filter applied when set), soft=True from the probabilities predict_proba
        returns; with a CUDA tensor neither leaves HBM and a CUDA tensor comes back."""
        if X.shape[0] % 2:
            raise ValueError(f"global_ancestry: X holds {X.shape[0]} haplotype rows, an individual has two")
        mf = self.smooth.mode_filter
        if resident.is_cuda(X):
            import torch
            pd = torch.float64 if self.dev.proba_dtype() == np.float64 else torch.float32
            with resident.torch_stream(self.dev.ctx):
                p, lab = self.dev.infer_device(resident.check_x(X, self.C, self.dev.ctx.device), want_proba=bool(soft), want_labels=True,
                                               proba_dtype=pd)
                if mf:
                    lab = self.dev.mode_filter_device(lab, mf)
                s = self.dev.ancestry_summary_device(lab, weights, p)
                rows = s.soft if soft else s.hard
                return (rows[0::2] + rows[1::2]) / 2
        p, lab = self.dev.infer(X, want_proba=bool(soft), want_labels=True)
        if mf:
            lab = self.dev.mode_filter(lab, mf)
        s = self.dev.ancestry_summary(lab, weights, p)
        rows = s.soft if soft else s.hard
        return (rows[0::2] + rows[1::2]) / 2

    def allele_frequencies(self, X):
        """ancestry-specific allele counts of X under the labels predict returns (mode_filter applied when set) -> AlleleCounts of (A, C)
        int32 tables n_obs / n_alt / n_miss (postprocess.AlleleCounts; .freq() = n_alt / n_obs, NaN where nothing was observed), counted
        on the device (k_ancestry_allele_counts); with a CUDA tensor neither X nor the labels leave HBM and CUDA tensors come back.
        For re-phased haplotypes: X_phased, _ = model.phase(X); model.allele_frequencies(X_phased)"""
        with self._rows_and_labels(X) as (rows, lab, on_device):
            return (self.dev.ancestry_allele_counts_device if on_device else self.dev.ancestry_allele_counts)(rows, lab)

    def ancestry_association(self, X, y, Z=None, use=None, min_ac=1, model="linear"):
        """ancestry-specific association (the Tractor model) of X under the labels predict returns (mode_filter applied when set):
        per SNP, y = Z g + sum_{a < A-1} alpha_a hapcount_a + sum_a beta_a dosage_a by OLS over the individuals (rows 2 i, 2 i + 1)
        -> assoc.AncestryAssoc(beta, se, t, p, n_alt, n_hap, n, df, n_miss, status).  y (N / 2,), Z (N / 2, K) with the intercept
        column (None = the intercept only), use (N / 2,) bytes.  The sufficient statistics are reduced on the device
        (k_ancestry_assoc_snp); with a CUDA tensor neither X nor the labels leave HBM.  Results are numpy arrays.
        model="logistic": a case / control trait (y coded 0 / 1), the same terms with a logit link, fitted by maximum likelihood on the
        device (k_ancestry_assoc_logit_snp) -> assoc.AncestryAssocLogit.  Any other value: ValueError.
        A 2-D y is Y (N / 2, T): T quantitative traits at once (DeviceModel.ancestry_assoc_traits: D^T Y on the float64 matrix cores, one
        factorisation per SNP for all traits; complete cases across the traits) -> assoc.AncestryAssocTraits with beta, se, t, p shaped
        (C, A, T); ValueError where that exceeds 2 GiB (walk dev.ancestry_assoc_traits_chunks instead); with model="logistic":
        NotImplementedError."""
        if model not in ("linear", "logistic"):
            raise ValueError(f"model must be 'linear' or 'logistic', got {model!r}")
        if np.ndim(y) == 2:
            if model == "logistic":
                raise NotImplementedError("ancestry_association: several traits at once (a 2-D y) are fitted with model='linear' only")
            fit = lambda X, lab: self.dev.ancestry_assoc_traits(X, lab, y, Z, use, min_ac)
        else:
            fit = (lambda X, lab: self.dev.ancestry_assoc(X, lab, y, Z, use, min_ac)) if model == "linear" else (
                lambda X, lab: self.dev.ancestry_assoc_logit(X, lab, y, Z, use, min_ac))
        with self._rows_and_labels(X) as (rows, lab, _):
            return fit(rows, lab)

    def admixture_mapping(self, X, y_or_Y, Z=None, use=None, labels=None, min_hap=1, n_perm=0, seed=0):
        """admixture mapping: the regression of the trait(s) on the LOCAL ANCESTRY itself, window by window, under the labels predict
        returns for X (mode_filter applied when set), or under `labels` (N, W) (a numpy array or a CUDA tensor), in which case X is not
        looked at and no prediction runs.  y_or_Y (N / 2,) or (N / 2, T) (a 1-D y gives a trait axis of length 1); Z, use as
        ancestry_association takes them.  n_perm > 0: Freedman-Lane max-T permutations.  The blocks are reduced on the float64 matrix
        cores (k_ancestry_assoc_admix_main); with a CUDA tensor the labels never leave HBM -> admixmap.AdmixMap (numpy arrays; the
        module states the model, the status codes and how runs on several chromosomes combine)."""
        if labels is not None:
            return self.dev.admixture_map(labels, y_or_Y, Z, use, min_hap, n_perm, seed)
        with self._rows_and_labels(X) as (_, lab, _on_device):
            return self.dev.admixture_map(lab, y_or_Y, Z, use, min_hap, n_perm, seed)

    def ancestry_scores(self, X, weights, effect=None):
        """ancestry-partitioned polygenic scores ("partial PRS") of X under the labels predict returns (mode_filter applied when set):
        per individual (rows 2 i, 2 i + 1), ancestry a and score s, the sum of weights[c, a, s] over the SNPs c and the individual's
        haplotypes labelled a at c's window that carry the effect allele -> postprocess.AncestryScores(score (N / 2, A, S), n_effect,
        n_scored, n_miss (N / 2, A); .avg() = score / n_scored).  weights (C,), (C, A) or (C, A, S) (score.weights_from_assoc,
        score.read_score_file); effect None (ALT everywhere) or (C,) of 1 (ALT), 0 (REF), 255 (not scored).  One fused pass on the
        device (k_ancestry_score_partial); with a CUDA tensor neither X nor the labels leave HBM and CUDA tensors come back."""
        with self._rows_and_labels(X) as (rows, lab, on_device):
            return (self.dev.ancestry_scores_device if on_device else self.dev.ancestry_scores)(rows, lab, weights, effect)

    def ancestry_pair_counts(self, X, ancestry, snp_range=None):
        """the pairwise count tables of one ancestry (index into population_order) of X under the labels predict returns (mode_filter
        applied when set) -> asmds.PairCounts(DD, DO, OO), (N / 2, N / 2) int32 each: sums over the SNPs of d[i] d[j], d[i] o[j] and
        o[i] o[j], o = an individual's haplotypes labelled `ancestry` with an observed call, d = those of them that are ALT.  One fused
        pass on the int8 matrix cores (k_ancestry_pairs); with a CUDA tensor neither X nor the labels leave HBM and CUDA tensors come back."""
        with self._rows_and_labels(X) as (rows, lab, on_device):
            return (self.dev.ancestry_pair_counts_device if on_device else self.dev.ancestry_pair_counts)(rows, lab, ancestry, snp_range)

    def ancestry_mds(self, X, ancestry, k=4, min_sites=1000, min_pair_sites=None):
        """ancestry-specific MDS: the structure inside one ancestry component.  ancestry_pair_counts, then on the host (gnomix_amd.asmds)
        the individuals with at least min_sites compared sites of their own and min_pair_sites (default: min_sites) with every other
        kept individual (asmds.select), their allele-sharing distances mism / comp and classical MDS with k components ->
        asmds.AncestryMDS(coords (n_kept, k), eigenvalues, explained, kept, n_sites), or None when fewer than k + 1 individuals are kept"""
        from . import asmds
        counts = self.ancestry_pair_counts(X, ancestry)
        counts = asmds.PairCounts(*(t.cpu().numpy() if hasattr(t, "is_cuda") else t for t in counts))
        return asmds.ancestry_mds(counts, k=k, min_sites=min_sites, min_pair_sites=min_pair_sites)

    @contextmanager
    def _rows_and_labels(self, X, resident_rows=False):
        """X and the labels predict returns (mode_filter applied when set) -> (rows, labels, on_device) for the block.  A CUDA tensor is
        labelled in HBM (so is a numpy X with resident_rows: it is uploaded first) and the library stays bound to torch's current stream
        until the block ends, the op's own launch included; a numpy X is labelled through the host entry points"""
        mf = self.smooth.mode_filter
        if resident_rows or resident.is_cuda(X):
            import torch
            with resident.torch_stream(self.dev.ctx):
                if not resident.is_cuda(X):
                    X = torch.from_numpy(self.dev._x(X)).to("cuda:%d" % self.dev.ctx.device)
                X = resident.check_x(X, self.C, self.dev.ctx.device)
                _, lab = self.dev.infer_device(X, want_proba=False, want_labels=True)
                yield X, self.dev.mode_filter_device(lab, mf) if mf else lab, True
            return
        _, lab = self.dev.infer(X, want_proba=False, want_labels=True)
        yield self.dev._x(X), self.dev.mode_filter(lab, mf) if mf else lab, False

    def ancestry_ld(self, X, ancestry, c0=0, c1=None, band=256):
        """ancestry-specific LD: the banded count tables of one ancestry (index into population_order) of X under the labels predict
        returns (mode_filter applied when set), for the SNPs [c0, c1) and the offsets 0 .. band - 1 -> ld.LDCounts(n11, n1o, no1, noo, c0,
        band) of (c1 - c0, band) int32 arrays (.r(), .r2(), .pair(c, c')): sums over the haplotypes labelled `ancestry` at both SNPs with
        both calls observed.  One fused pass on the int8 matrix cores (k_ancestry_ld); with a CUDA tensor neither X nor the labels leave
        HBM and CUDA tensors come back."""
        with self._rows_and_labels(X) as (rows, lab, on_device):
            return (self.dev.ancestry_ld_counts_device if on_device else self.dev.ancestry_ld_counts)(rows, lab, ancestry, c0, c1, band)

    def ancestry_clump(self, X, res, p1=1e-4, p2=1e-2, r2=0.5, kb=250):
        """clumping of an association result (assoc.AncestryAssoc / AncestryAssocLogit of these SNPs) ancestry by ancestry -> index_of
        (C, A) int64: column a is ld.clump of res.p[:, a] with ancestry a's LD under the labels predict returns, at the model's SNP
        positions (an index SNP holds its own position in the SNP order, a clumped SNP its index's, -1 neither).  X and the labels stay
        in HBM; only the tables around index SNPs are computed and read back.  score.weights_from_assoc(res, index_of=...) takes it."""
        from . import ld
        pos = np.asarray(self.snp_pos).astype(np.int64)
        p = np.asarray(res.p, dtype=np.float64)
        if p.shape != (self.C, self.A):
            raise ValueError(f"res.p must be (C={self.C}, A={self.A}), got {p.shape}")
        band = ld.band_for(pos, kb)
        out = np.full((self.C, self.A), -1, np.int64)
        with self._rows_and_labels(X, resident_rows=True) as (Xt, lab, _):
            for a in range(self.A):
                def counts_for(c0, c1, a=a):
                    t = self.dev.ancestry_ld_counts_device(Xt, lab, a, c0, c1, band)
                    return ld.LDCounts(*(v.cpu().numpy() for v in t[:4]), t.c0, t.band)
                out[:, a] = ld.clump(p[:, a], pos, counts_for, p1=p1, p2=p2, r2=r2, kb=kb)
        return out

    def phase(self, X, B=None, verbose=False, **gnofix_kw):
        """Gnofix re-phasing (model.py:188-214): -> X_phased (N, C) int, Y_phased (N, W) int.  `gnofix_kw`: gnofix()'s search
        options (check_criterion, max_center_offset, non_lin_s, prob_comp, prior_switch_prob, padding, max_it); the reference's
        Gnomix.phase passes none, which is the default here too."""
        assert self.smooth is not None, "Smoother is not trained, returning original haplotypes"
        assert self.smooth.gnofix, "Type of Smoother ({}) does not currently support re-phasing".format(self.smooth)
        if self.smooth.mode_filter:
            # gnofix() takes its labels from smoother.predict (src/Gnofix/gnofix.py): the filter would act inside its loop
            raise NotImplementedError("phase: mode_filter != 0 inside the Gnofix loop is not built (predict applies it; phase does not)")
        X = np.asarray(X)
        if B is None:
            B = self.base.predict_proba(X)
        Xp, Y, _ = self.dev.gnofix(X, B, **gnofix_kw)
        return Xp.astype(int), Y.astype(int)
