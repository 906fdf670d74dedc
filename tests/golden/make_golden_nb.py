#!/usr/bin/env python3
"""Generate tests/golden/G23_nb.npz by RUNNING THE REFERENCE's three Naive-Bayes bases (src/Base/models.py:96-132: per window
sklearn GaussianNB() / BernoulliNB(alpha=0) / MultinomialNB(alpha=0)) from the read-only checkout; nothing of it is copied here.

  G23_nb.npz   NB*Base.train (Base.train_vectorized, base.py:104-127) + Base.predict_proba (base.py:146-180) on a small synthetic
               panel (make_golden_knn.panel; RandomState(23), C = 257, M = 20, ctx = 5, A = 4, allele frequencies ~ U(0.2, 0.8), 240
               fit rows then 60 queries, 1 % missing): the inputs, every window's fitted attributes and each base's predict_proba.

The windows are narrow and the frequencies moderate on purpose: with M = 100 the top probability of 83-99 % of the query rows is
above 1 - 1e-9 and the fixture would check little but the argmax.  The generator ASSERTS that every attribute is finite (with
scikit-learn >= 1.4 alpha=0 stays a true 0 and a class-monomorphic SNP gives log 0; this panel has none), that every window holds
every class, and that no query row's top probability exceeds 1 - 1e-9.  Those are conditions on the fixture, not tolerances.
base_multithread is set to False (a Naive-Bayes fit has no randomness).  Uses the import stubs of make_golden.py.  Skips cleanly
when the reference checkout is absent.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (the stubs and the checkout's location)
from make_golden_knn import panel  # noqa: E402

KINDS = {"bernoulli": ("NBBernoulliBase", ("feature_log_prob_", "class_log_prior_")),
         "multinomial": ("NBMultinomialBase", ("feature_log_prob_", "class_log_prior_")),
         "gaussian": ("NBGaussianBase", ("theta_", "var_", "class_prior_"))}


def gen_g23(out_dir=HERE):
    if not os.path.isdir(MG.REF):
        print("G23 skipped: no reference checkout at", MG.REF)
        return None
    MG._stub_modules()
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    import src.Base.models as RM
    rng = np.random.RandomState(23)
    C, M, A, ctx = 257, 20, 4, 5
    W = C // M
    freq = rng.uniform(0.2, 0.8, size=(A, C))
    Xt, yt = panel(rng, freq, 240, W, M, 0.01)
    Xq, _ = panel(rng, freq, 60, W, M, 0.01)
    d = dict(C=C, M=M, A=A, ctx=ctx, Xt=Xt, yt=yt.astype(np.int32), Xq=Xq)
    for kind, (cls, names) in KINDS.items():
        base = getattr(RM, cls)(chm_len=C, window_size=M, num_ancestry=A, missing_encoding=2, context=ctx, n_jobs=1, seed=94305,
                                verbose=False)
        base.base_multithread = False
        base.log_inference = False
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            base.train(Xt, yt)
            B = np.asarray(base.predict_proba(Xq), dtype=np.float64)
        assert B.shape == (60, W, A) and np.all(np.isfinite(B))
        assert B.max(axis=2).max() <= 1.0 - 1e-9, "a query row is saturated: the fixture would not exercise the probabilities"
        d[kind + "_B"] = B
        for i, m in enumerate(base.models):
            assert list(m.classes_) == list(range(A)), "every window must hold every class"
            for nm in names:
                v = np.asarray(getattr(m, nm), dtype=np.float64)
                assert np.all(np.isfinite(v)), (kind, i, nm)
                d["%s_w%d_%s" % (kind, i, nm)] = v
        print("G23 %-11s top probability max %.12f" % (kind, B.max(axis=2).max()))
    path = os.path.join(out_dir, "G23_nb.npz")
    np.savez_compressed(path, **d)
    print("G23 written:", path, os.path.getsize(path), "bytes")
    return path


if __name__ == "__main__":
    gen_g23()
