#!/usr/bin/env python3
"""Generate tests/golden/G21_svm_rbf.npz by RUNNING THE REFERENCE's SVMBase (src/Base/models.py:148-159:
per window sklearn.svm.SVC(C=100., gamma=0.001, probability=True)) from the read-only checkout; nothing of it is copied here.

  G21_svm_rbf.npz   SVMBase.train (Base.train_vectorized, base.py:104-127) + Base.predict_proba (base.py:146-180) on a small
                    synthetic panel: inputs, every window's fitted arrays (support_, _dual_coef_, _intercept_, _probA, _probB,
                    _n_support, _gamma), the libsvm seeds the fits drew, and predict_proba of the query haplotypes.

The reference fits SVMBase's windows in spawned workers with unseeded generators (base_multithread = True); here
base_multithread is set to False and numpy's global generator is seeded, so the fits are sequential and reproducible: window w's
libsvm seed is the w-th `randint(np.iinfo("i").max)` of RandomState(SEED) (BaseLibSVM.fit; no kernel call reseeds anything).
Uses the import stubs of make_golden.py.  Skips cleanly when the reference checkout is absent.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (the stubs and the checkout's location)

SEED = 2121


def panel(rng, n, C, A, W, M, miss):
    """haplotypes whose allele frequencies depend on the ancestry of the window; the first 4 A rows are single-ancestry so that
    every window holds every class"""
    freq = rng.uniform(0.05, 0.95, size=(A, C))
    y = np.empty((n, W), dtype=np.int64)
    for i in range(n):
        if i < 4 * A:
            y[i] = i % A
        else:
            cuts = np.sort(rng.choice(np.arange(1, W), size=rng.randint(0, 3), replace=False))
            lab, prev = rng.randint(A), 0
            for c in list(cuts) + [W]:
                y[i, prev:c] = lab
                lab, prev = rng.randint(A), c
    anc = np.repeat(y, M, axis=1)
    anc = np.concatenate([anc, np.repeat(anc[:, -1:], C - anc.shape[1], axis=1)], axis=1)   # the last window takes the remainder
    X = (rng.uniform(size=(n, C)) < freq[anc, np.arange(C)[None, :]]).astype(np.int8)
    X[rng.uniform(size=X.shape) < miss] = 2
    return X, y


def gen_g21(out_dir=HERE):
    if not os.path.isdir(MG.REF):
        print("G21 skipped: no reference checkout at", MG.REF)
        return None
    MG._stub_modules()
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    from src.Base.models import SVMBase
    rng = np.random.RandomState(21)
    C, M, A, ctx = 1237, 100, 4, 50
    W = C // M
    Xt, yt = panel(rng, 240, C, A, W, M, 0.01)
    Xq, _ = panel(rng, 60, C, A, W, M, 0.01)
    base = SVMBase(chm_len=C, window_size=M, num_ancestry=A, missing_encoding=2, context=ctx, n_jobs=1, seed=94305, verbose=False)
    base.base_multithread = False
    base.log_inference = False
    np.random.seed(SEED)
    base.train(Xt, yt)
    B = np.asarray(base.predict_proba(Xq))
    seeds = np.random.RandomState(SEED).randint(np.iinfo("i").max, size=W).astype(np.uint32)
    d = dict(C=C, M=M, A=A, ctx=ctx, Xt=Xt, yt=yt.astype(np.int32), Xq=Xq, B=B, seeds=seeds, np_seed=SEED, svc_C=100.0)
    for i, m in enumerate(base.models):
        assert list(m.classes_) == list(range(A)) and m.kernel == "rbf"
        d["w%d_support" % i] = m.support_.astype(np.int32)
        d["w%d_dual" % i] = m._dual_coef_
        d["w%d_intercept" % i] = m._intercept_
        d["w%d_probA" % i] = m._probA
        d["w%d_probB" % i] = m._probB
        d["w%d_n_support" % i] = np.asarray(m._n_support, dtype=np.int32)
        d["w%d_gamma" % i] = np.float64(m._gamma)
    path = os.path.join(out_dir, "G21_svm_rbf.npz")
    np.savez_compressed(path, **d)
    print("G21 written:", path, os.path.getsize(path), "bytes")
    return path


if __name__ == "__main__":
    gen_g21()
