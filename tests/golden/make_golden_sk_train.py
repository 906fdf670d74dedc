#!/usr/bin/env python3
"""Generate tests/golden/G27_sk_train.npz by RUNNING THE REFERENCE's StringKernelBase and PolynomialStringKernelBase
(src/Base/models.py:161-193: per window sklearn.svm.SVC(kernel=<callable>, probability=True)) from the read-only checkout;
nothing of it is copied here.

  G27_sk_train.npz  Base.train (base.py:104-127) + Base.predict_proba (base.py:146-180) of both bases on one small synthetic
                    panel (make_golden_svm.panel): the inputs, every window's fitted arrays (support_, _dual_coef_, _intercept_,
                    _probA, _probB, _n_support) under the prefixes sk_ (StringKernelBase) and pk_ (PolynomialStringKernelBase),
                    the libsvm seeds the fits drew, predict_proba of the query haplotypes (sk_B, pk_B), and window 0's
                    poly_kernel(Xw, Xw) matrix (pk_K0).

Both bases fit their windows sequentially (base_multithread = False) and neither kernel touches numpy's global generator, so after
np.random.seed(SEED) window w's libsvm seed is the w-th `randint(np.iinfo("i").max)` of RandomState(SEED) (BaseLibSVM.fit).
Uses the import stubs of make_golden.py.  Skips cleanly when the reference checkout is absent.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (the stubs and the checkout's location)
from make_golden_svm import panel  # noqa: E402

SEED = 2727


def gen_g27(out_dir=HERE):
    if not os.path.isdir(MG.REF):
        print("G27 skipped: no reference checkout at", MG.REF)
        return None
    MG._stub_modules()
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    import numpy
    from src.Base import models as RM
    from src.Base.string_kernel import poly_kernel
    rng = np.random.RandomState(27)
    C, M, A, ctx = 643, 100, 3, 50
    W = C // M
    Xt, yt = panel(rng, 60, C, A, W, M, 0.01)
    Xq, _ = panel(rng, 20, C, A, W, M, 0.01)
    seeds = np.random.RandomState(SEED).randint(np.iinfo("i").max, size=W).astype(np.uint32)
    d = dict(C=C, M=M, A=A, ctx=ctx, Xt=Xt, yt=yt.astype(np.int32), Xq=Xq, seeds=seeds, np_seed=SEED, poly_p=1.2)
    for pre, name in (("sk_", "StringKernelBase"), ("pk_", "PolynomialStringKernelBase")):
        real_ver = numpy.__version__
        numpy.__version__ = "1.26.4"  # models.py:166 / :183 parse the MINOR version ("2.2.6" -> 2 < 20)
        try:
            base = getattr(RM, name)(chm_len=C, window_size=M, num_ancestry=A, missing_encoding=2, context=ctx, n_jobs=1, seed=94327,
                                     verbose=False)
        finally:
            numpy.__version__ = real_ver
        assert base.base_multithread is False
        base.log_inference = False
        np.random.seed(SEED)
        base.train(Xt, yt)
        d[pre + "B"] = np.asarray(base.predict_proba(Xq))
        for i, m in enumerate(base.models):
            assert list(m.classes_) == list(range(A)) and callable(m.kernel)
            d["%sw%d_support" % (pre, i)] = m.support_.astype(np.int32)
            d["%sw%d_dual" % (pre, i)] = m._dual_coef_
            d["%sw%d_intercept" % (pre, i)] = m._intercept_
            d["%sw%d_probA" % (pre, i)] = m._probA
            d["%sw%d_probB" % (pre, i)] = m._probB
            d["%sw%d_n_support" % (pre, i)] = np.asarray(m._n_support, dtype=np.int32)
    Xp = np.concatenate([Xt[:, :ctx][:, ::-1], Xt, Xt[:, -ctx:][:, ::-1]], axis=1)   # base.py:41-44
    d["pk_K0"] = poly_kernel(Xp[:, :M + 2 * ctx], Xp[:, :M + 2 * ctx], p=1.2)
    path = os.path.join(out_dir, "G27_sk_train.npz")
    np.savez_compressed(path, **d)
    print("G27 written:", path, os.path.getsize(path), "bytes")
    return path


if __name__ == "__main__":
    gen_g27()
