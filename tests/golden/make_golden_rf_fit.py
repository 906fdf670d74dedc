#!/usr/bin/env python3
"""Generate tests/golden/G26_rf_fit.npz by RUNNING THE REFERENCE's RFBase (src/Base/models.py:54-66: per window sklearn
RandomForestClassifier(n_estimators=20, max_depth=4)) from the read-only checkout; nothing of it is copied here.

  G26_rf_fit.npz   RFBase.train (Base.train_vectorized, base.py:104-127) + Base.predict_proba (base.py:146-180) at C = 437, M = 50,
                   context 25 (W = 8, widths 100 and 137: rem > 0), A = 3, 60 fit rows, 24 queries: the inputs, the per-window seeds,
                   the fitted forests as rf_* arrays (gnomix_amd.convert.rforest_from_sklearn) and the base's predict_proba.

The reference fits in spawned workers with unseeded generators; here base_multithread is set to False and each window model's
random_state to its seed, so that the fit can be repeated.  Uses the import stubs of make_golden.py.  Skips cleanly when the reference
checkout is absent.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402  (the stubs and the checkout's location)
from rf_exact import make_problem  # noqa: E402

C, M, CX, A, N, NQ = 437, 50, 25, 3, 60, 24


def gen_g26(out_dir=HERE):
    if not os.path.isdir(MG.REF):
        print("G26 skipped: no reference checkout at", MG.REF)
        return None
    MG._stub_modules()
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    import sklearn
    import src.Base.models as RM
    from gnomix_amd.convert import rforest_from_sklearn
    W = C // M
    X, y0 = make_problem(A, C, N + NQ, 26)
    X, Xq = np.ascontiguousarray(X[:N]), np.ascontiguousarray(X[N:])
    rng = np.random.RandomState(2600)
    y = np.empty((N, W), np.int32)
    for w in range(W):   # labels that follow a few SNPs of the window, every class present
        y[:, w] = (X[:, w * M:w * M + 4].sum(axis=1) + rng.randint(0, 2, N)) % A
        y[:A, w] = np.arange(A)
    seeds = rng.randint(2 ** 31 - 1, size=W).astype(np.int64)
    base = RM.RFBase(chm_len=C, window_size=M, num_ancestry=A, missing_encoding=2, context=CX, n_jobs=1, seed=94305, verbose=False)
    base.base_multithread = False
    base.log_inference = False
    for m, s in zip(base.models, seeds):
        m.random_state = int(s)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base.train(X, y)
        B = np.asarray(base.predict_proba(Xq), dtype=np.float64)
    assert B.shape == (NQ, W, A) and np.all(np.isfinite(B))
    d = dict(sklearn_version=np.array(sklearn.__version__), C=C, M=M, ctx=CX, A=A, X=X, y=y, Xq=Xq, seeds=seeds, B=B)
    d.update(rforest_from_sklearn(base.models, A))
    path = os.path.join(out_dir, "G26_rf_fit.npz")
    np.savez_compressed(path, **d)
    print("G26 written:", path, os.path.getsize(path), "bytes;", len(d["rf_left"]), "nodes")
    return path


if __name__ == "__main__":
    gen_g26()
