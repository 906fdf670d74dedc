#!/usr/bin/env python3
"""Generate tests/golden/G25_lda_base.npz by RUNNING THE REFERENCE's LDABase (src/Base/models.py:83-94: per window sklearn
LinearDiscriminantAnalysis()) from the read-only checkout; nothing of it is copied here.

  G25_lda_base.npz   LDABase.train (Base.train_vectorized, base.py:104-127) + Base.predict_proba (base.py:146-180) on the panel of
                     tests/lda_exact.sixth_panel (C = 203, M = 24, context 12: W = 8, widths 48 and 59; 96 fit rows, 64 queries; window
                     0 with duplicated and constant columns, window 3 with columns constant within every class), once with A = 3 and
                     once with A = 2: the inputs, every window's coef_ / intercept_ and the base's predict_proba.

The generator ASSERTS that every window holds every class and that every stored value is finite.  base_multithread is set to False (an
LDA fit has no randomness).  Uses the import stubs of make_golden.py.  Skips cleanly when the reference checkout is absent.
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
from lda_exact import sixth_panel  # noqa: E402


def gen_g25(out_dir=HERE):
    if not os.path.isdir(MG.REF):
        print("G25 skipped: no reference checkout at", MG.REF)
        return None
    MG._stub_modules()
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    import sklearn
    import src.Base.models as RM
    d = dict(sklearn_version=np.array(sklearn.__version__))
    for A in (3, 2):
        (C, M, cx, _), X, y, Xq = sixth_panel(A=A)
        W = C // M
        base = RM.LDABase(chm_len=C, window_size=M, num_ancestry=A, missing_encoding=2, context=cx, n_jobs=1, seed=94305, verbose=False)
        base.base_multithread = False
        base.log_inference = False
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            base.train(X, y)
            B = np.asarray(base.predict_proba(Xq), dtype=np.float64)
        assert B.shape == (len(Xq), W, A) and np.all(np.isfinite(B))
        pre = "A%d_" % A
        d.update({pre + "C": C, pre + "M": M, pre + "ctx": cx, pre + "X": X, pre + "y": y.astype(np.int32), pre + "Xq": Xq, pre + "B": B})
        for i, m in enumerate(base.models):
            assert list(m.classes_) == list(range(A)), "every window must hold every class"
            for nm in ("coef_", "intercept_"):
                v = np.asarray(getattr(m, nm), dtype=np.float64)
                assert np.all(np.isfinite(v)), (A, i, nm)
                d["%sw%d_%s" % (pre, i, nm)] = v
        print("G25 A = %d: top probability in [%.6f, %.12f]" % (A, B.max(axis=2).min(), B.max(axis=2).max()))
    path = os.path.join(out_dir, "G25_lda_base.npz")
    np.savez_compressed(path, **d)
    print("G25 written:", path, os.path.getsize(path), "bytes")
    return path


if __name__ == "__main__":
    gen_g25()
