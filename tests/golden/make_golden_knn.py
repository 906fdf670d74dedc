#!/usr/bin/env python3
"""Generate tests/golden/G22_knn.npz by RUNNING THE REFERENCE's KNNBase (src/Base/models.py:135-146: per window
sklearn.neighbors.KNeighborsClassifier(n_neighbors=1)) from the read-only checkout; nothing of it is copied here.

  G22_knn.npz   KNNBase.train (Base.train_vectorized, base.py:104-127) + Base.predict_proba (base.py:146-180) on a small
                synthetic panel (G21's: C = 1237, M = 100, ctx = 50, A = 4, 240 fit rows, 60 queries, 1 % missing): the inputs,
                every window's _fit_X (int8) and labels classes_[_y], predict_proba of the queries, and per (query, window)
                whether the set of minimum-distance fit rows carries more than one label (`ambiguous`, computed in numpy
                with integer distances).

scikit-learn's choice among equidistant neighbours is unspecified, so the fixture must be (almost) free of label-ambiguous
cells: the generator ASSERTS that their share is <= 2 % of the 60 x 12 cells (with 200-wide random windows it is 0).  That is
a condition on the fixture, not a tolerance of any test.
base_multithread is set to False (the reference fits KNNBase's windows in spawned workers; a 1-NN fit has no randomness).
The panel is make_golden_svm.py's with ONE change: fit rows and queries share the ancestries' allele frequencies (G21 draws
new ones for its queries, which makes every query equally far from every ancestry: 11.7 % of the cells are then label-ambiguous).
Uses the import stubs of make_golden.py.  Skips cleanly when the reference checkout is absent.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (the stubs and the checkout's location)
import knn_exact as KE  # noqa: E402  (tests/knn_exact.py: integer distances)


def panel(rng, freq, n, W, M, miss):
    """haplotypes whose allele frequencies freq (A, C) depend on the ancestry of the window; the first 4 A rows are
    single-ancestry so that every window holds every class"""
    A, C = freq.shape
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


def gen_g22(out_dir=HERE):
    if not os.path.isdir(MG.REF):
        print("G22 skipped: no reference checkout at", MG.REF)
        return None
    MG._stub_modules()
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    from src.Base.models import KNNBase
    rng = np.random.RandomState(22)
    C, M, A, ctx = 1237, 100, 4, 50
    W = C // M
    freq = rng.uniform(0.05, 0.95, size=(A, C))
    Xt, yt = panel(rng, freq, 240, W, M, 0.01)
    Xq, _ = panel(rng, freq, 60, W, M, 0.01)
    base = KNNBase(chm_len=C, window_size=M, num_ancestry=A, missing_encoding=2, context=ctx, n_jobs=1, seed=94305, verbose=False)
    base.base_multithread = False
    base.log_inference = False
    base.train(Xt, yt)
    B = np.asarray(base.predict_proba(Xq), dtype=np.float64)
    assert B.shape == (60, W, A) and set(np.unique(B).tolist()) <= {0.0, 1.0}
    d = dict(C=C, M=M, A=A, ctx=ctx, Xt=Xt, yt=yt.astype(np.int32), Xq=Xq, B=B)
    wins = []
    for i, m in enumerate(base.models):
        assert list(m.classes_) == list(range(A)) and m.n_neighbors == 1
        fx = np.asarray(m._fit_X)
        assert np.array_equal(fx, np.rint(fx)) and fx.min() >= 0 and fx.max() <= 2
        lab = np.asarray(m.classes_)[np.asarray(m._y)].astype(np.int32)
        d["w%d_fit_X" % i] = fx.astype(np.int8)
        d["w%d_y" % i] = lab
        wins.append((fx.astype(np.int8), lab))
    _, _, amb = KE.predict(Xq, wins, C, M, ctx, A)
    share = float(amb.mean())
    print("G22: ambiguous cells %d of %d (%.3f %%)" % (int(amb.sum()), amb.size, 100 * share))
    assert share <= 0.02, "the fixture has too many label-ambiguous cells: choose another seed"
    d["ambiguous"] = amb
    path = os.path.join(out_dir, "G22_knn.npz")
    np.savez_compressed(path, **d)
    print("G22 written:", path, os.path.getsize(path), "bytes")
    return path


if __name__ == "__main__":
    gen_g22()
