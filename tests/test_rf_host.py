"""The random-forest base trainer on the CPU: the plain-Python restatement (tests/rf_exact.py) against live scikit-learn, bit for bit;
the reference's RFBase fit (G26) against the restatement; the untrained model, the accepted-names message, header and binding."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rf_exact as E  # noqa: E402

# (A, width, N, seed): widths 17..349 with non-multiples of 16, N 8..200; make_problem puts code 2, duplicated columns (an eighth),
# constant columns (an eighth) and columns of 0s and 2s only into every one
PROBLEMS = [(2, 17, 24, 1), (3, 33, 8, 2), (7, 349, 200, 3), (3, 64, 60, 4), (2, 100, 37, 5), (7, 237, 150, 6), (3, 75, 100, 7),
            (2, 48, 12, 8), (7, 200, 64, 9), (3, 129, 33, 10), (2, 300, 50, 11)]
TREE_ARRAYS = ("children_left", "children_right", "feature", "threshold")


def _against_sklearn(X, y, A, seed, counters):
    from sklearn.ensemble import RandomForestClassifier
    rf = RandomForestClassifier(n_estimators=20, max_depth=4, random_state=seed).fit(X, y)
    mine = E.fit_forest(X, y, A, seed, counters=counters)
    assert len(mine) == len(rf.estimators_) == 20
    nodes = 0
    for i, (e, m) in enumerate(zip(rf.estimators_, mine)):
        t = e.tree_
        for k in TREE_ARRAYS:
            a, b = getattr(t, k), m[k]
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (i, k)
        assert t.value.dtype == np.float64 and np.array_equal(t.value[:, 0, :], m["value"]), (i, "value")
        nodes += t.node_count
    return nodes


def test_restatement_equals_live_scikit_learn_bit_for_bit():
    sklearn = pytest.importorskip("sklearn")
    counters = E.new_counters()
    nodes = 0
    for A, width, N, seed in PROBLEMS:
        X, y = E.make_problem(A, width, N, seed)
        assert 2 in X and sorted(set(y.tolist())) == list(range(A))
        nodes += _against_sklearn(X, y, A, seed, counters)
    # four identical row pairs with different labels: impure nodes whose every column is constant, leaves above depth 4
    X, y = E.identical_pairs(4, 40)
    before = dict(counters)
    nodes += _against_sklearn(X, y, 2, 3, counters)
    assert counters["all_constant_search"] > before["all_constant_search"] and counters["leaf_above_max_depth"] > before["leaf_above_max_depth"]
    print("scikit-learn", sklearn.__version__, "nodes", nodes, counters)
    for k in E.COUNTER_NAMES:     # the inputs cannot quietly stop covering these branches
        assert counters[k] > 0, k


def test_bootstrap_of_the_package_equals_the_restatements():
    from gnomix_amd.train import rforest_bootstrap
    wt, st = rforest_bootstrap([5, 2 ** 31 - 2], 20, 37)
    for w, seed in enumerate((5, 2 ** 31 - 2)):
        ew, es = E.bootstrap(seed, 20, 37)
        assert np.array_equal(wt[w], ew) and np.array_equal(st[w], es) and wt[w].sum(axis=1).tolist() == [37] * 20
    assert st.dtype == np.uint32 and wt.shape == (2, 20, 37)


def test_reference_fit_G26_equals_the_restatement():
    g = load_golden("G26_rf_fit.npz")
    C, M, cx, A = int(g["C"]), int(g["M"]), int(g["ctx"]), int(g["A"])
    assert C - M * (C // M) > 0 and cx > 0
    ref = E.fit_windows(g["X"], g["y"], M, cx, A, g["seeds"])
    for k, v in ref.items():
        assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), k


def test_untrained_model_placeholder_and_names(oracle, tmp_path):
    from gnomix_amd import _lib
    from gnomix_amd.model import GnxModelData
    from gnomix_amd.train import untrained_model
    C, M, cx = 437, 50, 25
    for A in (2, 7):
        d = untrained_model(C, M, A, 5, cx, "default", base="rf", seed=1)
        W = C // M
        assert d.base_kind == "rforest" and d.smooth_kind == "xgb" and d.rf_train == dict(n_trees=20, max_depth=4)
        assert d.rf_win_tree0.tolist() == list(range(W + 1)) and d.rf_tree_off.tolist() == list(range(W + 1))
        assert d.rf_left.tolist() == [-1] * W == d.rf_right.tolist() and d.rf_value.shape == (W, A) and d.rf_thr.dtype == np.float64
        Xq = np.random.RandomState(A).randint(0, 3, (9, C)).astype(np.int8)
        rf = dict(win_tree0=d.rf_win_tree0, tree_off=d.rf_tree_off, left=d.rf_left, right=d.rf_right, feat=d.rf_feat, thr=d.rf_thr,
                  value=d.rf_value)
        assert np.array_equal(oracle.base_rforest(rf, Xq, M, cx, A), np.full((9, W, A), 1.0 / A))
        desc, keep = d.to_desc()
        assert desc.base_kind == _lib.BASE_RFOREST
        path = str(tmp_path / ("rf%d.gnx" % A))
        d.save(path)      # the hyper-parameters stay in memory
        assert "rf_train" not in np.load(path, allow_pickle=False).files
        e = GnxModelData.load(path)
        assert e.base_kind == "rforest" and e.rf_train is None and np.array_equal(e.rf_value, d.rf_value)
    with pytest.raises(ValueError, match=r'"rf" \(RFBase') as err:
        untrained_model(C, M, 3, 5, cx, "default", base="forest")
    for word in ("svm", "xgb", "knn", "nb_bernoulli", "nb_multinomial", "nb_gaussian", "lda_svd"):
        assert word in str(err.value)


def test_train_rforest_base_refuses_bad_inputs_before_touching_the_device():
    from gnomix_amd.train import train_rforest_base, untrained_model
    C, M, A, cx = 53, 20, 3, 4
    d = untrained_model(C, M, A, 1, cx, "default", base="rf")
    X, y = np.zeros((6, C), np.int8), np.tile(np.array([0, 1, 2, 0, 1, 2], np.int32)[:, None], (1, 2))
    y1 = y.copy()
    y1[:, 1] = np.where(y1[:, 1] == 2, 0, y1[:, 1])
    for Xb, yb, word in ((X[:, :-1], y, "X must be"), (X + 3, y, "codes"), (X.astype(np.float64) + 0.5, y, "whole"), (X, y[:, :1], "y must be"),
                         (X, y + 1, "labels"), (X, y1, "window 1: class 2 has no row")):
        with pytest.raises(ValueError, match=word):
            train_rforest_base(d, Xb, yb)


def test_header_and_binding_agree():
    from gnomix_amd import _lib
    h = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    assert "#define GNX_ABI_VERSION 16\n" in h and _lib.GNX_ABI_VERSION == 16
    assert re.search(r"gnx_train_rforest\s+<- Base\.train\(X, y\) of RFBase\s+src/Base/models\.py:54-66", h)
    for name in ("gnx_train_rforest", "gnx_train_rforest_dev"):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == 21
        m = re.search(r"\bint %s\(([^;]*)\);" % name, h)
        assert m and len(m.group(1).split(",")) == 21
    lib = _lib.load()
    assert lib.gnx_abi_version() == 16 and hasattr(lib, "gnx_train_rforest") and hasattr(lib, "gnx_train_rforest_dev")
