"""The plain and the polynomial string-kernel SVC bases without a GPU: the C ABI stays 16 and gains its entries, the trainer's
kernel names, untrained_model's placeholders and their C description, the window tag through a .gnx round trip, and the fixture
G27 (the reference's own StringKernelBase / PolynomialStringKernelBase fits) explained by sklearn on the oracle's Gram matrices with
the seeds the sequential fits draw."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("gnx_train_svc_poly", "gnx_train_svc_poly_dev", "gnx_svc_gram")


def test_abi_is_16_and_the_new_entries_are_declared_bound_and_exported():
    from gnomix_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnomix_hip.h")).read()
    assert re.search(r"#define GNX_ABI_VERSION 16\b", header) and _lib.GNX_ABI_VERSION == 16
    lib = _lib.load()
    assert lib.gnx_abi_version() == 16
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(gnx_ctx\* ctx," % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"^ \*   %s\s+<-" % name, header, re.M) or name.endswith("_dev"), name   # the entry-to-reference table


def test_kernel_names_of_the_trainer():
    from gnomix_amd import train as T
    assert T.SVC_KERNEL_KINDS == {"CovRSK": 0, "string_kernel": 2}
    assert T.SVC_TRAIN_KINDS == {"CovRSK": 0, "string_kernel": 2, "rbf": 3, "poly_kernel": 1}
    assert T.svc_window_kernel(dict(ms=np.arange(3))) == "CovRSK"                         # untagged: as before
    assert T.svc_window_kernel(dict(poly_p=1.2, run_value=np.zeros(4))) == "CovRSK"       # an untagged converted pickle too
    assert T.svc_window_kernel(dict(kernel=np.array("rbf"))) == "rbf"
    with pytest.raises(ValueError):
        T.svc_window_kernel(dict(kernel=np.array("sigmoid")))
    with pytest.raises(ValueError):
        T.train_svc_arrays(np.zeros((4, 8), np.int8), np.zeros((4, 2), np.int32), 4, 0, 2, np.zeros(2), kernel="poly")


@pytest.mark.parametrize("base_name,tag,kind", [("string_kernel", "string_kernel", 0), ("poly_string_kernel", "poly_kernel", 1)])
def test_placeholders_their_description_and_the_tag_through_a_gnx(tmp_path, base_name, tag, kind):
    from gnomix_amd import GnxModelData, _lib
    from gnomix_amd.model import svc_window_is_rbf
    from gnomix_amd.train import untrained_model, svc_window_kernel
    C, M, ctx, A = 83, 40, 3, 3
    d = untrained_model(C, M, A, 1, ctx, "default", base=base_name)
    assert d.base_kind == "covrsk" and len(d.svc) == d.W == 2 and d.smooth_kind == "xgb"
    path = str(tmp_path / "m.gnx")
    d.save(path)
    again = GnxModelData.load(path)
    for m in (d, again):
        for w, s in enumerate(m.svc):
            width = m.window_width(w)
            assert svc_window_kernel(s) == tag and not svc_window_is_rbf(s) and s["xfit"].shape == (A, width)
            if kind == 1:
                assert float(s["poly_p"]) == 1.2 and np.array_equal(s["run_value"], np.arange(width + 1) ** 1.2) and "ms" not in s
            else:
                assert np.array_equal(s["ms"], np.arange(1, width + 1)) and "poly_p" not in s
        desc, keep = m.to_desc()
        assert desc.base_kind == _lib.BASE_COVRSK_SVC
        arr = ctypes.cast(desc.svc, ctypes.POINTER(_lib.SvcWindow))
        for w in range(m.W):
            width = m.window_width(w)
            assert arr[w].kernel_kind == kind and arr[w].width == width and arr[w].n_sv == A
            if kind == 1:
                assert arr[w].poly_p == 1.2 and arr[w].run_value and not arr[w].ms
            else:
                assert arr[w].n_ms == width and arr[w].ms      # GNX_SVC_KERNEL_SUBSTRINGS over every length
    for a, b in zip(again.svc, d.svc):
        assert set(a) == set(b)
        for k in b:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_unknown_base_names_are_refused_with_every_name_listed():
    from gnomix_amd.train import untrained_model
    for bad in ("lda", "poly_kernel", "polynomial"):
        with pytest.raises(ValueError) as e:
            untrained_model(83, 40, 3, 1, 3, "default", base=bad)
        msg = str(e.value)
        for part in ("svm", "xgb", '"rf" (RFBase', "knn", "nb_bernoulli", "nb_multinomial", "nb_gaussian", "lda_svd",
                     '"string_kernel" (StringKernelBase', '"poly_string_kernel" (PolynomialStringKernelBase'):
            assert part in msg, part


def test_unchained_seeds_are_the_generators_first_draws():
    from gnomix_amd.train import svc_seeds_unchained, SVC_SEED_HIGH
    np.random.seed(99)
    s = svc_seeds_unchained(5)
    ref = np.random.RandomState(99)
    assert np.array_equal(s, ref.randint(SVC_SEED_HIGH, size=5).astype(np.uint32))
    st, st_ref = np.random.get_state(), ref.get_state()
    assert np.array_equal(st[1], st_ref[1]) and st[2] == st_ref[2]


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300) + 1e-300)


def test_G27_is_sklearn_on_the_oracles_gram_with_the_sequential_seeds(oracle):
    """what the GPU test of the fixture rests on: the reference's fits are libsvm on these integer Gram matrices, seeded with
    RandomState(np_seed).randint(2**31 - 1) window by window (no seed chain, no re-seeding by the kernels)"""
    from sklearn.svm import SVC
    from gnomix_amd.convert import poly_run_values
    from gnomix_amd.train import window_columns, SVC_SEED_HIGH
    g = load_golden("G27_sk_train.npz")
    C, M, A, ctx = int(g["C"]), int(g["M"]), int(g["A"]), int(g["ctx"])
    W = C // M
    assert C % M > 0 and (g["Xt"] == 2).any() and all(len(np.unique(g["yt"][:, w])) == A for w in range(W))
    assert np.array_equal(g["seeds"], np.random.RandomState(int(g["np_seed"])).randint(SVC_SEED_HIGH, size=W).astype(np.uint32))
    rv = poly_run_values(M + 2 * ctx + C % M, float(g["poly_p"]))["run_value"]
    X0 = g["Xt"][:, window_columns(C, M, ctx, 0)]
    assert np.array_equal(oracle.poly_kernel(X0, X0, rv, float(g["poly_p"])), g["pk_K0"])
    for pre in ("sk_", "pk_"):
        rs = np.random.RandomState(int(g["np_seed"]))   # one generator through all windows, as numpy's global one in the reference
        for w in range(W):
            Xw = g["Xt"][:, window_columns(C, M, ctx, w)]
            K = oracle.string_kernel(Xw, Xw) if pre == "sk_" else oracle.poly_kernel(Xw, Xw, rv, float(g["poly_p"]))
            assert K.max() < 2 ** 24
            sk = SVC(kernel="precomputed", probability=True, random_state=rs).fit(K.astype(np.float64), g["yt"][:, w])
            assert np.array_equal(sk.support_, g["%sw%d_support" % (pre, w)]) and np.array_equal(sk._n_support, g["%sw%d_n_support" % (pre, w)])
            assert np.max(np.abs(sk._dual_coef_ - g["%sw%d_dual" % (pre, w)])) <= 1e-12
            assert np.max(np.abs(sk._intercept_ - g["%sw%d_intercept" % (pre, w)])) <= 1e-12
            assert _close(sk._probA, g["%sw%d_probA" % (pre, w)], 1e-10) and _close(sk._probB, g["%sw%d_probB" % (pre, w)], 1e-10)
        assert g[pre + "B"].shape == (len(g["Xq"]), W, A)
