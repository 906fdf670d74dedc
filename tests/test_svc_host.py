"""Host side of the CovRSK SVC trainer (no GPU): the libsvm seeds the reference's window fits use, the Platt fold permutation against
sklearn's own generator, the header's new struct against its ctypes mirror, and the untrained-model constructor of every mode."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seed_chain_matches_the_seeds_sklearn_draws(oracle, monkeypatch):
    """CovRSKBase.train's sequential fits: SVC(kernel=callable, probability=True).fit per window, the callable running CovSample's
    side effect on numpy's global generator (np.random.seed(37), width - 1 draws) before the oracle's kernel"""
    from sklearn.svm import SVC, _libsvm
    from gnomix_amd.train import svc_seed_chain, SVC_SEED_HIGH
    seen = []
    real_fit = _libsvm.fit

    def spy(*a, **k):
        seen.append(int(k["random_seed"]))
        return real_fit(*a, **k)

    monkeypatch.setattr(_libsvm, "fit", spy)

    def covrsk(A_, B_):
        np.random.seed(37)
        np.random.rand(A_.shape[1] - 1)
        return oracle.covrsk(A_, B_).astype(np.float64)

    rng = np.random.RandomState(5)
    widths = [12, 12, 33, 12, 17]
    np.random.seed(3)
    first = np.random.RandomState(3).randint(SVC_SEED_HIGH)
    for width in widths:
        Xw = rng.randint(0, 3, size=(24, width)).astype(np.int8)
        yw = np.repeat(np.arange(3), 8)
        SVC(kernel=covrsk, probability=True).fit(Xw, yw)
    assert seen == [int(s) for s in svc_seed_chain(widths, first)]
    assert len(set(seen)) > 2
    ref = np.random.RandomState(37)
    ref.rand(widths[-1] - 1)
    st, st_ref = np.random.get_state(), ref.get_state()
    assert np.array_equal(st[1], st_ref[1]) and st[2] == st_ref[2]


@pytest.mark.parametrize("seed,l", [(0, 1), (1, 5), (11, 60), (1234567, 401), (2 ** 31 - 2, 2500), (7, 3)])
def test_fold_permutation_matches_newrand(seed, l):
    from sklearn.svm import _newrand
    from gnomix_amd.train import svc_fold_permutation
    _newrand.set_seed_wrap(seed)
    perm = list(range(l))
    for i in range(l):
        j = i + _newrand.bounded_rand_int_wrap(l - i)
        perm[i], perm[j] = perm[j], perm[i]
    assert svc_fold_permutation(seed, l).tolist() == perm


def test_svc_train_info_matches_the_header(tmp_path):
    import ctypes as C
    import subprocess
    from gnomix_amd import _lib
    ct = _lib.SvcTrainInfo
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnomix_hip.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(gnx_svc_train_info));']
    src += [f'  printf("{f} %zu\\n", offsetof(gnx_svc_train_info, {f}));' for f, _ in ct._fields_]
    src += ['  printf("kind %d %d %d\\n", GNX_SVC_KERNEL_SUBSTRINGS, GNX_SVC_KERNEL_POLY, GNX_SVC_KERNEL_ALL_LENGTHS);', '  return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(ct)
    for f, _ in ct._fields_:
        assert int(out[f]) == getattr(ct, f).offset, f
    from gnomix_amd.train import SVC_KERNEL_KINDS
    assert out["kind"].split() == ["0", "1", "2"] and SVC_KERNEL_KINDS == {"CovRSK": 0, "string_kernel": 2}


def _meta(C, A):
    return dict(snp_pos=np.arange(C) * 7 + 100, snp_ref=np.array(["A"] * C), snp_alt=np.array(["G"] * C),
                pop_order=["p%d" % a for a in range(A)])


def test_untrained_model_of_every_mode():
    from gnomix_amd import cli, synth
    from gnomix_amd.convert import cov_sample
    from gnomix_amd.train import untrained_model, cnn_init
    C, M, A, S, ctx, seed = 1237, 50, 4, 75, 12, 9
    meta = _meta(C, A)
    W = C // M
    for mode in ("default", "fast", "large"):
        d = untrained_model(C, M, A, S, ctx, mode, seed=seed, meta=meta)
        via_cli = cli._initial_model(C, M, A, S, ctx, mode, seed, meta)
        assert d.base_kind == via_cli.base_kind == "logistic"
        assert d.lr_coef.shape == (W, A, M + 2 * ctx + C % M) and not d.lr_coef.any() and not d.lr_intercept.any()
        assert np.array_equal(d.snp_pos, meta["snp_pos"]) and d.population_order == meta["pop_order"]
        for k in ("lr_coef", "lr_intercept", "crf_state", "crf_trans", "cnn_weight", "cnn_bias", "tree_off", "left", "cond"):
            a, b = getattr(d, k), getattr(via_cli, k)
            assert (a is None and b is None) or np.array_equal(a, b), (mode, k)
    assert untrained_model(C, M, A, S, ctx, "fast").smooth_kind == "crf"
    large = untrained_model(C, M, A, S, ctx, "large", seed=seed)
    w0, b0 = cnn_init(A, S, seed=seed)
    assert large.smooth_kind == "cnn" and np.array_equal(large.cnn_weight, w0) and np.array_equal(large.cnn_bias, b0)
    default = untrained_model(C, M, A, S, ctx, "default", seed=seed)
    trees = synth.synthetic_trees(1, A, S * A, seed=seed)
    assert default.smooth_kind == "xgb" and all(np.array_equal(getattr(default, k), v) for k, v in trees.items())

    best = untrained_model(C, M, A, S, ctx, "best", seed=seed, meta=meta)
    assert best.base_kind == "covrsk" and best.smooth_kind == "xgb" and len(best.svc) == W
    for w, s in enumerate(best.svc):
        width = best.window_width(w)
        assert s["xfit"].shape == (A, width) and list(s["ms"]) == list(cov_sample(width))
        assert s["dual_coef"].shape == (A - 1, A) and s["n_support"].sum() == len(s["support"]) == A
    desc, keep = best.to_desc()      # a description the library can load
    assert desc.base_kind == 2
    with pytest.raises(ValueError):
        untrained_model(C, M, A, S, ctx, "fastest")


def test_cli_still_refuses_best(tmp_path):
    from gnomix_amd import cli
    cfg = tmp_path / "c.yaml"
    cfg.write_text("model:\n  inference: best\n")
    _, _, err = cli.training_setup(["gnomix.py", "None", str(tmp_path / "o"), "22", "False", "g", "r", "s", str(cfg)])
    assert err and '"best"' in err


def test_window_columns_are_the_reference_padding():
    from gnomix_amd.train import window_columns
    C, M, ctx = 537, 50, 25
    X = np.arange(C)[None]
    Xp = np.concatenate([np.flip(X[:, :ctx], axis=1), X, np.flip(X[:, -ctx:], axis=1)], axis=1)   # base.py:41-44
    W = C // M
    for w in range(W):
        width = M + 2 * ctx + (C % M if w == W - 1 else 0)
        assert np.array_equal(window_columns(C, M, ctx, w), Xp[0, w * M:w * M + width])
