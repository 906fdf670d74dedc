"""Inputs of the ancestry-score tests (tests/test_score_host.py, tests/test_gpu_score.py).  Not a test.

The weights make the summation order visible: every entry is normal x 2^u with u an integer drawn from [-20, 20], so the terms of one
sum span 40 binary orders of magnitude and almost every add rounds; another order of the same terms gives other bits."""
import numpy as np


def weights(rng, C, A, S):
    return rng.normal(size=(C, A, S)) * np.exp2(rng.randint(-20, 21, size=(C, A, S)).astype(np.float64))


def case(N, C, M, W, A, S, seed=0):
    """-> X (N, C) int8 with codes 0, 1, 2 and -1 (the last two = missing), labels (N, W) int32 in [0, A) that change every other
    window, weights (C, A, S), effect (C,) uint8 with all three values (where C allows)"""
    rng = np.random.RandomState(1000 * seed + N + 7 * C + 31 * A + 101 * S + M)
    X = rng.choice([0, 1, 2, -1], size=(N, C), p=[0.5, 0.4, 0.06, 0.04]).astype(np.int8)
    lab = np.repeat(rng.randint(0, A, size=(N, W // 2 + 1)), 2, axis=1)[:, :W].astype(np.int32)
    w = weights(rng, C, A, S)
    effect = rng.choice([1, 0, 255], size=C, p=[0.6, 0.25, 0.15]).astype(np.uint8)
    if C == 1:
        effect[0] = 1
    return X, np.ascontiguousarray(lab), w, effect


def codes(X):
    """int8 bytes -> 2-bit codes: -1 becomes 3, every other missing byte 2"""
    return np.where((X == 0) | (X == 1), X, np.where(X == -1, 3, 2)).astype(np.uint8)
