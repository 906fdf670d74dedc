"""Inputs the admixture-mapping tests share (tests/test_admixmap_host.py on the CPU, tests/test_gpu_admixmap.py on the GPU).  Not a test.

case(n_ind, T, W, A, K) -> labels (N, W) int32, Y (n_ind, T), Z (n_ind, K), use (n_ind,) uint8.  Degenerate material in every case (a
window index is taken modulo W, an individual's index is folded into the few there are):
    use = 0 on individual 1; a NaN in Y on individual 2; +inf and -inf in Y on individual 3 (2 when n_ind = 3); a NaN in Z on individual 4
      (1 when n_ind <= 4);
    window 1: two labels out of range (A and -1) on individual 0 and one (2^20) on the last individual: their count comes back;
    window 2: ancestry A - 1 is absent;
    window 3: a single ancestry (0) is present: nothing is kept, q < 1;
    window 4: every individual but K + 1 usable ones carries a label out of range: df < 1;
    window 5: ancestry 1 is carried by exactly one haplotype: below MIN_HAP = 2.
GRID, for the device blocks: a thinned cross product of n_ind in {3, 8, 9} (under one group of 4, exactly two, two plus one), T in {1, 15,
16, 17, 33}, W in {1, 16, 19} (one window, exactly one 16-window tile, a tile plus three) and (A, K) in {(2, 1), (3, 3), (7, 3), (12, 5),
(13, 4)} (the last two give K + A = 17: a second tile of rows with one live row); every value of every axis appears.  With 9 individuals
of whom 4 are taken out, these cases have no degrees of freedom: they pin the blocks, the integer fields, status and the NaN patterns.
FIT, for the results: N_FIT = 61 individuals (15 groups of 4 plus one), W = 19, T = 3, every (A, K) of the grid; Z and Y are multiples of
2^-6 so that the Fraction arithmetic of admixmap_exact stays short (the grid's cases are not rounded, and FIT_RAW is one
more FIT-sized case, 63 individuals, that is not).  As in real calls a haplotype keeps a home ancestry
over 70 % of its windows, and EVERY trait carries a signal of the number of home-0 haplotypes (SIGNAL), so that every window has a real
effect: the project's bound is relative to max_a |beta| of the cell and says nothing useful about a cell whose every coefficient is zero
but for chance.  Trait 0 carries a signal of ancestry 0 at window 7 on top.  The grid also has T = 64 (four trait tiles per workgroup) and
(A, K) = (32, 16) (three row tiles, ten tile pairs of the Gram matrix).
Asserted here, on the CPU, with the restatement alone (check_fit_case, called by the tests before they compare anything):
    at most one quarter of the (window, trait) cells of a FIT case are outside the float comparison, whether degenerate on purpose or
    with kappa > assoc_cases.KAPPA_MAX;
and for the permutation case (PERM): no perm_max value lies within 1e-9 relative of an observed statistic, so p_adj is compared exactly."""
import numpy as np

import admixmap_exact as XE
import assoc_cases as AC

MIN_HAP = 2
AK = [(2, 1), (3, 3), (7, 3), (12, 5), (13, 4)]
GRID = [(3, 1, 1, 2, 1), (8, 15, 16, 3, 3), (9, 16, 19, 7, 3), (3, 17, 19, 12, 5), (8, 33, 1, 13, 4), (9, 33, 16, 12, 5), (9, 17, 19, 13, 4),
        (8, 16, 19, 2, 1), (3, 15, 16, 7, 3), (9, 1, 19, 3, 3), (9, 64, 19, 7, 3), (9, 2, 19, 32, 16)]
N_FIT, W_FIT, T_FIT = 61, 19, 3
FIT = [(N_FIT, T_FIT, W_FIT, A, K) for A, K in AK]
FIT_RAW = (63, T_FIT, W_FIT, 3, 3)          # as a FIT case, Z and Y with all their 53 bits: the device's sums round
SIGNAL = (1.0, -0.8, 0.6)
PERM = (N_FIT, 2, W_FIT, 3, 3)
N_PERM, SEED = 7, 20240
_cache, _fits = {}, {}


def case(n_ind, T, W, A, K):
    key = (n_ind, T, W, A, K)
    if key not in _cache:
        rng = np.random.RandomState(7000 + 1000 * n_ind + 37 * T + 11 * W + 5 * A + K)
        N = 2 * n_ind
        lab = rng.randint(0, A, size=(N, W)).astype(np.int32)
        Z = np.concatenate([np.ones((n_ind, 1)), rng.normal(size=(n_ind, K - 1))], 1)
        Y = rng.normal(size=(n_ind, T))
        if n_ind == N_FIT:                  # (the grid's cases keep all 53 bits: their sums round)
            Z, Y = np.round(Z * 64) / 64, np.round(Y * 64) / 64
        if n_ind >= N_FIT:                  # tracts and a signal in every trait (the docstring says why)
            home = rng.randint(0, A, size=N)
            lab = np.where(rng.uniform(size=(N, W)) < 0.7, home[:, None], lab).astype(np.int32)
            Y += np.array([SIGNAL[t % 3] for t in range(T)]) * ((home[0::2] == 0) * 1.0 + (home[1::2] == 0))[:, None]
        Y[:, 0] += 0.5 * ((lab[0::2, 7 % W] == 0) * 1.0 + (lab[1::2, 7 % W] == 0))
        use = np.ones(n_ind, np.uint8)
        use[1] = 0
        Y[2, T // 2] = np.nan
        i_inf = 3 if n_ind > 3 else 2
        Y[i_inf, 0] = np.inf
        Y[i_inf, T - 1] = -np.inf
        i_z = 4 if n_ind > 4 else 1
        Z[i_z, K - 1] = np.nan
        w = lambda k: k % W
        lab[:, w(2)] = np.where(lab[:, w(2)] == A - 1, 0, lab[:, w(2)])
        lab[:, w(3)] = 0
        usable = [i for i in range(n_ind) if i not in (1, 2, i_inf, i_z)]
        for i in range(n_ind):
            if i not in usable[:K + 1]:
                lab[2 * i + (i & 1), w(4)] = A
        lab[:, w(5)] = np.where(lab[:, w(5)] == 1, 0, lab[:, w(5)])
        lab[2 * usable[0], w(5)] = 1
        lab[0, w(1)], lab[1, w(1)], lab[N - 1, w(1)] = A, -1, 1 << 20
        _cache[key] = (lab, Y, Z, use)
    return _cache[key]


def fit_of(key, min_hap=MIN_HAP):
    """the restatement's results of case(*key), computed once"""
    if (key, min_hap) not in _fits:
        lab, Y, Z, use = case(*key)
        _fits[(key, min_hap)] = XE.fit(lab, key[3], Y, Z, use, min_hap)
    return _fits[(key, min_hap)]


def compared(want):
    """the windows inside the float comparison: fitted (status 0) and kappa <= KAPPA_MAX"""
    return (want["status"] == 0) & (want["kappa"] <= AC.KAPPA_MAX)


def check_fit_case(key):
    want = fit_of(key)
    ok = compared(want)
    T = key[1]
    outside = (~ok).sum() * T + np.isnan(want["F"][ok]).sum()
    assert outside <= 0.25 * len(ok) * T, (key, int(outside), len(ok) * T)
    return want


_perm = {}


def perm_reference():
    """-> observed fit, perm_max_t, perm_max_F of the permutation case, with the closeness condition asserted"""
    if not _perm:
        lab, Y, Z, use = case(*PERM)
        want = fit_of(PERM)
        mt, mF = XE.permutation_maxima(lab, PERM[3], Y, Z, use, MIN_HAP, N_PERM, SEED)
        for obs, mx in ((np.abs(want["t"]), mt), (want["F"], mF)):
            o = obs[~np.isnan(obs)]
            for t in range(PERM[1]):
                rel = np.abs(mx[t][None, :] - obs[..., t][~np.isnan(obs[..., t])][:, None]) / mx[t][None, :]
                assert rel.size == 0 or rel.min() > 1e-9, "a permutation maximum ties with an observed statistic"
            assert o.size
        _perm["r"] = (want, mt, mF)
    return _perm["r"]
