"""Ancestry-specific MDS from the pairwise count tables of gnx_ancestry_pair_counts (include/gnomix_hip.h).  Host only,
numpy only: the device produces three exact (n, n) int32 tables per ancestry, everything after that is small.

For one ancestry a, individuals i, j and the SNPs c of a range, with o[i, c] = the haplotypes of i labelled a at c's window that have an
observed call (0..2) and d[i, c] = those of them that are ALT:

  DD[i, j] = sum_c d[i, c] d[j, c]      DO[i, j] = sum_c d[i, c] o[j, c]      OO[i, j] = sum_c o[i, c] o[j, c]

A pair of ancestry-a haplotypes, one from i and one from j (i != j), is compared at c when both have a call; it mismatches when exactly
one is ALT.  Summed over the pairs and SNPs: comp = OO[i, j], mism = DO[i, j] + DO[j, i] - 2 DD[i, j], and the ancestry-specific
allele-sharing distance is mism / comp.
"""
import collections

import numpy as np

_I32 = np.iinfo(np.int32)


class PairCounts(collections.namedtuple("PairCounts", "DD DO OO")):
    """three (n, n) int32 tables of one ancestry.  a + b adds the tables of two SNP ranges or chromosomes of the SAME individuals: the sum
    is taken in int64 and stored back as int32, and refused (OverflowError) only if a stored value leaves int32"""
    __slots__ = ()

    def __add__(self, other):
        if not isinstance(other, PairCounts):
            return NotImplemented
        out = []
        for x, y in zip(self, other):
            x, y = np.asarray(x), np.asarray(y)
            if x.shape != y.shape:
                raise ValueError(f"tables of different individuals: {x.shape} and {y.shape}")
            s = x.astype(np.int64) + y.astype(np.int64)
            if s.size and (s.max() > _I32.max or s.min() < _I32.min):
                raise OverflowError("the sum of the pair counts leaves int32")
            out.append(s.astype(np.int32))
        return PairCounts(*out)

    @property
    def n(self):
        return np.asarray(self.OO).shape[0]

    def mismatches(self):
        """(n, n) int64: DO + DO^T - 2 DD, the mismatching pairs of ancestry haplotypes one from i and one from j.  The diagonal is the
        same expression at i == j (an individual against itself, its two haplotypes counted both ways and each against itself)"""
        DD, DO = np.asarray(self.DD).astype(np.int64), np.asarray(self.DO).astype(np.int64)
        return DO + DO.T - 2 * DD

    def comparisons(self):
        """(n, n) int64: OO, the pairs compared"""
        return np.asarray(self.OO).astype(np.int64)

    def distances(self, min_sites=1):
        """(n, n) float64 allele-sharing distance mism / comp: NaN where comp < min_sites (min_sites >= 1), 0 on the diagonal"""
        min_sites = max(int(min_sites), 1)
        mism, comp = self.mismatches(), self.comparisons()
        out = np.full(comp.shape, np.nan, dtype=np.float64)
        np.divide(mism.astype(np.float64), comp.astype(np.float64), out=out, where=comp >= min_sites)
        np.fill_diagonal(out, 0.0)
        return out


def select(counts, min_sites, min_pair_sites):
    """the individuals an embedding keeps -> sorted int64 indices.  The rule, deterministic:
      1. keep i iff OO[i, i] >= min_sites;
      2. while some kept pair i != j has OO[i, j] < min_pair_sites: drop the kept individual with the most such pairs; ties go to the
         smaller OO[i, i], then to the larger index."""
    OO = np.asarray(counts.OO).astype(np.int64)
    n = OO.shape[0]
    own = np.diagonal(OO).copy() if n else np.zeros(0, np.int64)
    kept = own >= int(min_sites)
    short = OO < int(min_pair_sites)
    np.fill_diagonal(short, False)
    while True:
        idx = np.flatnonzero(kept)
        if idx.size == 0:
            break
        bad = short[np.ix_(idx, idx)].sum(axis=1)
        if bad.max() == 0:
            break
        # most short pairs, then the smaller OO[i, i], then the larger index
        order = sorted(range(idx.size), key=lambda q: (-int(bad[q]), int(own[idx[q]]), -int(idx[q])))
        kept[idx[order[0]]] = False
    return np.flatnonzero(kept).astype(np.int64)


AncestryMDS = collections.namedtuple("AncestryMDS", "coords eigenvalues explained kept n_sites")
AncestryMDS.__doc__ = """what classical_mds returns: coords (n_kept, k) float64, eigenvalues (k,) descending, explained (k,) = each
eigenvalue over the sum of the positive ones, kept (n_kept,) int64 indices into the individuals the distances were over (None: all of
them, in order), n_sites (n_kept,) int64 = OO[i, i] of the kept individuals (None when classical_mds was called on bare distances)"""


def classical_mds(delta, k, kept=None, n_sites=None):
    """classical (Torgerson) MDS of an (n, n) symmetric distance matrix: B = -1/2 J (delta * delta) J with J = I - 11^T / n,
    numpy.linalg.eigh, the k largest eigenvalues, which must be positive (ValueError otherwise, also for a NaN distance or k > n).
    Positive means above n * eps * lambda_1, eigh's own rounding of a zero eigenvalue: the third eigenvalue of points of a plane is not.
    Coordinates are V sqrt(lambda); each component's sign is fixed so that its entry of largest magnitude is positive (ties: the lowest
    index) -> AncestryMDS"""
    delta = np.asarray(delta, dtype=np.float64)
    k = int(k)
    if delta.ndim != 2 or delta.shape[0] != delta.shape[1]:
        raise ValueError(f"delta must be (n, n), got {delta.shape}")
    n = delta.shape[0]
    if k < 1 or k > n:
        raise ValueError(f"need 1 <= k <= n = {n}, got k = {k}")
    if not np.all(np.isfinite(delta)):
        raise ValueError("delta holds a distance that is not finite (a pair with too few compared sites: see select)")
    D2 = delta * delta
    J = np.eye(n) - np.full((n, n), 1.0 / n)
    B = -0.5 * (J @ D2 @ J)
    B = 0.5 * (B + B.T)
    lam, V = np.linalg.eigh(B)
    lam, V = lam[::-1], V[:, ::-1]
    floor = n * np.finfo(np.float64).eps * max(float(lam[0]), 0.0)
    if not np.all(lam[:k] > floor):
        raise ValueError(f"only {int(np.sum(lam > floor))} positive eigenvalues, k = {k} asked for")
    coords = V[:, :k] * np.sqrt(lam[:k])
    for q in range(k):
        if coords[int(np.argmax(np.abs(coords[:, q]))), q] < 0:   # argmax returns the lowest index of a tie
            coords[:, q] = -coords[:, q]
    pos = lam[lam > floor].sum()
    return AncestryMDS(coords, lam[:k].copy(), lam[:k] / pos, kept, n_sites)


def ancestry_mds(counts, k=4, min_sites=1, min_pair_sites=None):
    """select, distances and classical_mds on one ancestry's PairCounts -> AncestryMDS, or None when fewer than k + 1 individuals are
    kept.  min_pair_sites defaults to min_sites"""
    min_sites = max(int(min_sites), 1)
    min_pair = min_sites if min_pair_sites is None else max(int(min_pair_sites), 1)
    kept = select(counts, min_sites, min_pair)
    if kept.size < int(k) + 1:
        return None
    sub = PairCounts(*(np.asarray(t)[np.ix_(kept, kept)] for t in counts))
    delta = sub.distances(min_sites=min_pair)
    own = np.diagonal(np.asarray(sub.OO)).astype(np.int64)
    return classical_mds(delta, k, kept=kept, n_sites=own)
