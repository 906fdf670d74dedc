"""Ancestry-specific linkage disequilibrium from the banded count tables of gnx_ancestry_ld_counts (include/gnomix_hip.h),
and the clumping of association results that polygenic scores are built from.  Host only, numpy only: the tables are the device's
(DeviceModel.ancestry_ld_counts[_device / _gt2], HipGnomix.ancestry_ld / ancestry_clump); the .clumped.tsv writer is
postprocess.write_clumps."""
import collections

import numpy as np

GNX_LD_MAX_BAND = 4096     # include/gnomix_hip.h


class LDCounts(collections.namedtuple("LDCounts", "n11 n1o no1 noo c0 band")):
    """the four (rows, band) int32 tables of one ancestry over the SNPs c0 .. c0 + rows - 1: entry [c - c0, k] speaks of the pair
    (c, c + k) and sums over the haplotypes that carry the ancestry at both SNPs with both calls observed (noo of them): n1o the ALT
    calls at c, no1 those at c + k, n11 the haplotypes ALT at both.  Rows of two adjacent ranges concatenate with +."""
    __slots__ = ()

    @property
    def c1(self):
        return int(self.c0) + int(np.asarray(self.noo).shape[0])

    def __add__(self, other):
        if not isinstance(other, LDCounts):
            return NotImplemented
        if int(other.c0) != self.c1 or int(other.band) != int(self.band):
            raise ValueError(f"LDCounts: rows {other.c0} .. do not follow rows .. {self.c1 - 1}, or the bands differ ({self.band}, {other.band})")
        return LDCounts(*(np.concatenate([np.asarray(a), np.asarray(b)], axis=0) for a, b in zip(self[:4], other[:4])), self.c0, self.band)

    def r(self):
        """the correlation of the two SNPs' alleles over the jointly observed, jointly labelled haplotypes, float64 of the tables'
        shape: with exact int64 values num = noo n11 - n1o no1, v = n1o (noo - n1o), v' = no1 (noo - no1),
        r = float64(num) / sqrt(float64(v) float64(v')); NaN where v or v' is 0 (a SNP that is monomorphic among those haplotypes, or no
        such haplotype: no LD)"""
        n11, n1o, no1, noo = (np.asarray(t).astype(np.int64) for t in self[:4])
        num = noo * n11 - n1o * no1
        v, v2 = n1o * (noo - n1o), no1 * (noo - no1)
        out = np.full(num.shape, np.nan, dtype=np.float64)
        ok = (v != 0) & (v2 != 0)
        out[ok] = num[ok].astype(np.float64) / np.sqrt(v[ok].astype(np.float64) * v2[ok].astype(np.float64))
        return out

    def r2(self):
        """r squared, NaN where r is"""
        r = self.r()
        return r * r

    def pair(self, c, c2):
        """(n11, n1o, no1, noo) of the pair (c, c2) as ints, n1o the ALT calls at c and no1 those at c2, looked up from either side:
        below the diagonal the row is c2's and n1o, no1 change places"""
        c, c2 = int(c), int(c2)
        lo, k = (c, c2 - c) if c2 >= c else (c2, c - c2)
        if not (int(self.c0) <= lo < self.c1) or k >= int(self.band):
            raise IndexError(f"the pair ({c}, {c2}) is not in the rows {self.c0} .. {self.c1 - 1} with band {self.band}")
        n11, n1o, no1, noo = (int(np.asarray(t)[lo - int(self.c0), k]) for t in self[:4])
        return (n11, n1o, no1, noo) if c2 >= c else (n11, no1, n1o, noo)


def band_for(pos, kb):
    """the smallest band such that every SNP within kb kilobases after a SNP is inside it (pos ascending): the largest number of SNPs
    c' >= c with pos[c'] - pos[c] <= 1000 kb, the SNP itself included.  ValueError naming the number if that exceeds GNX_LD_MAX_BAND."""
    pos = np.asarray(pos).astype(np.int64)
    if pos.size == 0:
        return 1
    reach = np.searchsorted(pos, pos + int(round(float(kb) * 1000)), side="right") - np.arange(pos.size)
    band = max(1, int(reach.max()))
    if band > GNX_LD_MAX_BAND:
        raise ValueError(f"{kb} kb hold up to {band} SNPs, more than a band of GNX_LD_MAX_BAND = {GNX_LD_MAX_BAND}")
    return band


def clump(p, pos, counts_for, p1=1e-4, p2=1e-2, r2=0.5, kb=250):
    """clumping of one ancestry's association p-values -> index_of (C,) int64: an index SNP holds its own position in the SNP order, a
    clumped SNP its index's, -1 means neither.  counts_for(c0, c1) returns the LDCounts of the rows [c0, c1) (with a band that reaches
    kb kilobases: band_for), so only the ranges around index SNPs are ever computed.  The order, this project's definition:
      1. candidates are the SNPs with finite p <= p1, taken in ascending p, ties to the lower index;
      2. a candidate that is still unassigned becomes an index SNP;
      3. every unassigned SNP joins it that lies within 1000 kb bp on either side, has finite p <= p2 and whose r^2 with the index is
         >= r2, where a NaN r^2 never joins.
    pos ascending.  ValueError if the tables' band does not reach a SNP within kb."""
    p = np.asarray(p, dtype=np.float64)
    pos = np.asarray(pos).astype(np.int64)
    C = p.shape[0]
    if pos.shape != (C,):
        raise ValueError(f"p and pos must have one entry per SNP, got {p.shape} and {pos.shape}")
    index_of = np.full(C, -1, np.int64)
    fin = np.isfinite(p)
    cand = np.nonzero(fin & (p <= p1))[0]
    cand = cand[np.lexsort((cand, p[cand]))]
    may_join = fin & (p <= p2)
    span = int(round(float(kb) * 1000))
    for c in cand:
        c = int(c)
        if index_of[c] != -1:
            continue
        index_of[c] = c
        lo = int(np.searchsorted(pos, pos[c] - span, side="left"))
        hi = int(np.searchsorted(pos, pos[c] + span, side="right"))
        who = np.nonzero(may_join[lo:hi] & (index_of[lo:hi] == -1))[0] + lo
        if who.size == 0:
            continue
        counts = counts_for(lo, c + 1)
        band = int(counts.band)
        if c - lo >= band or hi - 1 - c >= band:
            raise ValueError(f"SNP {c}: {kb} kb reach the SNPs {lo} .. {hi - 1}, the tables' band is {band} (band_for gives the band to ask for)")
        rr = counts.r2()
        below, above = who[who < c], who[who > c]
        val = np.concatenate([rr[below - lo, c - below], rr[c - lo, above - c]])      # (a NaN compares False)
        index_of[np.concatenate([below, above])[val >= r2]] = c
    return index_of


class BlockCache:
    """counts_for over whole blocks of `block` rows, each fetched once and kept: for a source whose every call is dear (the file path's
    form builds the packed matrix again).  fetch(c0, c1) -> LDCounts; C = the number of SNPs"""

    def __init__(self, fetch, C, block=4096):
        self.fetch, self.C, self.block, self.have = fetch, int(C), int(block), {}

    def __call__(self, c0, c1):
        out = None
        for b in range(int(c0) // self.block, (int(c1) - 1) // self.block + 1):
            if b not in self.have:
                self.have[b] = self.fetch(b * self.block, min((b + 1) * self.block, self.C))
            out = self.have[b] if out is None else out + self.have[b]
        s0 = int(c0) - int(out.c0)
        return LDCounts(*(np.asarray(t)[s0:s0 + int(c1) - int(c0)] for t in out[:4]), int(c0), out.band)
