"""Plain-numpy restatement of gnx_ancestry_allele_counts / gnx_ancestry_dosage (include/gnomix_hip.h): np.add.at over win(c).

X (N, C): code 0 = REF, 1 = ALT, anything else = a missing call.  labels (N, W); the window of SNP c is win(c) = min(c // M, W - 1).
A label outside [0, A) counts for no ancestry.  Integer arithmetic throughout: every comparison against this file is np.array_equal."""
import numpy as np


def windows(C, M, W):
    return np.minimum(np.arange(C) // M, W - 1)


def unpack2(P, C):
    """2-bit rows (SNP j = bits 2 (j % 4).. of byte j // 4) -> (N, C) uint8 codes 0..3"""
    P = np.asarray(P, dtype=np.uint8)
    j = np.arange(C)
    return (P[:, j // 4] >> (2 * (j % 4)).astype(np.uint8)) & 3


def pack2(X, ldp=None, fill=0):
    """(N, C) codes 0..3 -> 2-bit rows of ldp >= ceil(C / 4) bytes; the fields past C of the last byte are zero, the bytes past it `fill`"""
    X = np.asarray(X).astype(np.uint8) & 3
    N, C = X.shape
    nb = (C + 3) // 4
    pad = np.zeros((N, nb * 4), np.uint8)
    pad[:, :C] = X
    q = pad.reshape(N, nb, 4)
    out = np.full((N, nb if ldp is None else ldp), fill, np.uint8)
    out[:, :nb] = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    return out


def allele_counts(X, labels, M, A):
    """-> n_obs, n_alt, n_miss, each (A, C) int32"""
    X, lab = np.asarray(X).astype(np.int64), np.asarray(labels).astype(np.int64)
    N, C = X.shape
    W = lab.shape[1]
    assert M >= 1 and W >= 1 and M * W <= C and lab.shape[0] == N
    a = lab[:, windows(C, M, W)]                      # (N, C): the label of every cell
    ok = (a >= 0) & (a < A)
    cols = np.broadcast_to(np.arange(C), (N, C))
    out = []
    for cell in ((X == 0) | (X == 1), X == 1, ~((X == 0) | (X == 1))):
        t = np.zeros((A, C), np.int32)
        m = ok & cell
        np.add.at(t, (a[m], cols[m]), 1)
        out.append(t)
    return tuple(out)


def dosage(X, labels, M, A, ancestry):
    """-> dosage, hapcount, each (N // 2, C) uint8"""
    X, lab = np.asarray(X).astype(np.int64), np.asarray(labels).astype(np.int64)
    N, C = X.shape
    assert N % 2 == 0 and 0 <= ancestry < A
    is_a = lab[:, windows(C, M, lab.shape[1])] == ancestry
    hap = is_a[0::2].astype(np.uint8) + is_a[1::2].astype(np.uint8)
    alt = is_a & (X == 1)
    return alt[0::2].astype(np.uint8) + alt[1::2].astype(np.uint8), hap


def afreq_text(chm, pos, M, W, n_obs, n_alt, populations):
    """the bytes of <prefix>.afreq.tsv"""
    C = len(pos)
    win = windows(C, M, W)
    lines = ["\t".join(["chm", "pos", "window"] + [p + s for p in populations for s in (".n_obs", ".n_alt", ".freq")])]
    for c in range(C):
        cells = [str(chm), str(int(pos[c])), str(int(win[c]))]
        for a in range(len(populations)):
            o, t = int(n_obs[a, c]), int(n_alt[a, c])
            cells += [str(o), str(t), format(t / o, ".6f") if o else "nan"]
        lines.append("\t".join(cells))
    return "\n".join(lines) + "\n"
