"""Global ancestry and tract summaries of window labels restated in plain Python, in the summation order of the kernel.

What gnomix_amd/csrc/summary/k_ancestry_summary.hip must reproduce EXACTLY (its header states the same rules).  Per row of W labels,
weights w (W float64, >= 0) and ancestry a:
  tract_total   = sum of w[k] over the windows with label a          hard = tract_total / den,  den = sum of all w[k]
  soft          = (sum of w[k] * P[k, a]) / den                      (P widened to float64 before the multiply)
  tract_count   = number of maximal runs of label a                  tract_longest = largest sum of w over one such run (0: none)
A label outside [0, A) belongs to no ancestry (and ends a run).

Summation order.  L = ceil(W / 64); lane c of 64 owns the windows [c L, min(W, (c + 1) L)).
  * a sum over windows: every lane adds its chunk's terms left to right onto 0.0 (windows of other classes are skipped; a soft
    term is the rounded product w[k] * P); the lane values are folded in six steps d = 32, 16, 8, 4, 2, 1: t[c] = t[c] + t[c + d]
    for c < d; t[0] is the sum.
  * a run's length: inside a chunk its windows are added left to right, the first term as it is.  A run that goes on past the
    chunk's end leaves its piece in v[c] (else v[c] = 0.0) with f[c] = 0 when the piece began at the chunk's first window as the
    continuation of the lane before, else f[c] = 1.  Inclusive segmented scan, d = 1, 2, 4, 8, 16, 32, all lanes at once from the
    values before the step: if c >= d and f[c] == 0: v[c] = v[c - d] + v[c]; if c >= d: f[c] |= f[c - d].  carry[c] = v[c - 1]
    after the scan (0.0 for lane 0).  A run that began in its lane has the length of its piece, one that came in from the lane before
    carry[c] + piece; it is counted by the lane that holds its last window.
`summary_row` is that text for one row in Python floats (IEEE float64, one rounding per operation); `summary` is the same
arithmetic element by element over all rows and classes at once with numpy (no numpy reduction is used: their order is not
ours); `summary_fraction` is the exact rational form.  Nothing here imports the package under test."""
from fractions import Fraction

import numpy as np

LANES = 64


def chunks(W):
    L = (W + LANES - 1) // LANES
    return [(min(W, c * L), min(W, (c + 1) * L)) for c in range(LANES)]


def fold(t):
    t = list(t)
    d = LANES // 2
    while d > 0:
        for c in range(d):
            t[c] = t[c] + t[c + d]
        d //= 2
    return t[0]


def window_sum(terms, W):
    """terms: a function k -> float or None (skipped)"""
    t = []
    for k0, k1 in chunks(W):
        s = 0.0
        for k in range(k0, k1):
            v = terms(k)
            if v is not None:
                s = s + v
        t.append(s)
    return fold(t)


def denominator(w):
    w = [float(v) for v in w]
    return window_sum(lambda k: w[k], len(w))


def tracts_row(lab, w, a):
    """-> (count, longest) of the runs of label a in one row"""
    W = len(lab)
    cnt, lng = 0, 0.0
    v, f, pending = [0.0] * LANES, [1] * LANES, []   # pending: (lane, piece) of runs whose length needs the lane's carry
    for c, (k0, k1) in enumerate(chunks(W)):
        is_open, from_prev, run = False, False, 0.0
        for k in range(k0, k1):
            if lab[k] == a:
                if not is_open:
                    is_open, run, from_prev = True, w[k], (k == k0 and k0 > 0 and lab[k0 - 1] == a)
                else:
                    run = run + w[k]
            elif is_open:
                if from_prev:
                    pending.append((c, run))
                else:
                    cnt, lng = cnt + 1, max(lng, run)
                is_open = False
        if is_open:
            if k1 < W and lab[k1] == a:     # goes on in the next lane
                v[c], f[c] = run, (0 if from_prev else 1)
            elif from_prev:
                pending.append((c, run))
            else:
                cnt, lng = cnt + 1, max(lng, run)
    d = 1
    while d < LANES:
        v0, f0 = list(v), list(f)
        for c in range(d, LANES):
            if not f0[c]:
                v[c] = v0[c - d] + v0[c]
            f[c] = f0[c] | f0[c - d]
        d *= 2
    for c, piece in pending:
        carry = v[c - 1] if c > 0 else 0.0
        cnt, lng = cnt + 1, max(lng, carry + piece)
    return cnt, lng


def summary_row(lab, w, A, P=None):
    """one row: lab (W,) ints, w (W,) floats, P None or (W, A) -> dict of five lists of A values (soft None without P)"""
    lab = [int(v) for v in lab]
    w = [float(v) for v in w]
    W = len(lab)
    den = denominator(w)
    out = {"hard": [], "soft": None if P is None else [], "tract_count": [], "tract_total": [], "tract_longest": []}
    for a in range(A):
        tot = window_sum(lambda k: w[k] if lab[k] == a else None, W)
        cnt, lng = tracts_row(lab, w, a)
        out["hard"].append(tot / den)
        out["tract_total"].append(tot)
        out["tract_count"].append(cnt)
        out["tract_longest"].append(lng)
        if P is not None:
            out["soft"].append(window_sum(lambda k: w[k] * float(P[k][a]), W) / den)
    return out


def _fold_np(t):
    t = t.copy()
    d = LANES // 2
    while d > 0:
        t[..., :d] = t[..., :d] + t[..., d:2 * d]
        d //= 2
    return t[..., 0]


def summary(labels, w, A, P=None):
    """all rows: labels (N, W) ints, w (W,), P None or (N, W, A) float32 / float64 -> dict of (N, A) arrays: hard, soft (None
    without P), tract_total, tract_longest float64 and tract_count int32.  The arithmetic of summary_row, element by element."""
    labels = np.asarray(labels)
    w = np.asarray(w, dtype=np.float64)
    N, W = labels.shape
    L = (W + LANES - 1) // LANES
    Wp = LANES * L
    cls = np.arange(A).reshape(1, A, 1)
    lab = np.full((N, Wp + 1), -1, np.int64)      # one more column: "the window after" of the last chunk
    lab[:, :W] = np.where((labels >= 0) & (labels < A), labels, -1)
    wp = np.zeros(Wp, np.float64)
    wp[:W] = w
    valid = (np.arange(Wp) < W).reshape(LANES, L)
    wl = wp.reshape(LANES, L)
    is_a = lab[:, None, :] == cls                                   # (N, A, Wp + 1)
    m = is_a[:, :, :Wp].reshape(N, A, LANES, L)
    prev = np.concatenate([np.zeros((N, A, 1), bool), is_a[:, :, :Wp - 1]], axis=2).reshape(N, A, LANES, L)[..., 0]
    nxt = is_a[:, :, 1:Wp + 1].reshape(N, A, LANES, L)[..., L - 1]  # the class of the window after the chunk's last
    den = 0.0 + _fold_np(_chunk_sum(np.broadcast_to(wl, (1, 1, LANES, L)), np.broadcast_to(valid, (1, 1, LANES, L))))[0, 0]
    tot = _fold_np(_chunk_sum(np.broadcast_to(wl, m.shape), m))
    soft = None
    if P is not None:
        Pp = np.zeros((N, Wp, A), np.float64)
        Pp[:, :W] = np.asarray(P).astype(np.float64)
        terms = wl[None, None] * Pp.transpose(0, 2, 1).reshape(N, A, LANES, L)
        soft = _fold_np(_chunk_sum(terms, np.broadcast_to(valid, terms.shape))) / den
    shp = (N, A, LANES)
    is_open, from_prev, head_closed = np.zeros(shp, bool), np.zeros(shp, bool), np.zeros(shp, bool)
    run, head, lng = np.zeros(shp), np.zeros(shp), np.zeros(shp)
    cnt = np.zeros(shp, np.int64)
    for j in range(L):
        mj = m[..., j]
        begins = mj & ~is_open
        run = np.where(begins, wl[:, j], np.where(mj, run + wl[:, j], run))
        from_prev = np.where(begins, prev if j == 0 else False, from_prev)
        ends = ~mj & is_open
        head = np.where(ends & from_prev, run, head)
        head_closed |= ends & from_prev
        done = ends & ~from_prev
        cnt += done
        lng = np.where(done, np.maximum(lng, run), lng)
        is_open = mj
    # (a padded window matches no class, so the last real lane's chunk ends its run like any other window would)
    goes_on = is_open & nxt
    v = np.where(goes_on, run, 0.0)
    f = ~(goes_on & from_prev)
    d = 1
    while d < LANES:
        v0, f0 = v.copy(), f.copy()
        v[..., d:] = np.where(f0[..., d:], v0[..., d:], v0[..., :-d] + v0[..., d:])
        f[..., d:] = f0[..., d:] | f0[..., :-d]
        d *= 2
    carry = np.concatenate([np.zeros((N, A, 1)), v[..., :-1]], axis=2)
    cnt += head_closed
    lng = np.where(head_closed, np.maximum(lng, carry + head), lng)
    last = is_open & ~goes_on
    cnt += last
    lng = np.where(last, np.maximum(lng, np.where(from_prev, carry + run, run)), lng)
    return {"hard": tot / den, "soft": soft, "tract_count": cnt.sum(axis=2).astype(np.int32), "tract_total": tot,
            "tract_longest": lng.max(axis=2)}


def _chunk_sum(terms, take):
    """(…, 64, L) terms, `take` of the same shape -> (…, 64): the lanes' left-to-right sums onto 0.0 of the terms taken"""
    s = np.zeros(terms.shape[:-1], np.float64)
    for j in range(terms.shape[-1]):
        s = np.where(take[..., j], s + terms[..., j], s)
    return s


def summary_fraction(lab, w, A, P=None):
    """one row, exactly: the same five lists as summary_row with Fractions (tract_count ints)"""
    lab = [int(v) for v in lab]
    wf = [Fraction(float(v)) for v in w]
    W = len(lab)
    den = sum(wf, Fraction(0))
    out = {"hard": [], "soft": None if P is None else [], "tract_count": [], "tract_total": [], "tract_longest": []}
    for a in range(A):
        runs, start = [], None
        for k in range(W + 1):
            if k < W and lab[k] == a:
                start = k if start is None else start
            elif start is not None:
                runs.append(sum(wf[start:k], Fraction(0)))
                start = None
        tot = sum(runs, Fraction(0))
        out["hard"].append(tot / den)
        out["tract_total"].append(tot)
        out["tract_count"].append(len(runs))
        out["tract_longest"].append(max(runs) if runs else Fraction(0))
        if P is not None:
            out["soft"].append(sum((wf[k] * Fraction(float(P[k][a])) for k in range(W)), Fraction(0)) / den)
    return out
