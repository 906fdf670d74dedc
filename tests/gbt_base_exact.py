"""An exact host restatement of the boosted-tree base trainer (gnx_train_gbt_base, forest/k_train_gbt_base.hip).  Plain numpy / Python
integers: no GPU, no oracle, no code shared with the library.

The algorithm, per window (features = the columns of the window's reflect-padded slice, codes 0 / 1 / 2 = missing):
  * A >= 3: multi:softprob, A trees per round, tree k adds to class k, float32 margins from base_score;
    A == 2: binary:logistic, one tree per round on y == 1, the margin from float32(log(bs / (1 - bs)));
  * the softmax / sigmoid through `det_exp` (float64, every operation rounded on its own: no fused multiply-add), gradient pairs
    rounded to multiples of 2^-30 (round half to even), every sum a Python int;
  * per node and feature three candidates, in this order: 1 = {0} | {1, m} (cond 0.5, missing right), 2 = {0, m} | {1} (cond 0.5,
    missing left), 3 = {0, 1} | {m} (cond 1.5, missing right); valid when both children's H reach min_child_weight and the float64
    gain exceeds max(gamma, 1e-6); the best gain wins, ties to the lowest feature, then the lowest candidate;
  * level by level to max_depth; a leaf holds float32(eta * (-G / (H + lambda))).
`train` returns the forest in the fb_* layout (window-major, round-major, nodes in heap order) and the mean log loss per round."""
import math

import numpy as np

FIX = 1073741824.0   # 2^30
F32 = np.float32


def window_columns(C, M, ctx, w):
    """columns of X behind window w's padded slice (Base.pad's reflection, base.py:41-44; the last window takes the remainder)"""
    W = C // M
    width = M + 2 * ctx + (C - M * W if w == W - 1 else 0)
    cols = []
    for j in range(width):
        p = w * M + j
        cols.append(ctx - 1 - p if p < ctx else (p - ctx if p < ctx + C else C - 1 - (p - ctx - C)))
    return cols


def det_exp(x):
    """exp(x) for x <= 0: range reduction by ln 2 in two parts, a degree-13 Horner polynomial, ldexp; every step one float64 operation"""
    x = float(x)
    if not (x > -745.0):
        return 0.0
    kf = float(np.rint(x * 1.4426950408889634))
    r = (x - kf * 6.93147180369123816490e-01) - kf * 1.90821492927058770002e-10
    p = 1.0 / 6227020800.0
    for c in (1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0,
              1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        t = p * r          # (two statements: two roundings)
        p = t + c
    return math.ldexp(p, int(kf))


def _fix(v):
    return int(round(v * FIX))     # Python's round: half to even, as llrint in the default rounding mode


def gradients(F, y, A):
    """F (N, K) float32 margins, y (N,) labels -> gi, hi: K lists of N Python ints; row losses (N floats)"""
    N, K = F.shape
    gi = [[0] * N for _ in range(K)]
    hi = [[0] * N for _ in range(K)]
    loss = []
    for n in range(N):
        yi = int(y[n])
        if K == 1:
            z = float(F[n, 0])
            e = det_exp(-z if z >= 0.0 else z)
            p = 1.0 / (1.0 + e) if z >= 0.0 else e / (1.0 + e)
            g = p - (1.0 if yi == 1 else 0.0)
            h = p * (1.0 - p)
            h = 1e-16 if h < 1e-16 else h
            gi[0][n], hi[0][n] = _fix(g), _fix(h)
            py = p if yi == 1 else 1.0 - p
        else:
            m = F[n, 0]
            for c in range(1, A):
                m = F[n, c] if F[n, c] > m else m
            e = [det_exp(float(F32(F[n, c]) - F32(m))) for c in range(A)]
            s = 0.0
            for c in range(A):
                s = s + e[c]
            py = 0.0
            for c in range(A):
                p = e[c] / s
                g = p - (1.0 if yi == c else 0.0)
                h = 2.0 * p * (1.0 - p)
                h = 1e-16 if h < 1e-16 else h
                gi[c][n], hi[c][n] = _fix(g), _fix(h)
                if yi == c:
                    py = p
        loss.append(-math.log(py if py > 1e-300 else 1e-300))
    return gi, hi, loss


def gain_of(GL, HL, Gn, Hn, lam):
    gl, hl = GL / FIX, HL / FIX
    gr, hr = (Gn - GL) / FIX, (Hn - HL) / FIX
    Gd, Hd = Gn / FIX, Hn / FIX
    return (gl * gl / (hl + lam) + gr * gr / (hr + lam)) - Gd * Gd / (Hd + lam)


def left_sums(c, Gn, Hn, G1, H1, Gm, Hm):
    if c == 1:
        return Gn - G1 - Gm, Hn - H1 - Hm
    if c == 2:
        return Gn - G1, Hn - H1
    return Gn - Gm, Hn - Hm


def goes_left(c, x):
    return (x != 1 and x != 2) if c == 1 else ((x != 1) if c == 2 else (x != 2))


def grow_tree(Xw, g, h, max_depth, eta, lam, gamma, mcw, trace=None):
    """one regression tree on the window's codes Xw (N, width) -> (nodes in heap order {heap index: tuple}, leaf heap index per row).
    A split is ("split", feature, candidate), a leaf ("leaf", float32 value)."""
    N, width = Xw.shape
    is1 = [np.flatnonzero(Xw[:, j] == 1) for j in range(width)]
    is2 = [np.flatnonzero(Xw[:, j] == 2) for j in range(width)]
    g_at, h_at = np.array(g, np.int64), np.array(h, np.int64)   # (only to GATHER a node's values: every sum is Python's, over ints)
    pos = np.zeros(N, np.int64)
    nodes = {}
    sums = {0: (sum(g), sum(h))}
    open_ = [0]
    floor_ = gamma if gamma > 1e-6 else 1e-6
    for d in range(max_depth + 1):
        nxt = []
        for node in open_:
            Gn, Hn = sums[node]
            best = None
            if d < max_depth:
                inn = pos == node
                for j in range(width):
                    r1, r2 = is1[j][inn[is1[j]]], is2[j][inn[is2[j]]]
                    G1, H1 = sum(g_at[r1].tolist()), sum(h_at[r1].tolist())
                    Gm, Hm = sum(g_at[r2].tolist()), sum(h_at[r2].tolist())
                    for c in (1, 2, 3):
                        GL, HL = left_sums(c, Gn, Hn, G1, H1, Gm, Hm)
                        if HL / FIX < mcw or (Hn - HL) / FIX < mcw:
                            continue
                        gain = gain_of(GL, HL, Gn, Hn, lam)
                        if not gain > floor_:
                            continue
                        if best is None or gain > best[0]:     # features and candidates ascend: the first of equals stays
                            best = (gain, j, c, GL, HL)
            if best is None:
                value = F32(eta * (-(Gn / FIX) / (Hn / FIX + lam)))
                nodes[node] = ("leaf", value)
                if trace is not None:
                    trace.append(dict(node=node, rows=np.flatnonzero(pos == node).tolist(), G=Gn, H=Hn, split=None, value=value))
                continue
            _, j, c, GL, HL = best
            nodes[node] = ("split", j, c)
            if trace is not None:
                trace.append(dict(node=node, rows=np.flatnonzero(pos == node).tolist(), G=Gn, H=Hn, split=(j, c), gain=best[0]))
            l, r = 2 * node + 1, 2 * node + 2
            sums[l], sums[r] = (GL, HL), (Gn - GL, Hn - HL)
            for n in np.flatnonzero(pos == node).tolist():
                pos[n] = l if goes_left(c, int(Xw[n, j])) else r
            nxt += [l, r]
        open_ = nxt
    return nodes, pos.tolist()


def train_window(Xw, yw, A, n_rounds=20, max_depth=4, eta=0.1, lam=1.0, gamma=0.0, mcw=1.0, base_score=0.5, trace=None):
    """-> (trees: list of (nodes, class) in round-major order, row losses per round: (n_rounds + 1) lists, final margins (N, K))"""
    N = Xw.shape[0]
    K = 1 if A == 2 else A
    m0 = F32(math.log(base_score / (1.0 - base_score))) if K == 1 else F32(base_score)
    F = np.full((N, K), m0, F32)
    trees, losses = [], []
    for r in range(n_rounds):
        gi, hi, loss = gradients(F, yw, A)
        losses.append(loss)
        for k in range(K):
            tr = None if trace is None else []
            nodes, pos = grow_tree(Xw, gi[k], hi[k], max_depth, eta, lam, gamma, mcw, trace=tr)
            if trace is not None:
                trace.append(dict(round=r, k=k, g=gi[k], h=hi[k], nodes=tr))
            trees.append((nodes, k))
            for n in range(N):
                F[n, k] = F32(F[n, k]) + F32(nodes[pos[n]][1])
    losses.append(gradients(F, yw, A)[2])
    return trees, losses, F


def train(X, y, M, ctx, A, **kw):
    """X (N, C) codes, y (N, W) labels -> (dict of fb_* arrays, losses (n_rounds + 1,) float64)"""
    X = np.asarray(X)
    N, C = X.shape
    W = C // M
    wt0, off, L, R, Fe, Cd, Dl, cls = [0], [0], [], [], [], [], [], []
    per_round = None
    for w in range(W):
        Xw = X[:, window_columns(C, M, ctx, w)]
        trees, losses, _ = train_window(Xw, np.asarray(y)[:, w], A, **kw)
        per_round = losses if per_round is None else [a + b for a, b in zip(per_round, losses)]
        for nodes, k in trees:
            order = sorted(nodes)
            idx = {h: i for i, h in enumerate(order)}
            for hnode in order:
                nd = nodes[hnode]
                if nd[0] == "split":
                    L.append(idx[2 * hnode + 1]); R.append(idx[2 * hnode + 2]); Fe.append(nd[1])
                    Cd.append(F32(1.5 if nd[2] == 3 else 0.5)); Dl.append(1 if nd[2] == 2 else 0)
                else:
                    L.append(-1); R.append(-1); Fe.append(0); Cd.append(F32(nd[1])); Dl.append(0)
            off.append(len(L))
            cls.append(k)
        wt0.append(len(off) - 1)
    fb = dict(fb_win_tree0=np.array(wt0, np.int32), fb_tree_off=np.array(off, np.int32), fb_left=np.array(L, np.int32),
              fb_right=np.array(R, np.int32), fb_feat=np.array(Fe, np.int32), fb_cond=np.array(Cd, np.float32),
              fb_default_left=np.array(Dl, np.uint8), fb_tree_class=np.array(cls, np.int32))
    return fb, np.array([math.fsum(l) / (N * W) for l in per_round], np.float64)
