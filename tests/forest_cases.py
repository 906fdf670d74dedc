"""Models, inputs, a plain reference and the restated launch arithmetic of the tree bases' edge tests
(tests/test_forest_cases_host.py, tests/test_gpu_forest_edges.py).  Not a test.

The two kernels (csrc/k_base_forest2.hip, the default, and csrc/k_base_forest.hip, GNX_FOREST_IMPL=1) walk a RUN of `wrun` consecutive
windows per block over a power-of-two ring of 16-SNP words and stage only each window's new words; k_base_forest also carries the next
window's words (`pre`) and trees (`tpre`) through registers.  The launchers choose wrun = 1 while tiles * windows fits one round of the
chip, which is every shape a quick test can afford: so the cases here force the run length (GNX_FOREST_WRUN, read once per context) and
state which of those paths they reach.  Every statement is computed again from the launch arithmetic restated below
(`paths`) and asserted by tests/test_forest_cases_host.py, together with the list of paths the whole case list has to reach.

Models are built so that every window splits on its first and last padded SNP, on both neighbours of every 16-SNP word boundary it
touches and on both sides of the seams of the reflect padding (`required_positions`): the shallowest nodes take those positions, so
that a word staged late, a ring slot not refreshed or a field off by one is read by most haplotypes.  SNP values are drawn from
0..3 (the kernels' contract), thresholds from every integer and half-integer the loader's 4-bit masks can tell apart."""
import functools
from dataclasses import dataclass, field

import numpy as np

# ---- geometry ---------------------------------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class Geo:
    name: str
    C: int
    M: int
    ctx: int

    @property
    def W(self):
        return self.C // self.M

    @property
    def rem(self):
        return self.C - self.M * self.W

    @property
    def width(self):
        return self.M + 2 * self.ctx

    @property
    def width_last(self):
        return self.width + self.rem

    def width_of(self, w):
        return self.width_last if w == self.W - 1 else self.width


GEO = {g.name: g for g in (
    Geo("drift", 937, 100, 50),            # M % 16 = 4: window starts visit every fourth offset inside a word, 0 .. 12
    Geo("ringchg", 824, 112, 56),          # main width 224 -> ring 16, last width 264 -> ring 32, M % 16 == 0
    Geo("noov", 64 * 8 + 5, 64, 0),        # ng0 == g1: every word of a window is new
    Geo("share1", 40 * 12 + 7, 40, 0),     # consecutive windows share one word or none
    Geo("deepctx", 48 * 12 + 5, 48, 120),  # ctx > M: several windows touch the reflect padding
    Geo("odd", 37 * 20 + 11, 37, 13),      # odd M, odd ctx: every offset inside a word
    Geo("wide", 1100 * 4 + 3, 1100, 10),   # > 64 new words per window, ring 128
    Geo("edge", 40 * 6 + 7, 40, 12),       # the split-edge cases' small geometry (width 64, last 71)
)}

# ---- the launch arithmetic, restated ----------------------------------------------------------------------------------------------
LDS_MAX = 160 * 1024
T2, H2, NTHR2, TPW2, CG2 = 128, 4, 512, 10, 8     # k_base_forest2.hip:23-33, 104
TP, LB, NPF = 16, 16, 4                           # k_base_forest.hip:55-57
N_CU = 256                                        # compute units of an MI355X


def window_words(g, w):
    """words [g0, g1) of window w in the padded row (k_base_forest2.hip:94-98, k_base_forest.hip:197-201)"""
    s = w * g.M
    return s >> 4, ((s + g.width_of(w) - 1) >> 4) + 1


def ring_words(width):
    """gnx_forest_ring_words (k_base_forest.hip:500-504; the same loop at k_base_forest.hip:436-437)"""
    ring = 16
    while ring < (width + 15 + 15) >> 4:
        ring <<= 1
    return ring


def tree_bytes(rf, D):
    """gnx_model_build.hip:812 (boosted trees: 2^D node words and 2^D leaves) and :904 (random forest: node words only)"""
    return max(16, 4 << D) if rf else 8 << D


def forest2_lds_bytes(A, ring, max_trees, D, rf):
    """gnx_forest2_lds_bytes (k_base_forest2.hip:355-357)"""
    return ring * T2 * 4 + (((max_trees << D) * 4 + 15) & ~15) + A * T2 * (8 if rf else 4)


def forest1_lds_bytes(A, ring, max_trees, tbytes, threads):
    """gnx_forest_lds_bytes (k_base_forest.hip:495-497)"""
    return ring * threads * 4 + ((max_trees * tbytes + 15) & ~15) + A * threads * 4


def runs_forest2(A, max_trees, D, rf, g):
    """does GNX_FOREST_IMPL=0 run k_base_forest2 (gnx_api.hip:519-520)?"""
    return (not rf or A <= 32) and forest2_lds_bytes(A, ring_words(g.width_last), max_trees, D, rf) <= LDS_MAX


def forest2_tpw(D):
    """trees side by side in k_base_forest2 (k_base_forest2.hip:208, :240)"""
    return TPW2 if D <= 4 else TPW2 - 2 if D <= 6 else TPW2 - 4


def forest2_wrun(N, n_windows, lds, forced=0, n_cu=N_CU):
    """launch_range2's run length (k_base_forest2.hip:326-339): cost rounds(r) * (r + 1), then the clamp"""
    per_cu = max(1, min(LDS_MAX // lds, (4 * 4) // (NTHR2 // 64)))
    tiles = (N + T2 - 1) // T2
    wrun = forced
    if wrun <= 0:
        best = None
        for r in range(1, min(24, n_windows) + 1):
            blocks = tiles * ((n_windows + r - 1) // r)
            cost = ((blocks + n_cu * per_cu - 1) // (n_cu * per_cu)) * (r + 1)
            if best is None or cost < best:
                best, wrun = cost, r
    return min(max(1, wrun), n_windows)


def forest1_threads(N, A, ring, max_trees, tbytes, knob=0):
    """launch_range's haplotypes per block (k_base_forest.hip:440-443)"""
    threads = knob // 64 * 64
    if threads < 64 or threads > 256:
        threads = 256
    while threads > 64 and forest1_lds_bytes(A, ring, max_trees, tbytes, threads) > LDS_MAX:
        threads -= 64
    while threads > 64 and threads - 64 >= N:
        threads -= 64
    return threads


def forest1_wrun(N, n_windows, threads, forced=0, n_cu=N_CU):
    """launch_range's run length (k_base_forest.hip:450-461): cost rounds(r) * (r + 2), then the clamp"""
    tiles = (N + threads - 1) // threads
    wrun = forced
    if wrun <= 0:
        best = None
        for r in range(1, min(16, n_windows) + 1):
            blocks = tiles * ((n_windows + r - 1) // r)
            cost = ((blocks + n_cu - 1) // n_cu) * (r + 2)
            if best is None or cost < best:
                best, wrun = cost, r
    return min(max(1, wrun), n_windows)


def forest1_halves(A, rf, threads, knob=0):
    """wave groups per tile (k_base_forest.hip:462-468): two unless GNX_FOREST_H=1, A == 2, or the random forest"""
    return 2 if (not rf and knob != 1 and A > 2 and threads * 2 <= 1024) else 1


def runs(w_first, n_windows, wrun):
    """[wa, wb) of every block row (k_base_forest2.hip:117, k_base_forest.hip:224)"""
    return [(wa, min(w_first + n_windows, wa + wrun)) for wa in range(w_first, w_first + n_windows, wrun)]


def forest1_pre(g, w):
    """is window w + 1 prefetched through registers while w is walked (k_base_forest.hip:276-279)?  -> "true", "size" (more than
    8 * LB / 2 = 64 new words) or "pad" (a new word touches the reflect padding or the row's end)"""
    _, g1 = window_words(g, w)
    ng0, ng1 = window_words(g, w + 1)
    pf_ga, pf_gb = max(ng0, g1), ng1
    if pf_gb - pf_ga > 8 * (LB // 2):
        return "size"
    return "true" if 16 * pf_ga >= g.ctx and 16 * pf_gb <= g.ctx + g.C else "pad"


def forest1_tpre(nt_next, tbytes, rf, threads, halves):
    """do the next window's trees travel through registers (k_base_forest.hip:235, :258-263)?"""
    tq = 2 if rf else 8 // halves
    np_next = nt_next * tbytes // 16
    return 0 < np_next <= tq * threads * halves


def forest2_batches(n, tpw):
    """the two-batch loop of k_base_forest2 on a class of n trees (k_base_forest2.hip:246-264): (trips, nA, nB of the last trip)"""
    trips = nA = nB = 0
    for t in range(0, n, 2 * tpw):
        trips, nA, nB = trips + 1, min(tpw, n - t), max(0, min(tpw, n - (t + tpw)))
    return trips, nA, nB


# ---- cases ------------------------------------------------------------------------------------------------------------------------
XGB_THR = (-0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5)
RF_THR = (-1.0, 0.0, 0.5, float(np.nextafter(1.0, 0.0)), 1.0, 1.5, 2.0, 3.0)


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                   # "x": boosted trees (base_kind "forest"), "r": random forest ("rforest")
    geo: str
    N: int
    A: int
    depth: int
    counts: tuple = (2,)        # per-window rows of per-class tree counts, cycled over the windows; a row shorter than the class count
                                # is cycled over the classes (A == 2 and the random forest have ONE count per window)
    wruns: tuple = None         # None: 1, 2, 3, the smallest length that does not divide the main windows, and one beyond them
    missing: int = 2
    uniform_x: bool = False     # SNP values uniform over 0..3 (else 0 and 1 with a tenth of 2 and of 3 each)
    enumerate_splits: bool = False   # trees walk through every (threshold, default direction) pair in turn
    base_score: float = 0.5
    claims: dict = field(default_factory=dict, hash=False, compare=False)

    @property
    def rf(self):
        return self.kind == "r"

    @property
    def g(self):
        return GEO[self.geo]

    @property
    def groups(self):
        return 1 if (self.rf or self.A == 2) else self.A

    def window_counts(self):
        """(W, groups) trees per window and class"""
        g, out = self.g, []
        for w in range(g.W):
            row = self.counts[w % len(self.counts)]
            row = (row,) if isinstance(row, int) else tuple(row)
            out.append([row[c % len(row)] for c in range(self.groups)])
        return np.array(out, np.int64)

    def run_lengths(self):
        if self.wruns is not None:
            return self.wruns
        nw = self.g.W - 1
        nd = next(r for r in range(2, nw + 2) if nw % r)
        return tuple(sorted({1, 2, 3, nd, nw + 2}))


ALL_COUNTS_D4 = (1, 9, 10, 11, 19, 20, 21, 31)       # TPW2 = 10: 1, TPW - 1 .. TPW + 1, 2 TPW - 1 .. 2 TPW + 1, > 2 TPW (a second trip)

CASES = [
    # ---- geometries: boosted trees of depth 4 and the random forest, every run length ----
    Case("x-drift", "x", "drift", 129, 3, 4,
         claims=dict(ring=(16, 16), wrun_eff={1: 1, 2: 2, 3: 3, 10: 8}, pre={"true"}, tpre={True}, starts=set(range(0, 16, 4)),
                     reuse=True, f1_threads=192)),
    Case("r-drift", "r", "drift", 5, 3, 4, counts=(3,), claims=dict(ring=(16, 16), pre={"true"}, tpre={True})),
    Case("x-ringchg", "x", "ringchg", 257, 3, 4,
         claims=dict(ring=(16, 32), wrun_eff={1: 1, 2: 2, 3: 3, 4: 4, 8: 6}, pre={"true"}, starts={0}, reuse=True, f1_threads=256)),
    Case("r-ringchg", "r", "ringchg", 1, 7, 4, counts=(3,), claims=dict(ring=(16, 32), f1_threads=64)),
    Case("x-noov", "x", "noov", 1, 3, 4, claims=dict(ring=(16, 16), shared={0}, new_words={4}, pre={"true"}, reuse=True)),
    Case("r-noov", "r", "noov", 5, 3, 4, counts=(3,), claims=dict(shared={0}, pre={"true"})),
    Case("x-share1", "x", "share1", 5, 3, 4, claims=dict(ring=(16, 16), shared={0, 1}, pre={"true"})),
    Case("r-share1", "r", "share1", 5, 3, 4, counts=(3,), claims=dict(shared={0, 1})),
    Case("x-deepctx", "x", "deepctx", 129, 3, 4, claims=dict(ring=(32, 32), pre={"true", "pad"}, pad_windows=(9, 2))),
    Case("r-deepctx", "r", "deepctx", 5, 3, 4, counts=(3,), claims=dict(ring=(32, 32), pre={"true", "pad"})),
    Case("x-odd", "x", "odd", 257, 3, 4, claims=dict(ring=(16, 16), starts=set(range(16)), pre={"true"}, reuse=True)),
    Case("r-odd", "r", "odd", 5, 3, 4, counts=(3,), claims=dict(starts=set(range(16)))),
    Case("x-wide", "x", "wide", 5, 3, 4, counts=(4,), claims=dict(ring=(128, 128), pre={"size"}, wrun_eff={1: 1, 2: 2, 3: 3, 5: 3})),
    Case("r-wide", "r", "wide", 1, 3, 4, counts=(12,), claims=dict(ring=(128, 128), pre={"size"})),
    # ---- depths 1 .. 8 at run length 3 (k_base_forest2 walks 10 / 8 / 6 trees side by side; k_base_forest compiles 5 .. 8 apart) ----
    # (shallow trees come in numbers that leave a split node for every required position)
    *[Case("x-depth%d" % D, "x", "drift", 5, 3, D, counts=({1: 13, 2: 5}.get(D, 2),), wruns=(1, 3),
           claims=dict(tpre={D < 8}, f2_tpw=10 if D <= 4 else 8 if D <= 6 else 6, f1_threads=64, f1_halves=2)) for D in range(1, 9)],
    *[Case("r-depth%d" % D, "r", "drift", 5, 3, D, counts=({1: 39, 2: 13, 3: 6}.get(D, 3),), wruns=(1, 3), claims=dict(tpre={D < 8})) for D in range(1, 9)],
    # ---- tree counts around the batch loops (per class, rotating through classes and windows) ----
    Case("x-counts-d4", "x", "noov", 5, 3, 4, counts=((1, 9, 10), (11, 19, 20), (21, 31, 1), (9, 10, 11), (19, 20, 21), (31, 1, 9)),
         wruns=(1, 3), claims=dict(f2_batches={1: (1, 1, 0), 9: (1, 9, 0), 10: (1, 10, 0), 11: (1, 10, 1), 19: (1, 10, 9),
                                               20: (1, 10, 10), 21: (2, 1, 0), 31: (2, 10, 1)}, unequal=True)),
    Case("x-counts-d5", "x", "noov", 5, 3, 5, counts=((7, 9, 17), (9, 17, 7), (17, 7, 9)), wruns=(1, 3),
         claims=dict(f2_tpw=8, f2_batches={7: (1, 7, 0), 9: (1, 8, 1), 17: (2, 1, 0)})),
    Case("x-counts-d7", "x", "noov", 5, 3, 7, counts=((5, 7, 13), (7, 13, 5), (13, 5, 7)), wruns=(1, 3),
         claims=dict(f2_tpw=6, f2_batches={5: (1, 5, 0), 7: (1, 6, 1), 13: (2, 1, 0)}, tpre={False})),
    Case("x-noclass", "x", "share1", 5, 3, 4, counts=((2, 2, 2), (0, 4, 2), (3, 0, 1), (2, 1, 0)), wruns=(1, 3),
         claims=dict(empty_class=True, unequal=True)),
    Case("x-binary", "x", "noov", 5, 2, 4, counts=ALL_COUNTS_D4, wruns=(1, 3), claims=dict(unequal=True, f1_halves=1)),
    Case("x-a5", "x", "share1", 5, 5, 4, counts=((2, 3, 1, 2, 4),), wruns=(1, 3), base_score=0.25, claims=dict(f1_halves=2)),
    Case("r-a9", "r", "share1", 5, 9, 3, counts=(9, 10, 11, 21), wruns=(1, 3), claims=dict(unequal=True)),
    Case("r-a17", "r", "share1", 5, 17, 3, counts=(3, 11), wruns=(1, 3)),
    Case("r-a32", "r", "share1", 5, 32, 3, counts=(3, 11), wruns=(1, 3)),
    # ---- split edges: SNP values uniform over 0..3, every threshold, every missing code, both default directions ----
    *[Case("x-split-d%d-m%d" % (D, m), "x", "edge", 16, 3, D, counts=(6 if D == 1 else 3,), wruns=(1, 3), missing=m, uniform_x=True,
           enumerate_splits=True) for D in (1, 3) for m in range(4)],
    *[Case("r-split-d%d" % D, "r", "edge", 16, 3, D, counts=(18 if D == 1 else 8,), wruns=(1, 3), uniform_x=True, enumerate_splits=True)
      for D in (1, 3)],
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the knob GNX_FOREST_H (k_base_forest: one or two wave groups per tile) on one case with runs
HALVES_CASE = "x-drift"


def _seed(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(case.name)) % (2 ** 31)


def required_positions(g, w):
    """split positions (inside the window's padded slice) that every model places: the first and last SNP, both neighbours of every
    16-SNP word boundary of the padded row inside the window, both sides of the two seams of the reflect padding"""
    s, width = w * g.M, g.width_of(w)
    want = {0, width - 1}
    for b in range((s >> 4) + 1, ((s + width - 1) >> 4) + 1):      # boundary between padded SNPs 16 b - 1 and 16 b
        want.update((16 * b - 1 - s, 16 * b - s))
    if g.ctx:
        for seam in (g.ctx, g.ctx + g.C):                            # padded positions seam - 1 | seam
            for p in (seam - 1 - s, seam - s):
                if 0 <= p < width:
                    want.add(p)
    if w == 0 and g.ctx:
        want.update((0, g.ctx // 2, g.ctx - 1))                      # inside the left flank
    if w == g.W - 1 and g.ctx:
        want.update((width - g.ctx, width - 1 - g.ctx // 2, width - 1))
    assert all(0 <= p < width for p in want)
    return sorted(want)


@functools.lru_cache(maxsize=None)
def build(name):
    """the case's model as a dict of GnxModelData fields (fb_* or rf_*), built once.

    Trees are in xgboost's order (round-major, a round holding one tree of every class that still has one), node arrays in preorder.
    The first tree of a window is complete; others stop early at one node in ten, unless the window then had fewer split nodes than
    required positions.  Split nodes are filled breadth-first over the whole window: the required positions first, then random ones."""
    case = BY_NAME[name]
    g, rng, D, A = case.g, np.random.RandomState(_seed(case)), case.depth, case.A
    thr_set = RF_THR if case.rf else XGB_THR
    combos = [(t, dl) for t in thr_set for dl in ((0,) if case.rf else (0, 1))]
    counts = case.window_counts()
    off, L, R, F, Cd, Dl, V, cls, wt0 = [0], [], [], [], [], [], [], [], [0]
    k_combo = 0
    for w in range(g.W):
        width, need = g.width_of(w), required_positions(g, w)
        order = [c for r in range(int(counts[w].max())) for c in range(case.groups) if r < counts[w][c]]
        assert len(order) >= 1
        for p_early in (0.1, 0.0):
            state = rng.get_state()
            trees = []
            for i in range(len(order)):
                nodes = []       # [left, right, depth] in preorder; left == -1: leaf

                def grow(d):
                    idx = len(nodes)
                    nodes.append([-1, -1, d])
                    if d < D and not (i > 0 and d > 0 and rng.rand() < p_early):
                        nodes[idx][0] = grow(d + 1)
                        nodes[idx][1] = grow(d + 1)
                    return idx

                grow(0)
                trees.append(nodes)
            internal = sorted((nd[2], i, k) for i, nodes in enumerate(trees) for k, nd in enumerate(nodes) if nd[0] != -1)
            if len(internal) >= len(need):
                break
            rng.set_state(state)
        assert len(internal) >= len(need), (name, w, len(internal), len(need))
        feats = list(rng.permutation(need)) + list(rng.randint(width, size=len(internal) - len(need)))
        feat_of = {(i, k): int(f) for (_, i, k), f in zip(internal, feats)}
        for i, nodes in enumerate(trees):
            for k, (l, r, _) in enumerate(nodes):
                L.append(l)
                R.append(r)
                if l == -1:
                    F.append(0)
                    Cd.append(-2.0 if case.rf else np.float32(rng.randn() * 0.2))
                    Dl.append(0)
                    V.append(rng.dirichlet(np.ones(A) * 0.5))
                else:
                    thr, dl = combos[k_combo % len(combos)] if case.enumerate_splits else combos[rng.randint(len(combos))]
                    k_combo += 1
                    F.append(feat_of[(i, k)])
                    Cd.append(thr)
                    Dl.append(dl)
                    V.append(rng.dirichlet(np.ones(A)))
            off.append(len(L))
            cls.append(order[i])
        wt0.append(len(off) - 1)
    i32 = lambda a: np.array(a, np.int32)
    if case.rf:
        return dict(rf_win_tree0=i32(wt0), rf_tree_off=i32(off), rf_left=i32(L), rf_right=i32(R), rf_feat=i32(F),
                    rf_thr=np.array(Cd, np.float64), rf_value=np.array(V, np.float64))
    return dict(fb_win_tree0=i32(wt0), fb_tree_off=i32(off), fb_left=i32(L), fb_right=i32(R), fb_feat=i32(F),
                fb_cond=np.array(Cd, np.float32), fb_default_left=np.array(Dl, np.uint8), fb_tree_class=i32(cls),
                fb_base_score=float(case.base_score), fb_missing=int(case.missing))


def tree_arrays(case):
    """(win_tree0, tree_off, left, right, feat) of the case's model, whichever base it is"""
    m, p = build(case.name), "rf_" if case.rf else "fb_"
    return tuple(m[p + k] for k in ("win_tree0", "tree_off", "left", "right", "feat"))


def model_data(ga, case):
    g = case.g
    return ga.GnxModelData(C=g.C, M=g.M, A=case.A, S=5, context=g.ctx, base_kind="rforest" if case.rf else "forest", **build(case.name))


@functools.lru_cache(maxsize=None)
def inputs(name):
    case = BY_NAME[name]
    rng = np.random.RandomState(_seed(case) ^ 0x5A5A)
    p = [0.25] * 4 if case.uniform_x else [0.4, 0.4, 0.1, 0.1]
    X = rng.choice(4, size=(case.N, case.g.C), p=p).astype(np.int8)
    X.setflags(write=False)
    return X


def oracle_output(O, case):
    m, g, X = build(case.name), case.g, inputs(case.name)
    if case.rf:
        return O.base_rforest({k[3:]: v for k, v in m.items()}, X, g.M, g.ctx, case.A)
    T = O.Trees(m["fb_tree_off"], m["fb_left"], m["fb_right"], m["fb_feat"], m["fb_cond"], m["fb_tree_class"], case.A,
                m["fb_base_score"], default_left=m["fb_default_left"])
    return O.base_forest(T, m["fb_win_tree0"], X, g.M, g.ctx, case.A, missing=case.missing)


# ---- the reference: plain numpy over the ORIGINAL tree arrays ---------------------------------------------------------------------
def padded_rows(X, g):
    """the row as the reference project pads it: the first and the last ctx SNPs flipped and put in front and behind"""
    C, ctx = g.C, g.ctx
    return np.concatenate([X[:, :ctx][:, ::-1], X, X[:, C - ctx:][:, ::-1]], axis=1)


def _leaf_ids(xs, o, left, right, feat, go_left):
    """node (index inside the tree at offset o) where every row of xs ends"""
    rows, nid = np.arange(xs.shape[0]), np.zeros(xs.shape[0], np.int64)
    while True:
        inner = left[o + nid] != -1
        if not inner.any():
            return nid
        gl = go_left(xs[rows, feat[o + nid]], o + nid)
        nid = np.where(inner, np.where(gl, left[o + nid], right[o + nid]), nid)


@functools.lru_cache(maxsize=None)
def reference(name):
    """XGBBase / RFBase.predict_proba restated (see oracle/gnx_oracle.c for the libraries' rules): float32 (N, W, A) for the boosted
    trees — leaves added per class in tree order in float32, base_score added, exp evaluated in float64 and rounded to float32, the
    sum of the exponentials in float64, one float32 division — float64 for the random forest (class rows added in estimator order,
    divided by the tree count)"""
    case = BY_NAME[name]
    m, g, A = build(name), case.g, case.A
    P = padded_rows(inputs(name), g)
    N, f32 = P.shape[0], np.float32
    out = np.empty((N, g.W, A), np.float64 if case.rf else np.float32)
    wt0, off, left, right, feat = tree_arrays(case)
    for w in range(g.W):
        xs = P[:, w * g.M: w * g.M + g.width_of(w)]
        assert xs.shape[1] == g.width_of(w)
        trees = range(wt0[w], wt0[w + 1])
        if case.rf:
            thr, val = m["rf_thr"], m["rf_value"]
            acc = np.zeros((N, A), np.float64)
            for t in trees:
                nid = _leaf_ids(xs, off[t], left, right, feat, lambda v, at: v.astype(f32).astype(np.float64) <= thr[at])   # v <= threshold
                acc += val[off[t] + nid]
            out[:, w] = acc / float(len(trees))
            continue
        cond, dl, cls, miss = m["fb_cond"], m["fb_default_left"], m["fb_tree_class"], case.missing
        go_left = lambda v, at: np.where(v == miss, dl[at] != 0, v.astype(f32) < cond[at])   # missing: default child, else v < threshold
        psum = np.zeros((N, case.groups), f32)
        for t in trees:
            nid = _leaf_ids(xs, off[t], left, right, feat, go_left)
            c = 0 if A == 2 else cls[t]
            psum[:, c] = psum[:, c] + cond[off[t] + nid]
        bs = f32(m["fb_base_score"])
        if A == 2:
            margin = np.log(bs / (f32(1) - bs), dtype=f32) + psum[:, 0]
            p1 = f32(1) / (f32(1) + np.exp(-margin.astype(np.float64)).astype(f32))
            out[:, w, 0], out[:, w, 1] = f32(1) - p1, p1
        else:
            marg = bs + psum
            assert marg.dtype == f32
            e = np.exp((marg - marg.max(axis=1, keepdims=True)).astype(np.float64)).astype(f32)
            wsum = np.zeros(N, np.float64)
            for a in range(A):
                wsum += e[:, a].astype(np.float64)
            out[:, w] = e / wsum.astype(f32)[:, None]
    out.setflags(write=False)
    return out


# ---- which paths a case reaches ---------------------------------------------------------------------------------------------------
def paths(case, halves_knob=0):
    """the case's launch, computed from the restated arithmetic: everything `claims` may name"""
    g, rf, D, A, N = case.g, case.rf, case.depth, case.A, case.N
    counts = case.window_counts()
    nt = counts.sum(axis=1)
    max_trees, tb = int(nt.max()), tree_bytes(rf, D)
    nw = g.W - 1
    ring = (ring_words(g.width), ring_words(g.width_last))
    out = dict(ring=ring, forest2=runs_forest2(A, max_trees, D, rf, g), f2_tpw=forest2_tpw(D),
               starts={(w * g.M) & 15 for w in range(g.W)},
               unequal=len(set(nt.tolist())) > 1, empty_class=bool(((counts == 0).any(axis=1) & (nt >= 1)).any()),
               f2_batches={int(n): forest2_batches(int(n), forest2_tpw(D)) for n in np.unique(counts) if n > 0})
    shared, new_words = set(), set()
    for w in range(nw - 1):
        (_, g1), (ng0, ng1) = window_words(g, w), window_words(g, w + 1)
        shared.add(max(0, g1 - ng0))
        new_words.add(ng1 - max(ng0, g1))
    out.update(shared=shared, new_words=new_words)
    threads = forest1_threads(N, A, ring[0], max_trees, tb)
    halves = forest1_halves(A, rf, threads, halves_knob)
    out.update(f1_threads=threads, f1_halves=halves, f1_tpw=TP // halves,
               f1_threads_last=forest1_threads(N, A, ring[1], max_trees, tb))
    lds2 = forest2_lds_bytes(A, ring[0], max_trees, D, rf)
    out["wrun_eff"], out["wrun_auto"] = {}, (forest2_wrun(N, nw, lds2), forest1_wrun(N, nw, threads))
    pre, tpre, reuse, steps, pad_windows = set(), set(), False, {}, set()
    for wrun in case.run_lengths():
        eff = forest1_wrun(N, nw, threads, forced=wrun)
        assert eff == forest2_wrun(N, nw, lds2, forced=wrun) == min(wrun, nw)
        out["wrun_eff"][wrun] = eff
        steps[wrun] = []
        for wa, wb in runs(0, nw, eff):
            for w in range(wa, wb - 1):
                kind = forest1_pre(g, w)
                tp = forest1_tpre(int(nt[w + 1]), tb, rf, threads, halves)
                steps[wrun].append((w + 1, kind, tp))
                pre.add(kind)
                tpre.add(tp)
                if kind == "pad":
                    pad_windows.add(w + 1)
                # a word of window w + 1 lands in a slot that held another word of this run
                reuse = reuse or window_words(g, w + 1)[1] - window_words(g, wa)[0] > ring[0]
    out.update(pre=pre, tpre=tpre, reuse=reuse, steps=steps,
               pad_windows=(min(pad_windows), len(pad_windows)) if pad_windows else None)
    return out


def close_f32(got, ref):
    """tests/test_gpu_parity.py's _close_f32, the project's bar for the boosted-tree base in float32: walks and margins are bit-exact,
    the last bit of expf may differ (float(exp(double)) against glibc's expf) and knock on through the sum and the division"""
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 2.4e-7
    assert np.count_nonzero(got != ref) <= max(3, got.size // 20)


TOL = 2.4e-7
