"""k_sim_admix and its two check kernels on the MI355X at the places the sibling file never reaches: every access width of load16 /
store16 on F, X and the ancestry rows (the device entry on rows of chosen base alignment and stride), every boundary position and
every tie of the label rule, the smallest and the tile-exact geometries, the second trip of both grid-stride loops, and the
"first offence" promise of the validation.  Every comparison is exact; the references are simulate.expand_numpy / window_labels,
which tests/test_simulate_host.py holds to the reference project's files.

The table builders and the alignment bookkeeping are plain functions (no GPU): group_a_cases(), reached(), literal_table(), ..."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_FILL, F_FILL, ANC_FILL, Y_FILL = 77, 2, 99, -7     # F's padding holds a value no founder may hold: reading it would show
GUARD = 48                                           # bytes (Y: elements) behind the last row, >= 32
AOF10 = np.array([0, 0, 1, 1, 2, 2, 255, 255, 1, 0], np.uint8)   # 255 = simulate.NOT_A_FOUNDER


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


# ---- tables -----------------------------------------------------------------------------------------------------------------
def tables(segs):
    off, beg, src = [0], [], []
    for hap in segs:
        for b, s in hap:
            beg.append(b); src.append(s)
        off.append(len(beg))
    return np.array(off, np.int64), np.array(beg, np.int32), np.array(src, np.int32)


def edge_segs(C, r):
    """the segment tables of test_gpu_simulate.py::test_edge_geometries (C >= 33)"""
    return [[(0, 3)],                                             # no crossover
            [(0, 0), (16, 2), (32, 5)],                           # boundaries on 16-byte chunks
            [(0, 1), (5, 4), (17, 0), (C - 1, 9)],                # off chunks, a one-SNP last segment
            [(0, 5)] + [(int(b), int(r.choice([0, 1, 2, 3, 4, 5, 8, 9]))) for b in sorted(r.choice(np.arange(1, C), 12, replace=False))]]


def expected(F, off, beg, src, aof, C, M):
    from gnomix_amd import simulate as S
    Xn, ancn = S.expand_numpy(F, off, beg, src, aof, C)
    return Xn, S.window_labels(ancn, M).astype(np.int32), ancn


# ---- alignment bookkeeping (what the kernel's width tests will see) ---------------------------------------------------------
def cls(a):
    """the branch of load16 / store16 an address takes: 16, 8, 4 or 1 (bytes)"""
    return 16 if a % 16 == 0 else 8 if a % 8 == 0 else 4 if a % 4 == 0 else 1


def reached(off, beg, src, C, ldf, fo, ldx, xo, ao):
    """-> (F, X, anc): the sets of branches k_sim_admix takes on each array.  A 16-column chunk that lies inside one segment is one
    load16 of the founder row; every full chunk is one store16 to X and one to the ancestry row.  Offsets are from a 16-byte
    aligned address."""
    f, x, a = set(), set(), set()
    for n in range(len(off) - 1):
        b = beg[off[n]:off[n + 1]]
        s = src[off[n]:off[n + 1]]
        for c0 in range(0, C - 15, 16):
            x.add(cls(xo + n * ldx + c0))
            a.add(cls(ao + n * C + c0))
            k = int(np.searchsorted(b, c0, side="right")) - 1
            e = int(b[k + 1]) if k + 1 < len(b) else C
            if c0 + 16 <= e:
                f.add(cls(fo + int(s[k]) * ldf + c0))
    return f, x, a


def up16(C):
    return (C + 15) // 16 * 16


# (ld - C, o) of the issue, by name; "R" = the pad that rounds the stride up to a multiple of 16.  The branch a spec is meant to
# hit is the one of row 0, cls(o): rows 0 of F and of X are always moved by whole chunks (edge_segs: source 0 covers [0, 16)).
SPECS = {"p0o0": (0, 0), "p0o1": (0, 1), "p3o0": (3, 0), "p4o4": (4, 4), "p8o8": (8, 8), "p12o4": (12, 4), "Ro0": ("R", 0), "Ro8": ("R", 8)}
COMBOS = [("Ro0", "Ro0"),      # both 16-byte: what the host entry stages
          ("Ro8", "Ro8"),      # both 8-byte and nothing else
          ("p4o4", "p4o4"),    # 4-byte bases
          ("p0o1", "p0o1"),    # byte bases, stride C
          ("p0o1", "Ro0"),     # mixed: F bytes, X 16-aligned
          ("Ro0", "p0o1"),     # mixed: F 16-aligned, X bytes
          ("p0o0", "p0o0"),    # aligned base, stride C: the branch changes row by row
          ("p3o0", "p8o8"),
          ("p8o8", "p3o0"),
          ("p12o4", "Ro8"),
          ("Ro8", "p12o4"),
          ("p4o4", "Ro0"),
          ("Ro0", "Ro8")]


def spec(name, C):
    pad, o = SPECS[name]
    return C + (up16(C) - C if pad == "R" else pad), o


def group_a_cases():
    return [(C, f, x) for C in (100, 333, 4099) for f, x in COMBOS]


def group_a_inputs(C):
    r = np.random.RandomState(C)
    F = r.randint(0, 2, size=(10, C)).astype(np.int8)
    return F, tables(edge_segs(C, r))


# ---- the device entry on rows of chosen alignment ---------------------------------------------------------------------------
class Flat:
    """one flat buffer filled with a sentinel; the payload's row 0 starts `o` elements behind a 16-byte aligned address, rows are
    `ld` apart, and at least GUARD elements follow the last row"""
    def __init__(self, dev, dtype, fill, rows, cols, ld, o):
        import torch
        self.rows, self.cols, self.ld, self.fill = rows, cols, ld, fill
        self.np_dtype = {torch.int8: np.int8, torch.uint8: np.uint8, torch.int32: np.int32}[dtype]
        isz = torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((16 + o + rows * ld + GUARD + 16,), fill, dtype=dtype, device=dev)
        lead = (-self.buf.data_ptr()) % 16
        assert lead % isz == 0
        self.start = lead // isz + o
        assert (self.buf.data_ptr() + (self.start - o) * isz) % 16 == 0          # measured, not assumed
        self.ptr = self.buf.data_ptr() + self.start * isz
        self.offset_bytes = self.ptr % 16
        assert self.offset_bytes == (o * isz) % 16

    def index(self):
        return (self.start + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]).ravel()

    def put(self, a):
        import torch
        host = self.buf.cpu().numpy()
        host[self.index()] = np.asarray(a).ravel()
        self.buf.copy_(torch.from_numpy(host))

    def expect(self, payload=None):
        """the whole buffer as it must read back: the sentinel everywhere but the payload (None: nothing written)"""
        e = np.full(self.buf.numel(), self.fill, self.np_dtype)
        if payload is not None:
            e[self.index()] = np.asarray(payload).ravel()
        return e

    def host(self):
        return self.buf.cpu().numpy()


def dev_call(ctx, F, off, beg, src, aof, A, C, M, ldf=None, fo=0, ldx=None, xo=0, ao=0, want_anc=True):
    """gnx_simulate_admix_dev on torch tensors -> (rc, message, fF, fX, fY, fA), the four arrays as Flat buffers"""
    import torch
    dev = torch.device("cuda", ctx.device)
    nF, N, W = F.shape[0], len(off) - 1, C // M
    ldf, ldx = ldf or C, ldx or C
    fF = Flat(dev, torch.int8, F_FILL, nF, C, ldf, fo)
    fF.put(F)
    fX = Flat(dev, torch.int8, X_FILL, N, C, ldx, xo)
    fY = Flat(dev, torch.int32, Y_FILL, N, W, W, 0)
    fA = Flat(dev, torch.uint8, ANC_FILL, N, C, C, ao)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (off, beg, src, aof)]
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rc = ctx.lib.gnx_simulate_admix_dev(ctx.h, fF.ptr, nF, ldf, C, M, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                        A, N, fX.ptr, ldx, fY.ptr, fA.ptr if want_anc else None)
    torch.cuda.synchronize()
    msg = ctx.lib.gnx_last_error(ctx.h).decode() if rc != 0 else ""
    return rc, msg, fF, fX, fY, fA


def assert_dev_result(res, F, Xn, Yn, ancn, want_anc=True):
    rc, msg, fF, fX, fY, fA = res
    assert rc == 0, msg
    got = fX.host()
    assert np.array_equal(got[fX.index()].reshape(Xn.shape), Xn)                      # X[:, :C]
    assert np.array_equal(got, fX.expect(Xn))                                         # and the sentinel everywhere else
    assert np.array_equal(fY.host(), fY.expect(Yn))
    assert np.array_equal(fA.host(), fA.expect(ancn if want_anc else None))
    assert np.array_equal(fF.host(), fF.expect(F))                                    # the founders are read only


def assert_nothing_written(res):
    _, _, _, fX, fY, fA = res
    assert np.array_equal(fX.host(), fX.expect()) and np.array_equal(fY.host(), fY.expect()) and np.array_equal(fA.host(), fA.expect())


def host_call(ctx, F, ldf, off, beg, src, aof, A, C, M, want_anc=True):
    """gnx_simulate_admix on host arrays; F may be a strided view whose rows are ldf apart -> (rc, X, Y, anc)"""
    N, W = len(off) - 1, C // M
    assert F.strides == (ldf, 1)
    X = np.full((N, C), X_FILL, np.int8)
    Y = np.full((N, W), Y_FILL, np.int32)
    anc = np.full((N, C), ANC_FILL, np.uint8) if want_anc else None
    rc = ctx.lib.gnx_simulate_admix(ctx.h, F.ctypes.data, F.shape[0], ldf, C, M, off.ctypes.data, beg.ctypes.data, src.ctypes.data,
                                    aof.ctypes.data, A, N, X.ctypes.data, C, Y.ctypes.data, anc.ctypes.data if want_anc else None)
    return rc, X, Y, anc


def assert_host_equals(ctx, F, off, beg, src, aof, A, C, M, ldf=None):
    rc, X, Y, anc = host_call(ctx, F, ldf or C, off, beg, src, aof, A, C, M)
    assert rc == 0, ctx.lib.gnx_last_error(ctx.h).decode()
    Xn, Yn, ancn = expected(F, off, beg, src, aof, C, M)
    assert np.array_equal(X, Xn) and np.array_equal(anc, ancn)
    assert np.array_equal(Y, Yn)
    rc, X2, Y2, _ = host_call(ctx, F, ldf or C, off, beg, src, aof, A, C, M, want_anc=False)
    assert rc == 0 and np.array_equal(X2, Xn) and np.array_equal(Y2, Yn)
    return Yn


# ---- A. access widths -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def group_a_reference():
    """C -> (F, (off, beg, src), Xn, Yn, ancn): computed once, shared by every alignment"""
    out = {}
    for C in (100, 333, 4099):
        F, tab = group_a_inputs(C)
        out[C] = (F, tab) + expected(F, *tab, AOF10, C, 7)
    return out


@pytest.mark.parametrize("want_anc", [False, True], ids=["noanc", "anc"])
@pytest.mark.parametrize("C,fspec,xspec", group_a_cases(), ids=["C%d-F%s-X%s" % c for c in group_a_cases()])
def test_access_widths(ctx, group_a_reference, C, fspec, xspec, want_anc):
    F, (off, beg, src), Xn, Yn, ancn = group_a_reference[C]
    (ldf, fo), (ldx, xo) = spec(fspec, C), spec(xspec, C)
    ao = xo                                                       # the ancestry rows (stride C) start at X's offset
    f, x, a = reached(off, beg, src, C, ldf, fo, ldx, xo, ao)
    assert cls(fo) in f, (fspec, sorted(f))                       # the branch this case is for is taken, on F ...
    assert cls(xo) in x, (xspec, sorted(x))                       # ... and on X
    if fspec.startswith("R"):
        assert f == {cls(fo)}                                     # a stride of 16s keeps every row in one branch
    if xspec.startswith("R"):
        assert x == {cls(xo)}
    res = dev_call(ctx, F, off, beg, src, AOF10, 3, C, 7, ldf, fo, ldx, xo, ao, want_anc)
    assert res[2].offset_bytes == fo and res[3].offset_bytes == xo and res[5].offset_bytes == ao
    assert_dev_result(res, F, Xn, Yn, ancn, want_anc)


def test_access_width_cases_cover_every_branch():
    """over the cases of one C, F is loaded and X is stored through each of the four branches, by design (cls of the offset) and
    in fact (reached); the ancestry rows take all four too"""
    for C in (100, 333, 4099):
        _, (off, beg, src) = group_a_inputs(C)
        want_f, want_x, all_a = set(), set(), set()
        for _, fs, xs in [c for c in group_a_cases() if c[0] == C]:
            (ldf, fo), (ldx, xo) = spec(fs, C), spec(xs, C)
            f, x, a = reached(off, beg, src, C, ldf, fo, ldx, xo, xo)
            assert cls(fo) in f and cls(xo) in x
            want_f.add(cls(fo)); want_x.add(cls(xo)); all_a |= a
        assert want_f == want_x == all_a == {16, 8, 4, 1}
    assert ("p0o1", "Ro0") in COMBOS and ("Ro0", "p0o1") in COMBOS          # the two mixed pairs


@pytest.mark.parametrize("fspec", ["Ro0", "Ro8", "p12o4", "p0o1", "p3o0"])
def test_founder_check_at_every_width(ctx, fspec):
    """k_sim_check_founders reads whole chunks through load16: a bad byte at any place of a chunk is found, at the right column,
    whatever branch the row's address takes"""
    C, M = 100, 7
    r = np.random.RandomState(5)
    F = r.randint(0, 2, size=(10, C)).astype(np.int8)
    off, beg, src = tables([[(0, 3)], [(0, 0), (40, 1)]])
    ldf, fo = spec(fspec, C)
    seen = set()
    for row, j in itertools.product((0, 1, 2, 5), (0, 3, 4, 7, 8, 11, 12, 15)):
        col = 16 * (1 + row % 3) + j
        F2 = F.copy()
        F2[row, col] = 2
        seen.add(cls(fo + row * ldf))
        res = dev_call(ctx, F2, off, beg, src, AOF10, 3, C, M, ldf, fo)
        assert res[0] != 0 and "founder haplotype %d (sample %d) holds 2 at SNP %d:" % (row, row // 2, col) in res[1], res[1]
        assert_nothing_written(res)
    assert cls(fo) in seen
    assert_dev_result(dev_call(ctx, F, off, beg, src, AOF10, 3, C, M, ldf, fo), F, *expected(F, off, beg, src, AOF10, C, M))


# ---- B. every boundary position ---------------------------------------------------------------------------------------------
AOF6 = np.array([0, 0, 1, 1, 2, 2], np.uint8)


def one_boundary_tables(C=48):
    """haplotype b - 1: ancestry 1 before b, ancestry 0 from b on, b = 1 .. C - 1"""
    return tables([[(0, 2 + b % 2), (b, (b // 2) % 2)] for b in range(1, C)])


def two_boundary_tables(C=34):
    """ancestries 2, 0, 2 with boundaries b1 < b2, every pair of 0 .. C - 1 (b1 = 0: the first piece is empty): C (C - 1) / 2 rows"""
    segs, pairs = [], []
    for b1, b2 in itertools.combinations(range(C), 2):
        segs.append(([(0, 4 + b1 % 2)] if b1 else []) + [(b1, b2 % 2), (b2, 5 - b1 % 2)])
        pairs.append((b1, b2))
    return tables(segs), pairs


def literal_table():
    """C = 27, M = 6: windows [0,6) [6,12) [12,18) and the last one [18,27), nine SNPs.  Sources 0,1 -> ancestry 0; 2,3 -> 1; 4,5 -> 2.
    -> (tables, the labels written out by hand)"""
    segs = [
        # 0..1 anc 2 | 2..3 anc 1 | 4..5 anc 0: 2/2/2 -> 0.   6..8 anc 2 | 9..11 anc 1: 3/3, no 0 -> 1.
        # 12..13 anc 1 | 14..16 anc 2 | 17 anc 1: 1 + 2 = 3 against 3 -> 1.   18..21 anc 1 | 22 anc 2 | 23..26 anc 0: 4/4 -> 0 (1 met first)
        [(0, 4), (2, 2), (4, 0), (6, 5), (9, 3), (14, 4), (17, 2), (22, 5), (23, 1)],
        # 0..7 anc 2 | 8..9 anc 0 | 10..14 anc 2: window 0 -> 2; window 1 holds 2,2,0,0,2,2: 2 + 2 = 4 beats 2 -> 2 (pieces not added: 0)
        # 12..14 anc 2 | 15..17 anc 1: 3/3 -> 1.   18..19 anc 1 | 20..23 anc 2 | 24..25 anc 1 | 26 anc 0: 4/4/1 -> 1; cut at 24 it were 2
        [(0, 4), (8, 0), (10, 5), (15, 2), (20, 4), (24, 3), (26, 0)],
        # 0..2 anc 0 | 3..8 anc 1 | 9..21 anc 0 | 22..26 anc 2: 3/3 with the smaller code first -> 0, then second -> 0; all 0 -> 0;
        # the last window is won by its tail, 5 x 2 against 4 x 0 -> 2 (cut at 24 it were 0)
        [(0, 1), (3, 3), (9, 0), (22, 4)],
    ]
    Y = [[0, 1, 1, 0],
         [2, 2, 1, 1],
         [0, 0, 0, 2]]
    return tables(segs), np.array(Y, np.int32)


def test_every_single_boundary(ctx):
    C, M, A = 48, 6, 3
    F = np.random.RandomState(48).randint(0, 2, size=(6, C)).astype(np.int8)
    off, beg, src = one_boundary_tables(C)
    Yn = assert_host_equals(ctx, F, off, beg, src, AOF6, A, C, M)
    for b in range(1, C):                                         # the rule itself, next to window_labels
        for w in range(C // M):
            ones = min(max(b - w * M, 0), M)
            assert Yn[b - 1, w] == (1 if ones > M - ones else 0), (b, w)      # the 3/3 cut labels 0, not the first-met 1
    assert [int(Yn[b - 1, b // M]) for b in range(3, C, M)] == [0] * 8         # ... at each window's middle


def test_every_pair_of_boundaries(ctx):
    C, M, A = 34, 8, 3
    F = np.random.RandomState(34).randint(0, 2, size=(6, C)).astype(np.int8)
    (off, beg, src), pairs = two_boundary_tables(C)
    assert len(pairs) == 561 and C // M == 4
    Yn = assert_host_equals(ctx, F, off, beg, src, AOF6, A, C, M)
    for n, (b1, b2) in enumerate(pairs):                          # ancestry 0 on [b1, b2), 2 elsewhere; windows end at 8, 16, 24, 34
        for w, (lo, hi) in enumerate([(0, 8), (8, 16), (16, 24), (24, 34)]):
            zeros = max(min(b2, hi) - max(b1, lo), 0)
            assert Yn[n, w] == (0 if zeros >= (hi - lo) - zeros else 2), (b1, b2, w)


def test_label_rule_written_out(ctx):
    from gnomix_amd import simulate as S
    C, M, A = 27, 6, 3
    (off, beg, src), Y_lit = literal_table()
    F = np.random.RandomState(27).randint(0, 2, size=(6, C)).astype(np.int8)
    Xn, ancn = S.expand_numpy(F, off, beg, src, AOF6, C)
    assert np.array_equal(S.window_labels(ancn, M), Y_lit)
    rc, X, Y, anc = host_call(ctx, F, C, off, beg, src, AOF6, A, C, M)
    assert rc == 0, ctx.lib.gnx_last_error(ctx.h).decode()
    assert np.array_equal(Y, Y_lit)
    assert np.array_equal(X, Xn) and np.array_equal(anc, ancn)
    res = dev_call(ctx, F, off, beg, src, AOF6, A, C, M, ldf=C + 3, fo=1, ldx=C, xo=0, ao=4)
    assert_dev_result(res, F, Xn, Y_lit, ancn)


# ---- C. geometry edges ------------------------------------------------------------------------------------------------------
GEOMETRIES = [(1, 1, ()), (15, 1, ()), (16, 1, ()), (17, 1, (16,)), (15, 15, ()), (4096, 1, (4095, 4096, 4097)), (4097, 1, (4095, 4096, 4097)),
              (8192, 8192, (4096,)), (8197, 4099, (4098, 4099)), (1000, 501, (500, 501))]


def geometry_tables(C, cuts, r):
    cuts = [b for b in cuts if 0 < b < C]                         # a boundary where C allows it
    segs = [[(0, 3)]]
    if cuts:
        segs.append([(0, 0)] + [(b, 1 + i % 5) for i, b in enumerate(cuts)])
    if C > 1:
        segs.append([(0, 4), (C - 1, 9)])                         # a one-SNP last segment
        k = min(12, C - 1)
        segs.append([(0, 5)] + [(int(b), int(r.choice([0, 1, 2, 3, 4, 5, 8, 9]))) for b in sorted(r.choice(np.arange(1, C), k, replace=False))])
    if C > 2:
        segs.append([(0, 2), (1, 4), (2, 0)])                     # two boundaries in the first chunk
    return tables(segs)


@pytest.mark.parametrize("C,M,cuts", GEOMETRIES, ids=["C%d-M%d" % g[:2] for g in GEOMETRIES])
def test_geometry_edges(ctx, C, M, cuts):
    r = np.random.RandomState(C + M)
    F = r.randint(0, 2, size=(10, C)).astype(np.int8)
    off, beg, src = geometry_tables(C, cuts, r)
    Yn = assert_host_equals(ctx, F, off, beg, src, AOF10, 3, C, M)
    assert Yn.shape == (len(off) - 1, C // M)


@pytest.mark.parametrize("C,pad", [(100, 1), (333, 19), (4099, 5)])
def test_host_founders_with_a_row_stride(ctx, C, pad):
    r = np.random.RandomState(C)
    F_big = np.full((10, C + pad), F_FILL, np.int8)               # what lies between the rows is no founder value
    F_big[:, :C] = r.randint(0, 2, size=(10, C))
    F = F_big[:, :C]
    off, beg, src = tables(edge_segs(C, r))
    assert_host_equals(ctx, F, off, beg, src, AOF10, 3, C, 7, ldf=F_big.shape[1])


# ---- D. second trip of the grid-stride loops --------------------------------------------------------------------------------
def many_haplotypes(N=65535 + 5, C=16, nF=6):
    n = np.arange(N)
    off = 2 * np.arange(N + 1, dtype=np.int64)
    beg = np.stack([np.zeros(N, np.int64), 1 + n % 15], axis=1).ravel().astype(np.int32)
    src = np.stack([n % nF, (n + 1) % nF], axis=1).ravel().astype(np.int32)
    return off, beg, src


def test_more_haplotypes_than_grid_rows(ctx):
    from gnomix_amd import simulate as S
    N, C, M, nF, A = 65535 + 5, 16, 8, 6, 3
    aof = np.array([0, 1, 2, 0, 1, 2], np.uint8)
    F = np.random.RandomState(16).randint(0, 2, size=(nF, C)).astype(np.int8)
    off, beg, src = many_haplotypes(N, C, nF)
    # every haplotype has the same shape of table: source n % 6 before column 1 + n % 15, source (n + 1) % 6 from there on
    n = np.arange(N)
    first = np.arange(C)[None, :] < (1 + n % 15)[:, None]
    Xn = np.where(first, F[n % nF], F[(n + 1) % nF])
    ancn = np.where(first, aof[n % nF][:, None], aof[(n + 1) % nF][:, None]).astype(np.uint8)
    Yn = S.window_labels(ancn, M)
    for k in (0, 1, 65534, 65535, 65536, N - 1):                  # the vectorised expectation against expand_numpy, row by row
        x1, a1 = S.expand_numpy(F, np.array([0, 2]), beg[2 * k:2 * k + 2], src[2 * k:2 * k + 2], aof, C)
        assert np.array_equal(x1[0], Xn[k]) and np.array_equal(a1[0], ancn[k])
    rc, X, Y, anc = host_call(ctx, F, C, off, beg, src, aof, A, C, M)
    assert rc == 0, ctx.lib.gnx_last_error(ctx.h).decode()
    assert np.array_equal(X, Xn) and np.array_equal(anc, ancn) and np.array_equal(Y, Yn)


def test_more_founders_than_grid_rows(ctx):
    from gnomix_amd import _lib
    nF, C, M, A = 65535 + 5, 16, 8, 3
    aof = (np.arange(nF) % 3).astype(np.uint8)                    # every row is a founder
    F = np.random.RandomState(17).randint(0, 2, size=(nF, C)).astype(np.int8)
    off, beg, src = tables([[(0, 0), (5, 65539)], [(0, 65536)]])
    F[65537, 5] = 2                                               # no segment uses the row; the check reads every founder
    rc = host_call(ctx, F, C, off, beg, src, aof, A, C, M)[0]
    msg = ctx.lib.gnx_last_error(ctx.h).decode()
    assert rc == _lib.GNX_EINVAL and "founder haplotype 65537 (sample 32768) holds 2 at SNP 5:" in msg, msg
    F[65537, 5] = 0
    assert_host_equals(ctx, F, off, beg, src, aof, A, C, M)


# ---- E. first offence and value checks --------------------------------------------------------------------------------------
def test_first_bad_haplotype_is_named(ctx):
    from gnomix_amd import _lib
    C, M, A = 64, 8, 3
    F = np.zeros((10, C), np.int8)
    good = [(0, 0), (10, 2)]
    segs = [list(good) for _ in range(8)]
    segs[5] = [(1, 0), (9, 1)]                                    # first begin is not 0 (reason 2)
    segs[2] = [(0, 1), (20, 6)]                                   # source 6 is not a founder (reason 5, the largest code)
    segs[7] = [(0, 0), (30, 1), (30, 2)]                          # begins do not increase (reason 3)
    off, beg, src = tables(segs)
    res = dev_call(ctx, F, off, beg, src, AOF10, A, C, M, ldf=C + 3, fo=1, ldx=C + 8, xo=8)
    assert res[0] == _lib.GNX_EINVAL and "segment table of haplotype 2: source is not a founder" in res[1], res[1]
    assert_nothing_written(res)
    rc = host_call(ctx, F, C, off, beg, src, AOF10, A, C, M)[0]
    assert rc == _lib.GNX_EINVAL and "segment table of haplotype 2: source is not a founder" in ctx.lib.gnx_last_error(ctx.h).decode()
    segs[2] = list(good)                                          # with 2 mended the next one is 5, then 7
    res = dev_call(ctx, F, *tables(segs), AOF10, A, C, M)
    assert res[0] == _lib.GNX_EINVAL and "segment table of haplotype 5: first begin is not 0" in res[1], res[1]
    segs[5] = list(good)
    res = dev_call(ctx, F, *tables(segs), AOF10, A, C, M)
    assert res[0] == _lib.GNX_EINVAL and "segment table of haplotype 7: begins do not increase or reach C" in res[1], res[1]
    assert_nothing_written(res)
    segs[7] = list(good)
    tab = tables(segs)
    assert_dev_result(dev_call(ctx, F, *tab, AOF10, A, C, M), F, *expected(F, *tab, AOF10, C, M))


def test_first_bad_founder_byte_is_named(ctx):
    from gnomix_amd import _lib
    C, M, A = 100, 7, 3
    F = np.random.RandomState(3).randint(0, 2, size=(10, C)).astype(np.int8)
    tab = tables([[(0, 3)], [(0, 0), (50, 9)]])
    F2 = F.copy()
    F2[3, 40] = F2[1, 90] = F2[1, 7] = 2
    for kw in ({}, {"ldf": C + 3, "fo": 1}):
        res = dev_call(ctx, F2, *tab, AOF10, A, C, M, **kw)
        assert res[0] == _lib.GNX_EINVAL and "founder haplotype 1 (sample 0) holds 2 at SNP 7:" in res[1], res[1]
        assert_nothing_written(res)
    rc = host_call(ctx, F2, C, *tab, AOF10, A, C, M)[0]
    assert rc == _lib.GNX_EINVAL and "founder haplotype 1 (sample 0) holds 2 at SNP 7:" in ctx.lib.gnx_last_error(ctx.h).decode()
    F2[1, 7] = 1
    res = dev_call(ctx, F2, *tab, AOF10, A, C, M)
    assert res[0] == _lib.GNX_EINVAL and "founder haplotype 1 (sample 0) holds 2 at SNP 90:" in res[1], res[1]
    F2[1, 90] = 0
    res = dev_call(ctx, F2, *tab, AOF10, A, C, M)
    assert res[0] == _lib.GNX_EINVAL and "founder haplotype 3 (sample 1) holds 2 at SNP 40:" in res[1], res[1]
    assert_nothing_written(res)


@pytest.mark.parametrize("value", [-1, -128, 2, 127])
def test_bad_byte_in_the_partial_last_chunk(ctx, value):
    """C = 333: columns 320 .. 332 are the partial chunk, the scalar path of k_sim_check_founders; the value is printed as stored"""
    from gnomix_amd import _lib
    C, M, A = 333, 7, 3
    r = np.random.RandomState(333)
    F = r.randint(0, 2, size=(10, C)).astype(np.int8)
    tab = tables(edge_segs(C, r))
    for col in (C - 1, 320):
        F2 = F.copy()
        F2[4, col] = value
        F2[5, 0] = value                                          # a later row, in a whole chunk: not the first offence
        for kw in ({}, {"ldf": C, "fo": 1}):
            res = dev_call(ctx, F2, *tab, AOF10, A, C, M, **kw)
            assert res[0] == _lib.GNX_EINVAL and "founder haplotype 4 (sample 2) holds %d at SNP %d:" % (value, col) in res[1], res[1]
            assert_nothing_written(res)
    F2 = F.copy()
    F2[2, 17] = value                                             # and in a whole chunk
    res = dev_call(ctx, F2, *tab, AOF10, A, C, M)
    assert res[0] == _lib.GNX_EINVAL and "founder haplotype 2 (sample 1) holds %d at SNP 17:" % value in res[1], res[1]
    assert_nothing_written(res)


def test_rows_that_are_no_founders_are_not_read(ctx):
    C, M, A = 333, 7, 3
    r = np.random.RandomState(334)
    F = r.randint(0, 2, size=(10, C)).astype(np.int8)
    tab = tables(edge_segs(C, r))                                 # sources 0..5, 8, 9: never 6 or 7
    assert AOF10[6] == AOF10[7] == 255 and not np.isin(tab[2], (6, 7)).any()
    ref = expected(F, *tab, AOF10, C, M)
    F2 = F.copy()
    F2[6], F2[7] = 2, -1
    assert_dev_result(dev_call(ctx, F2, *tab, AOF10, A, C, M), F2, *ref)
    assert_dev_result(dev_call(ctx, F2, *tab, AOF10, A, C, M, ldf=C + 4, fo=4, ldx=C, xo=1, ao=1), F2, *ref)
    rc, X, Y, anc = host_call(ctx, F2, C, *tab, AOF10, A, C, M)
    assert rc == 0 and np.array_equal(X, ref[0]) and np.array_equal(Y, ref[1]) and np.array_equal(anc, ref[2])
