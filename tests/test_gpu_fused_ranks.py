"""The rank image between the logistic pass and the tree smoother (gnx_infer_dev: k_base_logistic_i8 ranks every probability in its
flush, k_smooth_xgb_h32 copies its strip from the image) against the float route (GNX_FUSE_RANKS=0: float32 B in between, ranked by
the smoother while it stages).

Both routes rank the same float32 with the same function and table, so probabilities and labels must be BIT-identical.  The knob is
read at context creation: one context per route.  GNX_SMOOTH_IMPL=h32 (read at model load) forces the h32 kernel as
tests/test_gpu_smooth_h32.py does; small batches otherwise take the rank kernel and the fused route declines.

Shapes: M = 10 keeps C small; the loader refuses W < 2 S.  W = 150 at S = 75 is two window blocks (one per reflection), W = 230 adds an
interior block and a ragged last one, W = 100 (96 + 4) runs at S = 49.  N = 1, 31, 33 and 257: a lone partial block of 32 haplotypes, a
block and one haplotype, and a crossing of the base pass's tile (64 rows up to N = 512: 257 is five tiles and nine blocks, the last of
one haplotype).  A = 8 fills the base pass's column tile exactly (2 window slots x 8 classes = 16), A = 12 needs two tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


@pytest.fixture(scope="module")
def ctxs(ga):
    """(context with the fused route, context with GNX_FUSE_RANKS=0)"""
    from gnomix_amd import _lib
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("GNX_FUSE_RANKS", raising=False)
        on = _lib.Context(0)
        mp.setenv("GNX_FUSE_RANKS", "0")
        off = _lib.Context(0)
    yield on, off
    on.close()
    off.close()


def _data(W, A, S, rounds=3, depth=4, seed=0):
    from gnomix_amd import synth
    return synth.synthetic_model(C=W * 10 + 3, M=10, A=A, S=S, context=5, n_rounds=rounds, depth=depth, seed=seed + W + A)


def _x(N, C, ldx=None, seed=0):
    """int8 haplotypes in HBM, rows ldx bytes apart (ldx > C: the bytes between rows are 3s, which no weight may meet)"""
    import torch
    from gnomix_amd import synth
    X = synth.synthetic_X(N, C, seed=seed + N, miss=0.03)
    if ldx is None:
        return torch.from_numpy(X).cuda()
    buf = torch.full((N, ldx), 3, dtype=torch.int8, device="cuda")
    buf[:, :C] = torch.from_numpy(X).cuda()
    return buf[:, :C]


def _infer(ga, monkeypatch, ctx, data, Xt, calibrate=False):
    import torch
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "h32")
    m = ga.DeviceModel(data, ctx=ctx)
    try:
        if calibrate:
            m.set_calibrate(True)
        p, lab = m.infer_device(Xt)
        torch.cuda.synchronize()
        return p.cpu(), lab.cpu()
    finally:
        m.close()


def _same(a, b):
    import torch
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _live(ctx):
    """device workspaces the context holds"""
    out = np.full(64, -1, np.int32)
    n = ctx.lib.gnx_debug_ws_devices(ctx.h, out.ctypes.data, out.size)
    assert n >= 0
    return n


CASES = ([(7, 75, W, N) for W in (150, 230) for N in (1, 31, 33, 257)] + [(7, 49, 100, N) for N in (1, 31, 33, 257)] +
         [(2, 75, 150, 33), (8, 75, 150, 257)])


@pytest.mark.parametrize("A,S,W,N", CASES)
def test_fused_equals_unfused(ga, ctxs, monkeypatch, A, S, W, N):
    data = _data(W, A, S)
    Xt = _x(N, data.C)
    fused = _infer(ga, monkeypatch, ctxs[0], data, Xt)
    plain = _infer(ga, monkeypatch, ctxs[1], data, Xt)
    assert _same(fused, plain)
    assert bool((fused[0].sum(-1) - 1).abs().max() < 1e-5)      # probabilities, not an empty buffer


def test_fused_equals_unfused_odd_row_stride(ga, ctxs, monkeypatch):
    """rows an odd number of bytes apart, more than C"""
    A, S, W, N = 7, 75, 230, 33
    data = _data(W, A, S)
    Xt = _x(N, data.C, ldx=(data.C + 37) | 1)
    assert Xt.stride(0) % 2 == 1 and Xt.stride(0) > data.C
    fused = _infer(ga, monkeypatch, ctxs[0], data, Xt)
    assert _same(fused, _infer(ga, monkeypatch, ctxs[1], data, Xt))
    assert _same(fused, _infer(ga, monkeypatch, ctxs[0], data, Xt.contiguous()))


def test_fused_route_is_taken_and_keeps_b_unwritten(ga, monkeypatch):
    """a fresh context that only ever runs the fused route holds a rank image and no float B: one workspace fewer than the float
    route would need beside it (the declines below lean on the same count)"""
    from gnomix_amd import _lib
    data = _data(150, 7, 75)
    Xt = _x(33, data.C)
    monkeypatch.delenv("GNX_FUSE_RANKS", raising=False)
    on = _lib.Context(0)
    monkeypatch.setenv("GNX_FUSE_RANKS", "0")
    off = _lib.Context(0)
    try:
        a = _infer(ga, monkeypatch, on, data, Xt)
        b = _infer(ga, monkeypatch, off, data, Xt)
        assert _same(a, b)
        n_on = _live(on)
        assert n_on == _live(off)                     # the image in place of B
        other = _data(150, 7, 75, depth=3)            # the rank kernel's shape: float B in the context's scratch as well
        _infer(ga, monkeypatch, on, other, _x(33, other.C))
        assert _live(on) == n_on + 1
        _infer(ga, monkeypatch, off, other, _x(33, other.C))
        assert _live(off) == n_on
    finally:
        on.close()
        off.close()


def test_thresholds_that_are_base_probabilities(ga, ctxs, monkeypatch):
    """every split threshold is a float32 probability the base pass produces on this very input: ranks sit exactly on thresholds"""
    import torch
    A, S, W, N = 7, 75, 150, 33
    data = _data(W, A, S, rounds=4)
    Xt = _x(N, data.C)
    m = ga.DeviceModel(data, ctx=ctxs[1])
    B = m.base_predict_device(Xt).cpu().numpy()
    m.close()
    split = data.left != -1
    rng = np.random.RandomState(5)
    cond = data.cond.copy()
    cond[split] = rng.choice(B.reshape(-1), size=int(split.sum()))
    data.cond = cond.astype(np.float32)
    assert np.isin(data.cond[split], B).all()
    fused = _infer(ga, monkeypatch, ctxs[0], data, Xt)
    plain = _infer(ga, monkeypatch, ctxs[1], data, Xt)
    assert _same(fused, plain)
    # and against the smoother alone on that B (the float route in two calls)
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "h32")
    m = ga.DeviceModel(data, ctx=ctxs[1])
    p, lab = m.smooth_predict_device(torch.from_numpy(B).cuda())
    torch.cuda.synchronize()
    assert _same(fused, (p.cpu(), lab.cpu()))
    m.close()


def test_calibrator_after_the_fused_route(ga, ctxs, monkeypatch):
    """the calibrator reads the smoother's probabilities, whichever route produced them"""
    A, S, W, N = 7, 75, 150, 33
    data = _data(W, A, S)
    rng = np.random.RandomState(2)
    xs = [np.sort(rng.random_sample(5)).astype(np.float64) for _ in range(A)]
    data.calib_off = np.cumsum([0] + [len(x) for x in xs]).astype(np.int32)
    data.calib_x = np.concatenate(xs)
    data.calib_y = np.concatenate([np.sort(rng.random_sample(len(x))) for x in xs])
    Xt = _x(N, data.C)
    fused = _infer(ga, monkeypatch, ctxs[0], data, Xt, calibrate=True)
    plain = _infer(ga, monkeypatch, ctxs[1], data, Xt, calibrate=True)
    raw = _infer(ga, monkeypatch, ctxs[0], data, Xt)
    assert _same(fused, plain)
    assert not _same(fused, raw)


@pytest.mark.parametrize("A,S,W,N", [(7, 75, 230, 33), (7, 75, 150, 257), (8, 75, 150, 31), (7, 49, 100, 1)])
def test_rank_image(ga, ctxs, monkeypatch, A, S, W, N):
    """the base launch with the image and B both requested: every written position is the host's rank of the float32 beside it,
    r(p) = #{k : U[k] <= p} over the ensemble's sorted distinct finite thresholds (tests/test_rank_table_host.py's brute force)"""
    import torch
    data = _data(W, A, S, rounds=4)
    Xt = _x(N, data.C)
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "h32")
    m = ga.DeviceModel(data, ctx=ctxs[0])
    nb = (N + 31) // 32
    SENT = 0x5A5A
    rk = torch.full((nb, W, A, 32), SENT, dtype=torch.int16, device="cuda")
    B = torch.empty((N, W, A), dtype=torch.float32, device="cuda")
    m._bind_torch_stream()
    fn = m.lib.gnx_base_predict_ranks_dev
    m.ctx.check(fn(m.h, Xt.data_ptr(), N, Xt.stride(0), B.data_ptr(), rk.data_ptr()))
    rk_only = torch.full_like(rk, SENT)
    m.ctx.check(fn(m.h, Xt.data_ptr(), N, Xt.stride(0), None, rk_only.data_ptr()))   # the image alone: what gnx_infer_dev asks for
    torch.cuda.synchronize()
    B_ref = m.base_predict_device(Xt).cpu().numpy()
    m.close()
    Bh = B.cpu().numpy()
    assert np.array_equal(Bh.view(np.int32), B_ref.view(np.int32))
    U = data.cond[data.left != -1]
    U = np.unique(U[np.isfinite(U)].astype(np.float32))
    want = np.searchsorted(U, Bh, side="right").astype(np.uint16)
    want[np.isnan(Bh)] = 0xFFFF
    assert len(np.unique(want)) > 10
    img = rk.cpu().numpy().view(np.uint16)
    got = img.transpose(0, 3, 1, 2).reshape(nb * 32, W, A)      # [n / 32][w][a][n % 32] -> [n][w][a]
    assert np.array_equal(got[:N], want)
    assert torch.equal(rk[:, :, :, :], rk_only)
    if N % 32:                                                   # rows of haplotypes >= N are not compared; here: not written either
        assert (got[N:] == SENT).all()


def test_rank_image_refused_where_the_base_pass_writes_none(ga, ctxs, monkeypatch):
    import torch
    from gnomix_amd import _lib
    data = _data(150, 12, 3)                                     # two column tiles: k_base_logistic_i8_dl
    Xt = _x(5, data.C)
    m = ga.DeviceModel(data, ctx=ctxs[0])
    rk = torch.zeros((1, 150, 12, 32), dtype=torch.int16, device="cuda")
    m._bind_torch_stream()
    with pytest.raises(ga.GnxError) as e:
        m.ctx.check(m.lib.gnx_base_predict_ranks_dev(m.h, Xt.data_ptr(), 5, Xt.stride(0), None, rk.data_ptr()))
    assert e.value.code == _lib.GNX_EUNSUPPORTED
    m.close()


DECLINES = [
    ("two_column_tiles", dict(W=100, A=12, S=21), False),        # A = 12: 24 class columns, k_base_logistic_i8_dl
    ("depth_3", dict(W=150, A=7, S=75, depth=3), False),         # k_smooth_xgb_h32 walks depth-4 trees only: the rank kernel runs
    ("packed_input", dict(W=150, A=7, S=75), True),              # 2-bit rows
]


@pytest.mark.parametrize("name,shape,packed", DECLINES, ids=[d[0] for d in DECLINES])
def test_dispatch_declines(ga, monkeypatch, name, shape, packed):
    """shapes the fused route does not serve take the float route: the same outputs as with the knob off, and no rank image — the
    context gains that workspace only when a call the fused route serves follows"""
    import torch
    from gnomix_amd import _lib
    N = 33
    data = _data(**shape)
    Xt = _x(N, data.C)
    monkeypatch.delenv("GNX_FUSE_RANKS", raising=False)
    on = _lib.Context(0)
    monkeypatch.setenv("GNX_FUSE_RANKS", "0")
    off = _lib.Context(0)
    monkeypatch.setenv("GNX_SMOOTH_IMPL", "h32")

    def run(ctx):
        m = ga.DeviceModel(data, ctx=ctx)
        p, lab = m.infer_packed_device(m.pack_device(Xt)) if packed else m.infer_device(Xt)
        torch.cuda.synchronize()
        m.close()
        return p.cpu(), lab.cpu()
    try:
        a, b = run(on), run(off)
        assert _same(a, b)
        if packed:                                               # the packed route equals the int8 one, fused
            assert _same(a, _infer(ga, monkeypatch, off, data, Xt))
        n_on = _live(on)
        assert n_on == _live(off)
        served = _data(150, 7, 75)
        _infer(ga, monkeypatch, on, served, _x(N, served.C))
        assert _live(on) == n_on + 1                             # the image, for the first time
        _infer(ga, monkeypatch, off, served, _x(N, served.C))
        assert _live(off) == n_on
    finally:
        on.close()
        off.close()
