"""gnx_confusion_dev / gnx_confusion (csrc/score/k_confusion.hip) on the MI355X against np.add.at: the A x A counts of true labels
against int32 predictions or against probability rows whose first-maximum argmax the kernel takes itself, at every size where the
pass changes shape (nothing, one element, a partial wave, many workgroups with a grid-stride tail), at the smallest and the largest
A, with ties and NaN, with labels out of range, beyond the largest A, and with the early flush forced."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("labels", "f64", "f32")
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _case(n, A):
    """y, probabilities on a grid of quarters (so most rows carry exact ties), their np.argmax, and the np.add.at counts of both
    prediction forms: drawn once per (n, A) and shared, unchanged, by every test that uses the size"""
    if (n, A) not in _cache:
        rng = np.random.RandomState(1000 * A + n % 997)
        y = rng.randint(0, A, size=n).astype(np.int32)
        P = rng.randint(0, 3, size=(n, A)).astype(np.float64) * 0.25
        lab = rng.randint(0, A, size=n).astype(np.int32)
        ref_lab, ref_arg = np.zeros((A, A), np.int64), np.zeros((A, A), np.int64)
        np.add.at(ref_lab, (y, lab), 1)
        np.add.at(ref_arg, (y, np.argmax(P, axis=-1) if n else np.zeros(0, np.int64)), 1)
        _cache[(n, A)] = (y, P, lab, ref_lab, ref_arg)
    return _cache[(n, A)]


def _pred(kind, P, lab):
    return {"labels": lab, "f64": P, "f32": P.astype(np.float32)}[kind]


def _dev_counts(ctx, y, pred, A, **kw):
    import torch
    from gnomix_amd import resident
    return resident.confusion_counts(ctx, torch.from_numpy(y).cuda(), torch.from_numpy(np.ascontiguousarray(pred)).cuda(), A, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, 65, 1_000_003])
def test_counts_equal_add_at_at_every_size(ctx, n, kind):
    y, P, lab, ref_lab, ref_arg = _case(n, 3)
    got = _dev_counts(ctx, y, _pred(kind, P, lab), 3)
    assert got.dtype == np.int64 and got.shape == (3, 3)
    assert np.array_equal(got, ref_lab if kind == "labels" else ref_arg)
    assert int(got.sum()) == n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A", [1, 2, 32])
def test_counts_equal_add_at_for_the_smallest_and_the_largest_A(ctx, A, kind):
    y, P, lab, ref_lab, ref_arg = _case(4099, A)
    got = _dev_counts(ctx, y, _pred(kind, P, lab), A)
    assert np.array_equal(got, ref_lab if kind == "labels" else ref_arg)


def test_ties_go_to_the_first_maximum(ctx):
    # quarters in {0, 0.25, 0.5} over 3 classes: about two rows in three hold their maximum more than once
    y, P, _, _, ref_arg = _case(65, 3)
    tied = np.sum(P == P.max(axis=1, keepdims=True), axis=1) > 1
    assert tied.sum() >= 20
    for kind in ("f64", "f32"):
        assert np.array_equal(_dev_counts(ctx, y, _pred(kind, P, None), 3), ref_arg)


def test_nan_counts_as_a_maximum_and_the_first_nan_wins(ctx):
    """np.argmax treats NaN as larger than every number and returns the first NaN of a row (its loop takes v when !(v <= best) and
    stops at a NaN); Base.evaluate's np.argmax(B, -1) therefore does, and so does the kernel."""
    nan = np.nan
    P = np.array([[0.1, nan, 0.9], [nan, nan, 0.2], [0.3, 0.2, nan], [0.9, 0.1, nan], [0.2, 0.7, 0.1]], np.float32)
    assert np.argmax(P, axis=-1).tolist() == [1, 0, 2, 2, 1]      # numpy's behaviour, stated
    y = np.array([0, 1, 2, 0, 1], np.int32)
    ref = np.zeros((3, 3), np.int64)
    np.add.at(ref, (y, [1, 0, 2, 2, 1]), 1)
    assert np.array_equal(_dev_counts(ctx, y, P, 3), ref)
    assert np.array_equal(_dev_counts(ctx, y, P.astype(np.float64), 3), ref)


def _raw_dev(ctx, y, pred, kind, A, flush_every=0):
    import torch
    ty, tp = torch.from_numpy(y).cuda(), torch.from_numpy(np.ascontiguousarray(pred)).cuda()
    cm = torch.full((max(A * A, 1),), -7, dtype=torch.int64, device="cuda")
    nfl = C.c_int64(-1)
    torch.cuda.synchronize()
    rc = ctx.lib.gnx_confusion_dev(ctx.h, ty.data_ptr(), tp.data_ptr(), kind, len(y), A, cm.data_ptr(), flush_every, C.byref(nfl))
    ctx.synchronize()
    return rc, cm.cpu().numpy(), nfl.value


def test_labels_out_of_range_are_reported_and_index_nothing(ctx):
    from gnomix_amd import _lib
    y, _, lab, _, _ = _case(4099, 3)
    y, lab = y.copy(), lab.copy()
    y[[5, 700]] = [-1, 3]
    lab[[9, 4000]] = [2 ** 31 - 1, -(2 ** 31)]
    ok = (y >= 0) & (y < 3) & (lab >= 0) & (lab < 3)
    assert (~ok).sum() == 4
    ref = np.zeros((3, 3), np.int64)
    np.add.at(ref, (y[ok], lab[ok]), 1)
    rc, cm, _ = _raw_dev(ctx, y, lab, 0, 3)
    assert rc == _lib.GNX_EINVAL and b"4 of 4099" in ctx.lib.gnx_last_error(ctx.h)
    assert np.array_equal(cm.reshape(3, 3), ref)
    # the host-pointer form: the same verdict, the same counts
    cmh = np.zeros((3, 3), np.int64)
    rc = ctx.lib.gnx_confusion(ctx.h, y.ctypes.data, lab.ctypes.data, 0, len(y), 3, cmh.ctypes.data, 0, None)
    assert rc == _lib.GNX_EINVAL and np.array_equal(cmh, ref)
    # true labels out of range against probabilities
    P = np.full((len(y), 3), 0.25)
    rc, cm, _ = _raw_dev(ctx, y, P, 1, 3)
    ref_p = np.zeros((3, 3), np.int64)
    np.add.at(ref_p, (y[(y >= 0) & (y < 3)], 0), 1)
    assert rc == _lib.GNX_EINVAL and np.array_equal(cm.reshape(3, 3), ref_p)


def test_more_than_32_ancestries_are_unsupported(ctx):
    from gnomix_amd import _lib
    y = np.zeros(10, np.int32)
    rc, cm, _ = _raw_dev(ctx, y, y.copy(), 0, 33)
    assert rc == _lib.GNX_EUNSUPPORTED
    assert np.all(cm == -7)                                        # nothing written
    cmh = np.zeros((33, 33), np.int64)
    assert ctx.lib.gnx_confusion(ctx.h, y.ctypes.data, y.ctypes.data, 0, 10, 33, cmh.ctypes.data, 0, None) == _lib.GNX_EUNSUPPORTED
    with pytest.raises(_lib.GnxError):
        _dev_counts(ctx, y, y.copy(), 33)


def test_host_form_equals_the_device_form(ctx):
    from gnomix_amd import resident
    y, P, lab, ref_lab, ref_arg = _case(4099, 32)
    assert np.array_equal(resident.confusion_counts_host(ctx, y, lab, 32), ref_lab)
    assert np.array_equal(resident.confusion_counts_host(ctx, y, P, 32), ref_arg)
    assert np.array_equal(resident.confusion_counts_host(ctx, y, P.astype(np.float32), 32), ref_arg)
    assert np.array_equal(resident.confusion_counts_host(ctx, y[:0], lab[:0], 32), np.zeros((32, 32), np.int64))


def test_early_flush_keeps_the_counts(ctx):
    """the bound that protects the 32-bit counters, lowered from 2^31 to 1 000 elements through the entry's debug argument: a
    workgroup then adds its table to the global counters after every 3 steps of 256 elements (768 + 256 > 1 000), so 10^5 elements
    take at least 100 additions; with the built-in bound every workgroup makes exactly one"""
    n = 100_000
    y, P, lab, ref_lab, ref_arg = _case(n, 3)
    for kind, pred, ref in ((0, lab, ref_lab), (1, P, ref_arg), (2, P.astype(np.float32), ref_arg)):
        rc, cm, few = _raw_dev(ctx, y, pred, kind, 3)
        assert rc == 0 and np.array_equal(cm.reshape(3, 3), ref)
        rc, cm, many = _raw_dev(ctx, y, pred, kind, 3, flush_every=1000)
        assert rc == 0 and np.array_equal(cm.reshape(3, 3), ref)
        assert 1 <= few < n // 1000 <= many
