"""HipGnomix.train from device-resident splits on the MI355X: the model trained from CUDA tensors equals, bit for bit, the model
trained from the same values as numpy arrays — base, smoother, calibrator, accuracies and confusion matrices — and numpy's global
generator ends in the same state.  Geometry: C = 203, M = 10 (W = 20 windows, the last one 3 SNPs wider), context 5, S = 5,
96 / 48 / 24 haplotypes; the smoother is fitted with 8 boosting rounds to keep the file quick (the rounds run the same code)."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C_, M_, S_, CX = 203, 10, 5, 5
W_ = C_ // M_
ROWS = (96, 48, 24)
LD = 208
ROUNDS = 8
TREE_ARRAYS = ("tree_off", "left", "right", "feat", "cond", "tree_class")
CALIB_ARRAYS = ("calib_off", "calib_x", "calib_y")
_host = {}


@pytest.fixture(scope="module")
def ctx():
    from gnomix_amd import _lib
    return _lib.default_context(0)


def _splits(A):
    """three splits of haplotypes whose ancestry is piecewise constant along the chromosome (runs of 7 windows) and in which every
    window column of every split holds every class; SNPs follow a per-class prototype with a tenth of them flipped"""
    rng = np.random.RandomState(40 + A)
    proto = rng.randint(0, 2, size=(A, C_)).astype(np.int8)
    win_of_snp = np.minimum(np.arange(C_) // M_, W_ - 1)
    out, first = [], 0
    for n in ROWS:
        y = ((first + np.arange(n))[:, None] + (np.arange(W_) // 7)[None, :]) % A
        X = proto[y[:, win_of_snp], np.arange(C_)[None, :]]
        X = np.where(rng.random_sample(X.shape) < 0.1, 1 - X, X).astype(np.int8)
        assert all(len(np.unique(y[:, w])) == A for w in range(W_))
        out.append((X, y.astype(np.int32)))
        first += n
    return out


def _model(ctx, A, mode="default", calibrate=True):
    from gnomix_amd import HipGnomix
    from gnomix_amd.train import untrained_model
    return HipGnomix(untrained_model(C_, M_, A, S_, CX, mode, seed=1), ctx=ctx, calibrate=calibrate)


def _train(model, data, mode="default"):
    np.random.seed(7)
    kw = dict(n_rounds=ROUNDS) if mode == "default" else {}
    model.train(data=data, retrain_base=True, evaluate=True, **kw)
    return model, np.random.get_state()


def _host_model(ctx, A=3, calibrate=True, val=True):
    """the host-array model of a configuration, trained once and shared"""
    key = (A, calibrate, val)
    if key not in _host:
        s = _splits(A)
        data = (s[0], s[1], s[2] if val else (None, None))
        _host[key] = _train(_model(ctx, A, calibrate=calibrate), data)
    return _host[key]


def _adjacent(A, val=True):
    """the splits as consecutive row ranges of ONE (168, 208) allocation, X[:, :203] views of 16-byte aligned rows: what
    SimPlan.materialise_dev hands over"""
    import torch
    s = _splits(A)
    X = torch.zeros((sum(ROWS), LD), dtype=torch.int8, device="cuda")
    X[:, :C_] = torch.from_numpy(np.concatenate([p[0] for p in s]))
    Y = torch.from_numpy(np.concatenate([p[1] for p in s])).cuda()
    cuts = np.concatenate([[0], np.cumsum(ROWS)])
    data = [(X[a:b, :C_], Y[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert data[1][0].stride(0) == LD and data[1][0].data_ptr() % 16 == 0
    return (data[0], data[1], data[2] if val else (None, None))


def _separate(A):
    """every split a tensor of its own, rows 203 bytes apart (not 16-byte aligned): retraining concatenates on the device"""
    import torch
    return tuple((torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()) for X, y in _splits(A))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _assert_same_model(dev, host, calibrate):
    d, h = dev.dev.data, host.dev.data
    assert np.array_equal(d.lr_coef, h.lr_coef) and np.any(h.lr_coef != 0)
    assert np.array_equal(d.lr_intercept, h.lr_intercept)
    for k in TREE_ARRAYS:
        assert np.array_equal(getattr(d, k), getattr(h, k)), k
    assert d.base_score == h.base_score and len(h.tree_off) - 1 == ROUNDS * h.A
    if calibrate:
        for k in CALIB_ARRAYS:
            assert getattr(h, k) is not None and np.array_equal(getattr(d, k), getattr(h, k)), k
        assert d.calib_is_f32 == h.calib_is_f32
    else:
        assert d.calib_off is None and h.calib_off is None
    assert dev.accuracies == host.accuracies and len(host.accuracies) in (4, 8)
    assert dev.Confusion_Matrices.keys() == host.Confusion_Matrices.keys()
    for name, (cm, labels) in host.Confusion_Matrices.items():
        cm_d, labels_d = dev.Confusion_Matrices[name]
        assert labels_d == labels and cm_d.dtype == cm.dtype and np.array_equal(cm_d, cm), name


CASES = {
    "adjacent_ld208_calibrated": dict(A=3, calibrate=True, val=True, make=_adjacent),
    "adjacent_ld208_uncalibrated": dict(A=3, calibrate=False, val=True, make=_adjacent),
    "no_validation_split": dict(A=3, calibrate=True, val=False, make=lambda A: _adjacent(A, val=False)),
    "separate_tensors_concatenated": dict(A=3, calibrate=True, val=True, make=_separate),
    "two_ancestries": dict(A=2, calibrate=True, val=True, make=_adjacent),
}


@pytest.mark.parametrize("name", list(CASES))
def test_resident_training_equals_host_training_bit_for_bit(ctx, name):
    c = CASES[name]
    host, host_state = _host_model(ctx, c["A"], c["calibrate"], c["val"])
    before = ctx.bound_stream
    dev, dev_state = _train(_model(ctx, c["A"], calibrate=c["calibrate"]), c["make"](c["A"]))
    assert ctx.bound_stream == before                       # the context's stream is put back
    _assert_same_model(dev, host, c["calibrate"])
    assert _same_state(dev_state, host_state)               # numpy's global generator: the same draws, nothing more
    assert ("val" in host.Confusion_Matrices) == c["val"]


def test_retraining_reads_adjacent_splits_in_place():
    import torch
    from gnomix_amd import resident
    data = _adjacent(3)
    X = resident.adjacent_rows([p[0] for p in data])
    y = resident.adjacent_rows([p[1] for p in data])
    assert X.data_ptr() == data[0][0].data_ptr() and tuple(X.shape) == (sum(ROWS), C_) and X.stride(0) == LD
    assert y.data_ptr() == data[0][1].data_ptr() and tuple(y.shape) == (sum(ROWS), W_)
    assert torch.equal(X, torch.cat([p[0] for p in data])) and torch.equal(y, torch.cat([p[1] for p in data]))
    assert resident.adjacent_rows([data[1][0], data[0][0]]) is None          # out of order
    assert resident.adjacent_rows([data[0][0], data[2][0]]) is None          # a gap
    assert resident.adjacent_rows([p[0] for p in _separate(3)]) is None      # allocations of their own


def test_cuda_in_cuda_out(ctx):
    import torch
    host, _ = _host_model(ctx)
    (X1, _), (X2, _), _ = _splits(3)
    Xd = _adjacent(3)[1][0]                                                  # train2, padded rows
    lab = host.predict(Xd)
    assert lab.is_cuda and lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), host.predict(X2))
    p = host.predict_proba(Xd)
    ph = host.predict_proba(X2)
    assert p.is_cuda and str(p.dtype) == "torch." + str(ph.dtype) and np.array_equal(p.cpu().numpy(), ph)
    B = host.base.predict_proba(Xd)
    Bh = host.base.predict_proba(X2)
    assert B.is_cuda and B.dtype == torch.float64 and np.array_equal(B.cpu().numpy(), Bh)
    s, sh = host.smooth.predict(B), host.smooth.predict(Bh)
    assert s.is_cuda and s.dtype == torch.int64 and np.array_equal(s.cpu().numpy(), sh)
    sp, sph = host.smooth.predict_proba(B), host.smooth.predict_proba(Bh)
    assert sp.is_cuda and str(sp.dtype) == "torch." + str(sph.dtype) and np.array_equal(sp.cpu().numpy(), sph)


def test_train_base_and_train_smoother_take_tensors(ctx):
    host, _ = _host_model(ctx, calibrate=False)
    (X1, y1), (X2, y2), _ = _splits(3)
    d1, d2, _ = _separate(3)
    a, b = _model(ctx, 3, calibrate=False), _model(ctx, 3, calibrate=False)
    a.train_base(X1, y1)
    b.train_base(*d1)
    assert np.array_equal(a.dev.data.lr_coef, b.dev.data.lr_coef) and np.array_equal(a.dev.data.lr_intercept, b.dev.data.lr_intercept)
    a.train_smoother(a.base.predict_proba(X2), y2, n_rounds=ROUNDS)
    b.train_smoother(b.base.predict_proba(d2[0]), d2[1], n_rounds=ROUNDS)
    for k in TREE_ARRAYS:
        assert np.array_equal(getattr(a.dev.data, k), getattr(b.dev.data, k)), k
        assert np.array_equal(getattr(a.dev.data, k), getattr(host.dev.data, k)), k   # and the smoother of the full train()


def test_mixed_inputs_are_a_type_error(ctx):
    s, d = _splits(3), _separate(3)
    m = _model(ctx, 3)
    for data in ((d[0], s[1], s[2]), (s[0], s[1], d[2]), ((d[0][0], s[0][1]), d[1], d[2]), (d[0], d[1], (d[2][0], s[2][1]))):
        with pytest.raises(TypeError, match="mixes host arrays and CUDA tensors"):
            m.train(data=data)
    assert not np.any(m.dev.data.lr_coef)                                    # nothing was trained


def test_other_modes_fall_back_to_the_host_with_one_warning(ctx):
    s, d = _splits(3), _separate(3)
    np.random.seed(7)
    host = _model(ctx, 3, mode="fast", calibrate=False).train(data=tuple(s), retrain_base=True, evaluate=True)
    np.random.seed(7)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        dev = _model(ctx, 3, mode="fast", calibrate=False).train(data=d, retrain_base=True, evaluate=True)
    ours = [w for w in rec if "device-resident" in str(w.message)]
    assert len(ours) == 1 and issubclass(ours[0].category, RuntimeWarning) and '"fast"' in str(ours[0].message)
    dd, hd = dev.dev.data, host.dev.data
    assert hd.smooth_kind == "crf" and np.any(hd.crf_trans != 0)
    for k in ("lr_coef", "lr_intercept", "crf_state", "crf_trans"):
        assert np.array_equal(getattr(dd, k), getattr(hd, k)), k
    assert dev.accuracies == host.accuracies
