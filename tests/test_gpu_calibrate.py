"""The calibrator on the GPU (gnx_calibrate.h through k_calibrate and through Gnofix's calibrated labelling) against the plain numpy
restatement that tests/test_calibrated_host.py pins to scikit-learn, bit for bit, on all four arithmetic routes: maps fitted in
float32 or float64, applied to float32 or float64 raw probabilities.  No assertion here compares device output with device output.
The maps are scikit-learn's where it imports, else the library's own fit (pinned to scikit-learn by the CPU tests).  NaN raw
probabilities are out of scope, as scikit-learn refuses them."""
import numpy as np
import pytest

from test_calibrated_host import _draw_labels, calibrated_rows, calibrator_inputs, check_edge_result, edge_cases, fit_maps

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("map_dtype,row_dtype", [(F32, F32), (F32, F64), (F64, F32), (F64, F64)],
                                 ids=["maps32-rows32", "maps32-rows64", "maps64-rows32", "maps64-rows64"])


@pytest.fixture(scope="module")
def ga():
    import gnomix_amd
    gnomix_amd.load_library()
    return gnomix_amd


def _set_maps(d, maps):
    """the calib_* fields of GnxModelData from per-class (x_thr, y_thr) in the dtype they were fitted in"""
    d.calib_off = np.concatenate([[0], np.cumsum([len(xs) for xs, _ in maps])]).astype(np.int32)
    d.calib_x = np.concatenate([xs.astype(F64) for xs, _ in maps])
    d.calib_y = np.concatenate([ys.astype(F64) for _, ys in maps])
    d.calib_is_f32 = bool(maps[0][0].dtype == F32)
    return d


def _rows_model(ga, A, maps=None):
    """a model for calibrate_rows: a CRF smoother with zero weights (uniform marginals), any A"""
    d = ga.GnxModelData(C=8 * 2 + 1, M=2, A=A, S=5, context=0, smooth_kind="crf", crf_state=np.zeros((A, A)), crf_trans=np.zeros((A, A)))
    return ga.DeviceModel(d if maps is None else _set_maps(d, maps))


# ---------------------------------------------------------------- calibrate_rows: all four routes ----------------------------
@DTYPES
@pytest.mark.parametrize("A", [2, 3, 7, 12, 32])
def test_calibrate_rows_equals_the_restatement(ga, A, map_dtype, row_dtype):
    """R on both sides of the 256-thread block and several blocks; rows on every threshold, one ulp either side, outside the domain;
    a fitted one-point map"""
    for single in (None, A - 1):
        maps, _, rows = calibrator_inputs(A, map_dtype, row_dtype, R=1500, single=single)
        want, lab = calibrated_rows(maps, rows)
        dev = _rows_model(ga, A, maps)
        for R in (1, 255, 256, 257, 1500):
            got = dev.calibrate_rows(rows[:R])
            assert got.dtype == F64 and got.shape == (R, A)
            diff = got != want[:R]
            print("A %d single %s R %d: %d differing values, max |d| %.3g" % (A, single, R, int(diff.sum()), float(np.abs(got - want[:R]).max())))
            assert not diff.any()
            assert np.array_equal(np.argmax(got, axis=1), lab[:R])
        dev.close()


@DTYPES
@pytest.mark.parametrize("A", [2, 3, 7])
def test_special_branches_equal_the_restatement(ga, A, map_dtype, row_dtype):
    """hand-made maps: the NaN row -> 1/A, a tie, (1, 1 + 1e-5] -> 1, and tables on which np.interp's exact-hit rule differs from
    evaluating the segment below the threshold"""
    for name, maps, rows in edge_cases(A, map_dtype, row_dtype):
        want, lab = calibrated_rows(maps, rows)
        dev = _rows_model(ga, A, maps)
        got = dev.calibrate_rows(rows)
        print("A %d %s: %d differing values of %d" % (A, name, int((got != want).sum()), got.size))
        assert np.array_equal(got, want)
        check_edge_result(name, A, got, np.argmax(got, axis=1))
        if name == "flat":
            # the kernel's own label of a tie: uniform CRF marginals 1/A map to equal values (A = 7: below the domain, all zero,
            # the NaN row), so every class ties and the first one wins
            B = np.random.RandomState(0).dirichlet(np.ones(A), size=(2, dev.W))
            raw, _ = dev.smooth_predict(B)
            dev.set_calibrate(True)
            p, y = dev.smooth_predict(B)
            w, wl = calibrated_rows(maps, raw.reshape(-1, A))
            assert np.array_equal(p.reshape(-1, A), w) and np.array_equal(y.reshape(-1), wl)
            if A > 2:
                assert len(np.unique(w)) == 1 and not y.any()
        dev.close()


# ---------------------------------------------------------------- smooth_predict with the calibrate switch on ----------------
@pytest.mark.parametrize("map_dtype", [F32, F64], ids=["maps32", "maps64"])
@pytest.mark.parametrize("A", [2, 3, 7])
@pytest.mark.parametrize("kind", ["xgb", "cnn", "crf"])
def test_smooth_predict_calibrated_equals_the_restatement(ga, kind, A, map_dtype):
    """raw probabilities (switch off; float32 for xgb and cnn, float64 for crf) -> restatement, against every output form of the
    calibrated call.  350 rows: two blocks of k_calibrate, the last one ragged.  The maps are fitted on these very raw values, so
    rows sit exactly on thresholds."""
    from gnomix_amd import synth
    N, W, S, M = 5, 70, 5, 3
    d = synth.synthetic_model(C=W * M + 2, M=M, A=A, S=S, context=0, n_rounds=3, depth=3, seed=30 + A, smooth=kind)
    rng = np.random.RandomState(A)
    B = rng.dirichlet(np.ones(A) * 0.3, size=(N, W))
    plain = ga.DeviceModel(d)
    raw0, _ = plain.smooth_predict(B)
    plain.close()
    flat = raw0.reshape(-1, A)
    y = _draw_labels(rng, flat.astype(F64) ** 0.7)
    y[rng.rand(len(y)) < 0.2] = 0
    maps, _ = fit_maps(flat, y, map_dtype)
    dev = ga.DeviceModel(_set_maps(d, maps))
    raw, _ = dev.smooth_predict(B)                               # the same model, switch off
    assert raw.dtype == (F64 if kind == "crf" else F32)
    want, lab = calibrated_rows(maps, raw.reshape(-1, A))
    want, lab = want.reshape(N, W, A), lab.reshape(N, W)
    assert (lab != np.argmax(raw, axis=-1)).any()                # calibration moves labels here
    sm = ga.HipSmoother(dev, calibrate=True)
    p64, y64 = dev.smooth_predict(B, proba_dtype=F64)
    print("%s A %d: %d differing values of %d" % (kind, A, int((p64 != want).sum()), want.size))
    assert p64.dtype == F64 and np.array_equal(p64, want) and np.array_equal(y64, lab)
    p32, y32 = dev.smooth_predict(B, proba_dtype=F32)
    assert p32.dtype == F32 and np.array_equal(p32, want.astype(F32)) and np.array_equal(y32, lab)
    none, y0 = dev.smooth_predict(B, want_proba=False)
    assert none is None and np.array_equal(y0, lab)
    p, none = dev.smooth_predict(B, want_labels=False)
    assert none is None and p.dtype == F64 and np.array_equal(p, want)
    pp = sm.predict_proba(B)
    assert pp.dtype == F64 and np.array_equal(pp, want) and np.array_equal(sm.predict(B), lab)
    dev.close()


# ---------------------------------------------------------------- the calibrated label inside Gnofix -------------------------
@pytest.mark.parametrize("map_dtype", [F32, F64], ids=["maps32", "maps64"])
@pytest.mark.parametrize("W,A,M,rem,n_ind", [(16, 2, 3, 2, 8), (20, 3, 2, 1, 12)], ids=["a2", "a3"])
def test_gnofix_labels_of_unswitched_haplotypes(ga, W, A, M, rem, n_ind, map_dtype):
    """the geometries of the G26 fixture with synthetic trees: an individual Gnofix did not switch carries the calibrated labels of
    the raw smoother output (max_it = 0: every individual; max_it = 6: at least those whose two haplotypes are equal)"""
    from gnomix_amd import synth
    S = 5
    d = ga.GnxModelData(C=W * M + rem, M=M, A=A, S=S, context=0, smooth_kind="xgb")
    for k, v in synth.synthetic_trees(3, A, S * A, depth=3, seed=260 + A, leaf_scale=1.0).items():
        setattr(d, k, v)
    rng = np.random.RandomState(26 + A)
    X = rng.randint(0, 2, size=(2 * n_ind, d.C)).astype(np.int8)
    B = rng.dirichlet(np.ones(A) * 0.4, size=(2 * n_ind, W))
    X[1:n_ind:2], B[1:n_ind:2] = X[0:n_ind:2], B[0:n_ind:2]      # the first half: two equal haplotypes, nothing to switch
    Bfit = rng.dirichlet(np.ones(A) * 0.4, size=(80, W))
    plain = ga.DeviceModel(d)
    pfit, _ = plain.smooth_predict(Bfit)
    raw, _ = plain.smooth_predict(B)
    plain.close()
    assert raw.dtype == F32
    y = _draw_labels(rng, pfit.reshape(-1, A).astype(F64) ** 0.7)
    y[rng.rand(len(y)) < 0.15] = 0
    maps, _ = fit_maps(pfit.reshape(-1, A), y, map_dtype)
    lab = calibrated_rows(maps, raw.reshape(-1, A))[1].reshape(2 * n_ind, W)
    assert (lab != np.argmax(raw, axis=-1)).any()                # calibration moves labels here
    dev = ga.DeviceModel(_set_maps(d, maps))
    dev.set_calibrate(True)
    Xo, Y, nsw = dev.gnofix(X, B, max_it=0)
    assert np.array_equal(Y, lab) and np.array_equal(Xo, X) and not nsw.any()
    Xo, Y, nsw = dev.gnofix(X, B, max_it=6)
    still = np.repeat(nsw == 0, 2)
    print("W %d A %d: %d of %d individuals not switched" % (W, A, int((nsw == 0).sum()), n_ind))
    assert (nsw == 0).any() and np.array_equal(Y[still], lab[still]) and np.array_equal(Xo[still], X[still])
    dev.close()


# ---------------------------------------------------------------- refusals ---------------------------------------------------
def test_refusals(ga):
    from gnomix_amd import _lib
    A = 3
    rows = np.full((4, A), 1.0 / A)
    out = np.empty((4, A))
    plain = _rows_model(ga, A)                                   # no maps
    assert plain.lib.gnx_calibrate_rows(plain.h, rows.ctypes.data, 1, 4, out.ctypes.data) == _lib.GNX_ESTATE
    with pytest.raises(_lib.GnxError) as e:
        plain.calibrate_rows(rows)
    assert e.value.code == _lib.GNX_ESTATE
    plain.close()
    maps, _, _ = calibrator_inputs(A, F32, F32, R=1)
    dev = _rows_model(ga, A, maps)
    assert dev.lib.gnx_calibrate_rows(dev.h, None, 0, 0, None) == _lib.GNX_OK     # R = 0 is accepted
    assert dev.calibrate_rows(np.zeros((0, A), F32)).shape == (0, A)
    assert dev.lib.gnx_calibrate_rows(dev.h, rows.ctypes.data, 1, -1, out.ctypes.data) == _lib.GNX_EINVAL
    dev.close()
