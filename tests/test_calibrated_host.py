"""The calibrator's float64 fit (gnx_fit_isotonic_f64) against scikit-learn bit for bit, fit_calibrator on float64 probabilities
against the reference's Calibrator.fit arithmetic, and a plain numpy restatement of "the calibrated label of a row" (what
gnx_calibrate.h computes for k_calibrate and for Gnofix on a calibrated model) against Calibrator.transform + argmax.  No GPU."""
import numpy as np
import pytest

iso = pytest.importorskip("sklearn.isotonic")


def _sk(x, t):
    m = iso.IsotonicRegression(out_of_bounds="clip").fit(x, t)
    return m.X_thresholds_, m.y_thresholds_


def _same(x, t, what):
    from gnomix_amd import calibrate
    xt, yt = calibrate.fit_isotonic(x, t)
    rx, ry = _sk(x, t)
    assert xt.dtype == np.float64 and yt.dtype == np.float64, what
    assert np.array_equal(xt, rx) and np.array_equal(yt, ry), what


def test_isotonic_f64_fit_equals_scikit_learn_bit_for_bit():
    for seed in range(40):
        r = np.random.RandomState(100 + seed)
        n = int(r.randint(3, 600))
        x = r.beta(0.3, 0.3, size=n)
        if seed % 3 == 0:
            x = np.round(x, 2)                                     # heavy ties in x
        if seed % 4 == 0:
            x[: n // 2] += 4e-16 * r.randint(0, 3, size=n // 2)    # values closer than float64's resolution (1e-15)
        t = (r.rand(n) < x).astype(np.float64)
        if seed % 5 == 0:
            t = r.rand(n)                                          # real-valued targets: block means that are no short fractions
        _same(x, t, ("random", seed))
    r = np.random.RandomState(7)
    x = r.rand(300)
    _same(x, np.full(300, 0.25), "constant y")
    _same(x, np.zeros(300), "all zero")
    _same(x, np.sort(r.rand(300))[np.argsort(np.argsort(x))], "already monotone")
    _same(x, -np.sort(r.rand(300))[np.argsort(np.argsort(x))], "anti-monotone: one block")
    _same(np.full(50, 0.5), r.rand(50), "one x")
    _same(np.array([0.3]), np.array([1.0]), "n = 1")
    _same(np.array([0.3, 0.1]), np.array([1.0, 0.0]), "n = 2, increasing")
    _same(np.array([0.3, 0.1]), np.array([0.0, 1.0]), "n = 2, violating")
    _same(np.array([0.2, 0.2]), np.array([0.0, 1.0]), "n = 2, tied")


def test_fit_calibrator_on_float64_equals_the_references_fit():
    """Calibrator.fit (Calibration.py:43-55): one IsotonicRegression per class on (proba[:, i], one-hot column i of sorted classes),
    here on float64 probabilities as the CRF smoother returns them"""
    from gnomix_amd import calibrate
    rng = np.random.RandomState(26)
    A = 4
    proba = rng.dirichlet(np.ones(A) * 0.5, size=2500)
    y = np.array([rng.choice(A, p=p / p.sum()) for p in proba ** 0.7]) * 3 + 1    # labels need not be 0 .. A-1: sorted order counts
    d = calibrate.fit_calibrator(proba, y, A)
    assert d["calib_is_f32"] is False and d["calib_x"].dtype == np.float64
    classes = np.unique(y)
    for i in range(A):
        rx, ry = _sk(proba[:, i], (y == classes[i]).astype(np.float64))
        sl = slice(d["calib_off"][i], d["calib_off"][i + 1])
        assert np.array_equal(d["calib_x"][sl], rx) and np.array_equal(d["calib_y"][sl], ry), i
    d32 = calibrate.fit_calibrator(proba.astype(np.float32), y, A)      # float32 stays on the float32 fit
    assert d32["calib_is_f32"] is True
    with pytest.raises(ValueError):
        calibrate.fit_calibrator(proba, np.zeros_like(y), A)


# ---- the calibrated label, restated in plain numpy --------------------------------------------------------------------------
def calibrated_rows(maps, proba):
    """maps: per class (x_thr, y_thr) in the dtype they were fitted in; proba (R, A) raw probabilities.  Returns (R, A) float64
    calibrated probabilities and (R,) labels: clip, interpolate in the fitted type (float32 maps on float32 inputs: float32
    throughout; else float64), store as float64, normalise, NaN -> 1/A, (1, 1+1e-5] -> 1, first maximum."""
    R, A = proba.shape
    out = np.zeros((R, A))
    for c, (xs, ys) in enumerate(maps):
        x = proba[:, c]
        if len(xs) == 1:
            out[:, c] = ys[0]
            continue
        dt = np.float32 if (xs.dtype == np.float32 and x.dtype == np.float32) else np.float64
        xc = np.minimum(np.maximum(x, xs[0]), xs[-1]).astype(dt)
        k = np.clip(np.searchsorted(xs, xc, side="left"), 1, len(xs) - 1)
        if dt == np.float32:
            slope = (ys[k] - ys[k - 1]) / (xs[k] - xs[k - 1])
            out[:, c] = slope * (xc - xs[k - 1]) + ys[k - 1]
        else:
            slope = (ys[k] - ys[k - 1]) / (xs[k] - xs[k - 1])          # in the maps' own type
            out[:, c] = slope.astype(np.float64) * (xc - xs[k - 1].astype(np.float64)) + ys[k - 1].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if A == 2:
            out[:, 0] = 1.0 - out[:, 1]
        else:
            out /= out.sum(axis=1)[:, None]
    out[np.isnan(out)] = 1.0 / A
    out[(out > 1.0) & (out <= 1.0 + 1e-5)] = 1.0
    return out, np.argmax(out, axis=1)


class _Cal:
    """the reference's Calibrator.transform / normalize (src/Smooth/Calibration.py:26-41, 57-69), restated without its plotting
    imports, around scikit-learn's own fitted models"""

    def __init__(self, models):
        self.models, self.n_classes = models, len(models)

    def transform(self, proba):
        flat = proba.reshape(-1, self.n_classes)
        o = np.zeros((flat.shape[0], self.n_classes))
        for i in range(self.n_classes):
            o[:, i] = self.models[i].transform(flat[:, i])
        with np.errstate(invalid="ignore", divide="ignore"):
            if self.n_classes == 2:
                o[:, 0] = 1.0 - o[:, 1]
            else:
                o /= np.sum(o, axis=1)[:, np.newaxis]
        o[np.isnan(o)] = 1.0 / self.n_classes
        o[(1.0 < o) & (o <= 1.0 + 1e-5)] = 1.0
        return o


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("A", [2, 3])
def test_numpy_restatement_of_the_calibrated_label(A, dtype):
    rng = np.random.RandomState(3 + A)
    fit_p = rng.dirichlet(np.ones(A) * 0.6, size=1500).astype(dtype)
    fit_p[:, :] = np.clip(fit_p, 0.05, 0.9)                      # the maps' domain is [0.05, 0.9]: rows outside are clipped
    y = np.array([rng.choice(A, p=p / p.sum()) for p in fit_p.astype(np.float64) ** 2])
    models = [iso.IsotonicRegression(out_of_bounds="clip").fit(fit_p[:, i], (y == i).astype(np.float64)) for i in range(A)]
    maps = [(m.X_thresholds_, m.y_thresholds_) for m in models]
    assert maps[0][0].dtype == dtype
    rows = rng.dirichlet(np.ones(A) * 0.6, size=400).astype(dtype)
    rows[0] = 0.0                                                # all clipped below
    rows[1] = 1.0                                                # all clipped above
    got, lab = calibrated_rows(maps, rows)
    want = _Cal(models).transform(rows.copy())
    assert np.array_equal(got, want) and np.array_equal(lab, np.argmax(want, axis=1))
    assert (lab != np.argmax(rows, axis=1)).any()                # calibration moves labels here
    # a NaN row: maps that are 0 at the bottom of their domain, evaluated there (A > 2: 0 / 0; A == 2 never divides)
    flat = [(np.array([0.2, 0.8], dtype), np.array([0.0, 1.0], dtype)) for _ in range(A)]
    fm = []
    for xs, ys in flat:
        m = iso.IsotonicRegression(out_of_bounds="clip").fit(xs, ys)
        assert np.array_equal(m.X_thresholds_, xs) and np.array_equal(m.y_thresholds_, ys)
        fm.append(m)
    edge = np.zeros((3, A), dtype)
    edge[1] = 0.8                                                # every class at 1: A == 2 -> (0, 1), else 1/A each
    edge[2, A - 1] = 0.8                                         # one class at 1, the others at 0
    got, lab = calibrated_rows(flat, edge)
    want = _Cal(fm).transform(edge.copy())
    assert np.array_equal(got, want) and np.array_equal(lab, np.argmax(want, axis=1))
    if A > 2:
        assert np.array_equal(got[0], np.full(A, 1.0 / A)) and lab[0] == 0   # the NaN row: 1/A each, the first maximum
    # a value in (1, 1 + 1e-5]: A == 2 with p1 slightly negative makes p0 = 1 - p1 exceed one by less than 1e-5
    if A == 2:
        neg = [flat[0], (np.array([0.2, 0.8], dtype), np.array([-4e-6, 1.0], dtype))]
        nm = [fm[0], iso.IsotonicRegression(out_of_bounds="clip").fit(*neg[1])]
        assert np.array_equal(nm[1].y_thresholds_, neg[1][1])
        row = np.array([[0.5, 0.2], [0.5, 0.1]], dtype)
        p1 = float(nm[1].transform(row[:1, 1])[0])
        assert 1.0 < 1.0 - p1 <= 1.0 + 1e-5                                  # the branch is reached
        got, lab = calibrated_rows(neg, row)
        want = _Cal(nm).transform(row.copy())
        assert np.array_equal(got, want) and np.array_equal(lab, np.argmax(want, axis=1))
        assert got[0, 0] == 1.0 and got[0, 1] < 0 and lab[0] == 0            # clamped to exactly one
