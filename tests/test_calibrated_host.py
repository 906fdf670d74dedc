"""The calibrator's float64 fit (gnx_fit_isotonic_f64) against scikit-learn bit for bit, fit_calibrator on float64 probabilities
against the reference's Calibrator.fit arithmetic, and a plain numpy restatement of "the calibrated label of a row" (what
gnx_calibrate.h computes for k_calibrate and for Gnofix on a calibrated model) against Calibrator.transform + argmax.  No GPU.

The restatement (calibrated_rows) is pinned to scikit-learn on all four arithmetic routes: maps fitted in float32 or float64, applied
to float32 or float64 rows, with query values planted on every threshold and one ulp either side.  calibrator_inputs / edge_cases
build those inputs; the GPU tests import them and compare the kernels with calibrated_rows.  NaN raw probabilities are out of
scope: IsotonicRegression.transform refuses them (check_array), so nothing here or on the GPU asserts anything about them."""
import numpy as np
import pytest

try:
    from sklearn import isotonic as iso
except ImportError:                  # the helpers below still serve the GPU tests (maps from gnomix_amd.calibrate.fit_isotonic)
    iso = None
needs_sklearn = pytest.mark.skipif(iso is None, reason="scikit-learn is not installed")


def _sk(x, t):
    m = iso.IsotonicRegression(out_of_bounds="clip").fit(x, t)
    return m.X_thresholds_, m.y_thresholds_


def _same(x, t, what):
    from gnomix_amd import calibrate
    xt, yt = calibrate.fit_isotonic(x, t)
    rx, ry = _sk(x, t)
    assert xt.dtype == np.float64 and yt.dtype == np.float64, what
    assert np.array_equal(xt, rx) and np.array_equal(yt, ry), what


@needs_sklearn
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


@needs_sklearn
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
    """maps: per class (x_thr, y_thr) in the dtype they were fitted in; proba (R, A) raw probabilities of either dtype.  Returns
    (R, A) float64 calibrated probabilities and (R,) labels, as scikit-learn 1.7.2 / scipy 1.15.3 / numpy 2.2.6 compute them:
    the rows are cast to the maps' dtype (float64 rows are NARROWED for float32 maps) and clipped to [X_min, X_max]; float32 maps
    interpolate in float32 throughout, in interp1d's own form (k = clip(searchsorted(side="left"), 1, n-1),
    slope * (x - x[k-1]) + y[k-1]); float64 maps go through np.interp (np_interp below: exact hits return y[k] itself).  Then
    store as float64, normalise, NaN -> 1/A, (1, 1+1e-5] -> 1, first maximum."""
    R, A = proba.shape
    out = np.zeros((R, A))
    for c, (xs, ys) in enumerate(maps):
        if len(xs) == 1:
            out[:, c] = ys[0]
            continue
        x = proba[:, c].astype(xs.dtype)
        xc = np.minimum(np.maximum(x, xs[0]), xs[-1])
        if xs.dtype == np.float32:
            k = np.clip(np.searchsorted(xs, xc, side="left"), 1, len(xs) - 1)
            slope = (ys[k] - ys[k - 1]) / (xs[k] - xs[k - 1])
            out[:, c] = slope * (xc - xs[k - 1]) + ys[k - 1]
        else:
            out[:, c] = np_interp(xs, ys, xc)
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


# ---- inputs for every arithmetic route (shared with tests/test_gpu_calibrate.py) ------------------------------------------
def fit_maps(fit_p, y, dtype):
    """one isotonic map per class on (fit_p[:, i], y == i) in `dtype` -> (maps, scikit-learn's fitted models).  Without
    scikit-learn the maps are the library's own fit (pinned to scikit-learn above and in test_host_cpu) and models is None."""
    fit_p = np.ascontiguousarray(fit_p, dtype=dtype)
    if iso is not None:
        models = [iso.IsotonicRegression(out_of_bounds="clip").fit(fit_p[:, i], (y == i).astype(np.float64))
                  for i in range(fit_p.shape[1])]
        maps = [(m.X_thresholds_, m.y_thresholds_) for m in models]
    else:
        from gnomix_amd import calibrate
        models = None
        maps = [calibrate.fit_isotonic(np.ascontiguousarray(fit_p[:, i]), (y == i).astype(dtype)) for i in range(fit_p.shape[1])]
    assert all(xs.dtype == dtype and ys.dtype == dtype for xs, ys in maps)
    return maps, models


def _draw_labels(rng, q):
    """one label per row of q (R, A), drawn with probabilities q / q.sum()"""
    cum = np.cumsum(q / q.sum(axis=1, keepdims=True), axis=1)
    return np.minimum((rng.rand(len(q), 1) > cum).sum(axis=1), q.shape[1] - 1)


def planted_rows(maps, row_dtype):
    """(P, A) rows of `row_dtype` whose column c runs through, for every threshold t of class c: t itself, one ulp either side of it
    in the maps' type and in the rows' type, and the midpoint to the next float32 (a tie when a float64 row is narrowed)"""
    cols = []
    for xs, _ in maps:
        t = xs.astype(row_dtype)
        f = xs.astype(np.float32)
        cand = [t, np.nextafter(t, row_dtype(-np.inf)), np.nextafter(t, row_dtype(np.inf)),
                np.nextafter(xs, xs.dtype.type(-np.inf)).astype(row_dtype), np.nextafter(xs, xs.dtype.type(np.inf)).astype(row_dtype),
                ((f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2).astype(row_dtype)]
        cols.append(np.concatenate(cand))
    P = max(len(c) for c in cols)
    return np.stack([c[np.arange(P) % len(c)] for c in cols], axis=1)


def calibrator_inputs(A, map_dtype, row_dtype, R=None, single=None, n_fit=1500, seed=0):
    """-> (maps, scikit-learn's models or None, rows).  Maps: IsotonicRegression(out_of_bounds="clip").fit per class in map_dtype, on
    Dirichlet draws clipped to [0.2 / A, 0.9]; every other fit row is representable in float32, so that float32 rows hit float64
    thresholds exactly too; class `single` is fitted on one constant probability (a one-point map).  Rows of row_dtype, in this
    order: all zero, all one, half of X_min, midway between X_max and one; planted_rows; Dirichlet draws.  R = None returns them all
    (400 draws); else the first R, with as many draws as it takes (everything before the draws is in from R = 1500 on)."""
    rng = np.random.RandomState(1000 * seed + A)
    fit_p = np.clip(rng.dirichlet(np.ones(A) * 0.6, size=n_fit), 0.2 / A, 0.9)
    fit_p[::2] = fit_p[::2].astype(np.float32)
    y = _draw_labels(rng, fit_p ** 2)
    if single is not None:
        fit_p[:, single] = 0.25
    maps, models = fit_maps(fit_p, y, map_dtype)
    if single is not None:
        assert len(maps[single][0]) == 1                        # the fit really produced a one-point map
    lo = np.array([xs[0] for xs, _ in maps], np.float64)
    hi = np.array([xs[-1] for xs, _ in maps], np.float64)
    head = np.stack([np.zeros(A), np.ones(A), lo / 2, (hi + 1) / 2]).astype(row_dtype)
    planted = planted_rows(maps, row_dtype)
    n_draws = 400 if R is None else max(R - len(head) - len(planted), 0)
    draws = rng.dirichlet(np.ones(A) * 0.6, size=n_draws).astype(row_dtype)
    rows = np.ascontiguousarray(np.concatenate([head, planted, draws])[:R])
    assert rows.dtype == row_dtype
    return maps, models, rows


def edge_cases(A, map_dtype, row_dtype):
    """hand-made maps that reach the special branches -> [(name, maps, rows)]: the NaN row (A > 2: every class 0 -> 0 / 0 -> 1/A,
    and the first maximum of that tie), every class at one (a tie again), and for A == 2 a value in (1, 1 + 1e-5]"""
    flat = [(np.array([0.2, 0.8], map_dtype), np.array([0.0, 1.0], map_dtype)) for _ in range(A)]
    edge = np.zeros((3, A), row_dtype)
    edge[1] = 0.8                                                # every class at 1: A == 2 -> (0, 1), else 1/A each
    edge[2, A - 1] = 0.8                                         # one class at 1, the others at 0
    out = [("flat", flat, edge)]
    # strictly increasing tables whose y values run over many binades: y[k] - y[k-1] is then inexact, and evaluating the segment
    # below a threshold AT the threshold (slope * (x[k] - x[k-1]) + y[k-1]) is not always y[k], which is what np.interp returns
    # there.  Fitted one-hot maps show that difference on a threshold in a few hundred only; here every class has some.
    rng = np.random.RandomState(40 + A)
    n, span = (300, 600.0) if map_dtype == np.float64 else (50, 100.0)
    dense = []
    for _ in range(A):
        xs = np.sort(rng.rand(n))
        xs[::2] = xs[::2].astype(np.float32)
        xs = np.unique(xs.astype(map_dtype))
        ys = np.unique((2.0 ** rng.uniform(-span, 0.0, len(xs))).astype(map_dtype))
        xs = xs[:len(ys)]
        if map_dtype == np.float64:
            at = (ys[1:] - ys[:-1]) / (xs[1:] - xs[:-1]) * (xs[1:] - xs[:-1]) + ys[:-1]
            assert ((at != ys[1:]) & (xs[1:] == xs[1:].astype(np.float32))).any()   # float32 rows reach such a threshold too
        dense.append((xs, ys))
    out.append(("dense", dense, planted_rows(dense, row_dtype)))
    if A == 2:                                                # p1 slightly negative makes p0 = 1 - p1 exceed one by less than 1e-5
        neg = [flat[0], (np.array([0.2, 0.8], map_dtype), np.array([-4e-6, 1.0], map_dtype))]
        out.append(("clamp", neg, np.array([[0.5, 0.2], [0.5, 0.1]], row_dtype)))
    return out


def check_edge_result(name, A, got, lab):
    """what the special branches must give, whoever computed (got, lab) from edge_cases"""
    if name == "flat" and A > 2:
        assert np.array_equal(got[0], np.full(A, 1.0 / A)) and lab[0] == 0    # the NaN row: 1/A each, the first maximum
        assert np.array_equal(got[1], np.full(A, 1.0 / A)) and lab[1] == 0    # a tie of finite values: the first maximum
    if name == "clamp":
        assert got[0, 0] == 1.0 and got[0, 1] < 0 and lab[0] == 0             # clamped to exactly one


@needs_sklearn
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


def np_interp(xs, ys, x):
    """np.interp(x, xs, ys) for float64 x inside [xs[0], xs[-1]] (what scipy's interp1d(kind="linear") calls when x and y are
    float64), restated.  Worked out against numpy 2.2.6 (scikit-learn 1.7.2, scipy 1.15.3), see test_np_interp_rules: the bracket
    is xs[j] <= x < xs[j + 1]; x == xs[j] and x == xs[-1] return ys[j] itself; otherwise slope * (x - xs[j]) + ys[j] with
    slope = (ys[j + 1] - ys[j]) / (xs[j + 1] - xs[j]); where that is NaN, slope * (x - xs[j + 1]) + ys[j + 1]; where that is NaN too
    and ys[j] == ys[j + 1], ys[j].  (With finite thresholds the first form is never NaN: x - xs[j] is not zero there.)"""
    n = len(xs)
    j = np.searchsorted(xs, x, side="right") - 1
    j0 = np.minimum(j, n - 2)
    x0, x1, y0, y1 = xs[j0], xs[j0 + 1], ys[j0], ys[j0 + 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        slope = (y1 - y0) / (x1 - x0)
        v = slope * (x - x0) + y0
        alt = slope * (x - x1) + y1
    v = np.where(np.isnan(v), alt, v)
    v = np.where(np.isnan(v) & (y0 == y1), y0, v)
    v = np.where(x == x0, y0, v)
    return np.where(j >= n - 1, ys[n - 1], v)


def test_np_interp_rules():
    """the rules np_interp states, against the installed numpy: exact hits, the bracket one ulp either side of a threshold, and the
    NaN fallback on non-finite tables (which a fitted map never holds)"""
    rng = np.random.RandomState(11)
    inf = np.inf
    tables = [(np.sort(rng.rand(60)), np.sort(rng.rand(60))), (np.sort(rng.rand(700)), np.sort(rng.rand(700))),
              (np.array([0.0, 1.0]), np.array([-inf, 1.0])), (np.array([0.0, 1.0]), np.array([inf, inf])),
              (np.array([-inf, 0.0]), np.array([1.0, 2.0])), (np.array([0.0, 1.0, 2.0]), np.array([0.0, inf, 5.0])),
              (np.array([0.0, 4e-320]), np.array([0.0, 1.0]))]
    for xs, ys in tables:
        lo = xs[0] if np.isfinite(xs[0]) else -5.0
        q = np.concatenate([xs[np.isfinite(xs)], np.nextafter(xs, -inf), np.nextafter(xs, inf), rng.uniform(lo, xs[-1], size=300)])
        q = np.clip(q[np.isfinite(q)], xs[0], xs[-1])
        for x in (q, q[:5]):                                     # numpy precomputes the slopes only when len(x) >= len(xs)
            with np.errstate(invalid="ignore", over="ignore"):
                want = np.interp(x, xs, ys)
            assert np.array_equal(np_interp(xs, ys, x), want, equal_nan=True)


@needs_sklearn
@pytest.mark.parametrize("A", [2, 3, 7])
@pytest.mark.parametrize("row_dtype", [np.float32, np.float64], ids=["rows32", "rows64"])
@pytest.mark.parametrize("map_dtype", [np.float32, np.float64], ids=["maps32", "maps64"])
def test_restatement_equals_scikit_learn_on_every_route(map_dtype, row_dtype, A):
    """calibrated_rows == Calibrator.transform (+ argmax) bit for bit on the four routes, with rows on every threshold, one ulp
    either side, outside the maps' domain, a one-point map, and the NaN / clamp / tie constructions.  scikit-learn 1.7.2 casts the
    rows to the maps' dtype, clips, and lets scipy 1.15.3 interpolate: float32 maps in interp1d's own float32 searchsorted form,
    float64 maps through np.interp (numpy 2.2.6)."""
    for single in (None, A - 1):
        maps, models, rows = calibrator_inputs(A, map_dtype, row_dtype, single=single)
        hits = sum(int(np.isin(rows[:, c].astype(map_dtype), xs).sum()) for c, (xs, _) in enumerate(maps) if len(xs) > 1)
        assert hits >= sum(len(xs) for xs, _ in maps if len(xs) > 1)             # rows do sit on the thresholds
        got, lab = calibrated_rows(maps, rows)
        want = _Cal(models).transform(rows.copy())
        assert np.array_equal(got, want), (single, float(np.abs(got - want).max()))
        assert np.array_equal(lab, np.argmax(want, axis=1))
        assert (lab != np.argmax(rows, axis=1)).any()            # calibration moves labels here
    for name, maps, rows in edge_cases(A, map_dtype, row_dtype):
        models = [iso.IsotonicRegression(out_of_bounds="clip").fit(xs, ys) for xs, ys in maps]
        assert all(np.array_equal(m.X_thresholds_, xs) and np.array_equal(m.y_thresholds_, ys) for m, (xs, ys) in zip(models, maps))
        if name == "clamp":
            assert 1.0 < 1.0 - float(models[1].transform(rows[:1, 1])[0]) <= 1.0 + 1e-5      # the branch is reached
        got, lab = calibrated_rows(maps, rows)
        want = _Cal(models).transform(rows.copy())
        assert np.array_equal(got, want) and np.array_equal(lab, np.argmax(want, axis=1))
        check_edge_result(name, A, got, lab)
