"""CPU (not gpu): the numpy reference of descriptools_amd.filters (tests/_filters_ref.py) against brute force in plain
Python, the rank table, the properties of the denoising on the reference, and the argument checks, which raise before
any library call."""
import math

import numpy as np
import pytest

import _filters_ref as R

SHAPE = (37, 45)
_CACHE = {}


def _dem():
    if "dem" not in _CACHE:
        d = R.terrain(SHAPE[0], SHAPE[1], seed=11)
        d.setflags(write=False)
        _CACHE["dem"] = d
    return _CACHE["dem"]


def _windows(radius):
    if radius not in _CACHE:
        _CACHE[radius] = R.brute_windows(_dem(), radius)
    return _CACHE[radius]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_terrain_holds_every_kind_of_invalid_height():
    d = _dem()
    share = 1.0 - R.valid(d).mean()
    assert 0.05 <= share <= 0.20, share
    assert np.isnan(d).sum() == 1 and (d == np.inf).sum() == 1 and (d == -np.inf).sum() == 1
    assert (d == -150).sum() == 1 and (d == -100).any()


def test_key_orders_like_the_reals_and_round_trips():
    z = np.array([-99.5, -1.0, -0.0, 0.0, 1e-45, 1.0, 3.5, 3.4e38], np.float32)
    k = R.keys(z)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert np.array_equal(_bits(R.unkey(k)), _bits(z))
    assert [R._key_int(v) for v in z] == k.tolist()


@pytest.mark.parametrize("radius", [1, 5, 50])
def test_extremes_reference_equals_brute_force(radius):
    d = _dem()
    ref = R.extremes(d, radius)
    ok = R.valid(d)
    for name in ("min", "max", "range"):
        assert ref[name].dtype == np.float32 and (ref[name][~ok] == -100).all()
    for y, x, w in _windows(radius):
        lo, hi = np.float32(w[0][1]), np.float32(w[-1][1])
        assert ref["min"][y, x] == lo and ref["max"][y, x] == hi, (y, x)
        assert ref["range"][y, x] == np.float32(np.float64(hi) - np.float64(lo)), (y, x)
    if radius == 50:  # the window is the raster
        v = d[ok]
        assert (ref["min"][ok] == v.min()).all() and (ref["max"][ok] == v.max()).all()


@pytest.mark.parametrize("radius", [1, 5])
def test_opening_and_closing_reference_equal_brute_force(radius):
    d = _dem()
    ok = R.valid(d)
    lo, hi = R.extremes(d, radius)["min"], R.extremes(d, radius)["max"]
    op, cl = R.opening(d, radius), R.closing(d, radius)
    H, W = d.shape
    for y, x, _ in _windows(radius):
        ys, xs = slice(max(y - radius, 0), y + radius + 1), slice(max(x - radius, 0), x + radius + 1)
        m = ok[ys, xs]
        assert op[y, x] == lo[ys, xs][m].max() and cl[y, x] == hi[ys, xs][m].min(), (y, x)
    assert (op[~ok] == -100).all() and (cl[~ok] == -100).all()
    assert (op[ok] <= d[ok]).all() and (cl[ok] >= d[ok]).all()  # anti-extensive, extensive


@pytest.mark.parametrize("radius", [1, 3, 16])
def test_percentile_reference_equals_brute_force(radius):
    d = _dem()
    ok = R.valid(d)
    for q in (0, 25, 50, 100):
        ref = R.percentile(d, radius, q)
        assert ref.dtype == np.float32 and (ref[~ok] == -100).all()
        for y, x, w in _windows(radius):
            want = np.float32(w[R.brute_rank(len(w), q)][1])
            assert _bits(ref[y, x]) == _bits(want), (q, y, x)
    ext = R.extremes(d, radius)
    assert np.array_equal(_bits(R.percentile(d, radius, 0)), _bits(ext["min"]))
    assert np.array_equal(_bits(R.percentile(d, radius, 100)), _bits(ext["max"]))


def test_rank_table_is_pinned():
    from descriptools_amd import filters
    t0, t50, t100 = (filters.rank_table(2, q) for q in (0, 50, 100))
    for t in (t0, t50, t100):
        assert t.dtype == np.uint16 and t.shape == (26,) and t[0] == 0
    # n = 1, 2, 3, an even and an odd count
    assert [int(t0[n]) for n in (1, 2, 3, 24, 25)] == [0, 0, 0, 0, 0]
    assert [int(t50[n]) for n in (1, 2, 3, 24, 25)] == [0, 1, 1, 12, 12]  # floor(0.5 (n - 1) + 0.5): the upper middle
    assert [int(t100[n]) for n in (1, 2, 3, 24, 25)] == [0, 1, 2, 23, 24]
    assert [int(v) for v in filters.rank_table(1, 25)] == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    for r, q in ((1, 10.0), (16, 33.3), (16, 99.9)):
        t = filters.rank_table(r, q)
        n = np.arange(1, (2 * r + 1) ** 2 + 1)
        assert t.size == (2 * r + 1) ** 2 + 1
        assert np.array_equal(t[1:].astype(np.int64), R.rank_index(n, q))
        assert [int(v) for v in t[1:]] == [R.brute_rank(int(k), q) for k in n]


# ---- denoising on the reference ---------------------------------------------------------------------------------------
def test_denoise_keeps_a_level_raster():
    d = np.full((20, 24), 123.25, np.float32)
    assert np.array_equal(_bits(R.denoise(d, 2.0)), _bits(d))


def test_denoise_keeps_a_step_between_two_plateaus():
    d = np.full((24, 30), 50.0, np.float32)
    d[:, 15:] = 60.0
    assert np.array_equal(_bits(R.denoise(d, 2.0)), _bits(d))


def test_denoise_keeps_invalid_cells_and_bounds_the_change():
    d = R.terrain(41, 53, seed=3, noise=0.002)
    ok = R.valid(d)
    for mc in (0.5, 0.05):
        out = R.denoise(d, 2.0, max_change=mc)
        assert np.array_equal(_bits(out)[~ok], _bits(d)[~ok])
        assert (np.abs(out[ok].astype(np.float64) - d[ok].astype(np.float64)) <= mc).all()
        assert (out[ok] != d[ok]).any()


def test_denoise_plane_at_the_edge():
    """the linear extrapolation of missing neighbours keeps a plane a plane up to the raster's edge"""
    y, x = np.mgrid[0:30, 0:40]
    d = (100.0 + 0.5 * x + 0.25 * y).astype(np.float32)
    out = R.denoise(d, 2.0)
    assert np.abs(out.astype(np.float64) - d).max() < 0.005


@pytest.mark.parametrize("holes", [False, True])
def test_denoise_halves_the_error_of_a_noisy_surface(holes):
    """A smooth surface with a 10 m step plus Gaussian noise of sigma 0.15 m, px 2, the defaults: the RMSE against the
    clean surface falls below half the input's.  Measured with this reference on the 120 x 150 raster of seed 7: 0.0374
    against 0.1491 without holes, 0.0399 against 0.1491 with 5 % holes."""
    clean, noisy = R.step_surface(120, 150, 2.0, seed=7, holes=holes)
    ok = R.valid(noisy)
    out = R.denoise(noisy, 2.0)
    rmse = lambda a: float(np.sqrt(np.mean((a[ok].astype(np.float64) - clean[ok].astype(np.float64)) ** 2)))
    before, after = rmse(noisy), rmse(out)
    print("rmse", before, after)
    assert 0.13 < before < 0.17
    assert after < 0.5 * before, (before, after)


# ---- argument checks: ValueError before any library call -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from descriptools_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def test_bad_arguments_raise_before_any_library_call(no_library):
    from descriptools_amd import filters
    d = np.zeros((6, 7), np.float32)
    inexact = np.full((6, 7), 0.1, np.float64)
    bad = [
        lambda: filters.extremes(d, 0), lambda: filters.extremes(d, 4097), lambda: filters.extremes(d, 1.0),
        lambda: filters.extremes(d, True), lambda: filters.extremes(d, 1, ()), lambda: filters.extremes(d, 1, "min"),
        lambda: filters.extremes(d, 1, ("min", "mean")), lambda: filters.extremes(d, 1, ("min", "min")),
        lambda: filters.extremes(inexact, 1), lambda: filters.extremes(np.zeros(5, np.float32), 1),
        lambda: filters.minimum(d, 0), lambda: filters.maximum(d, 4097), lambda: filters.relief(d, -1),
        lambda: filters.opening(d, 0), lambda: filters.closing(d, 4097), lambda: filters.opening(inexact, 1),
        lambda: filters.percentile(d, 0), lambda: filters.percentile(d, 17), lambda: filters.percentile(d, 2.0),
        lambda: filters.percentile(d, 1, float("nan")), lambda: filters.percentile(d, 1, -0.1),
        lambda: filters.percentile(d, 1, 100.1), lambda: filters.percentile(d, 1, float("inf")),
        lambda: filters.percentile(d, 1, "half"), lambda: filters.percentile(inexact, 1), lambda: filters.median(d, 17),
        lambda: filters.rank_table(0, 50), lambda: filters.rank_table(1, 101),
        lambda: filters.denoise(d, 0.0), lambda: filters.denoise(d, float("nan")), lambda: filters.denoise(d, 2.0, 0),
        lambda: filters.denoise(d, 2.0, 17), lambda: filters.denoise(d, 2.0, threshold=0),
        lambda: filters.denoise(d, 2.0, threshold=90), lambda: filters.denoise(d, 2.0, threshold=float("nan")),
        lambda: filters.denoise(d, 2.0, threshold=1e-9), lambda: filters.denoise(d, 2.0, iterations=0),
        lambda: filters.denoise(d, 2.0, iterations=33), lambda: filters.denoise(d, 2.0, iterations=1.5),
        lambda: filters.denoise(d, 2.0, max_change=0), lambda: filters.denoise(d, 2.0, max_change=float("inf")),
        lambda: filters.denoise(inexact, 2.0), lambda: filters.denoise(np.zeros((2, 3, 4), np.float32), 2.0),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d raised nothing" % i)


def test_alias_module_serves_the_same_functions():
    import descriptools.filters as alias
    from descriptools_amd import filters
    for name in ("extremes", "minimum", "maximum", "relief", "opening", "closing", "percentile", "median",
                 "rank_table", "denoise"):
        assert getattr(alias, name) is getattr(filters, name)
    assert filters.OUTPUTS == ("min", "max", "range")
    assert math.isclose(filters.RADIUS_MAX, 4096)
