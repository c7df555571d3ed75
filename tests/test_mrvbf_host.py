"""CPU (not gpu): the numpy reference of MRVBF / MRRTF (tests/_mrvbf_ref.py) on analytic cases, its sensitivity to the
one transcendental function it calls, and default_levels, slope_threshold and the argument checks of
descriptools_amd.mrvbf, which run before any library call.

The valley raster.  243 x 300 cells at px = 25 m; across the columns a plateau of 60 cells, a 25 % side slope rising
over 60 cells, a flat valley floor of 60 cells, and the mirror image.  The whole raster carries a gradient of 0.0101 m
per row and 0.0037 m per column (0.04 % and 0.015 %: a valley drains).  The gradient is what makes the case say
anything about MRRTF: on a floor of exactly equal heights no cell is strictly higher than another, the higher percentile
is 0 at radius 3 and 6, and M_2 -- a lower bound of every later level -- is 1.99 by the definition itself.  With the
gradient the reference gives, on row 121: mrvbf 3.98 to 3.99 on the floor axis (columns 140 to 160) and 0.0009 at
mid-slope (columns 90, 210); mrrtf 4.87 and 4.97 on the outer plateau (columns 5, 295) and 0.754 / 0.861 on the floor
at columns 140 / 160.  On the axis itself (column 150) mrrtf is 1.249: the floor is widest there, and level 3 still
finds few cells higher than it within its radius."""
import numpy as np
import pytest

import _mrvbf_ref as R
from descriptools_amd import mrvbf


def valley():
    y, x = np.mgrid[0:243, 0:300]
    d = np.abs(x - 149.5)
    z = np.where(d <= 30, 0.0, np.where(d <= 90, (d - 30) * 25 * 0.25, 60 * 25 * 0.25))
    return (z + 50 + 0.0101 * y + 0.0037 * x).astype(np.float32)


def test_constant_raster_is_flat_at_every_level():
    dem = np.full((50, 60), 7, np.float32)
    levels = R.default_levels(dem.shape)
    assert levels == 4
    r = R.indices(dem, 25.0, ("mrvbf", "mrrtf"), pctl_valley=0.4, pctl_ridge=0.4)
    assert np.array_equal(r["mrvbf"], r["mrrtf"])
    assert (r["mrvbf"] > levels - 1).all() and (r["mrvbf"] < levels).all()


def test_valley_floor_slopes_and_plateau():
    dem = valley()
    assert R.default_levels(dem.shape) == 5
    r = R.indices(dem, 25.0, ("mrvbf", "mrrtf"))
    v, t = r["mrvbf"][121], r["mrrtf"][121]
    print("mrvbf floor %r mid-slope %r %r; mrrtf plateau %r %r floor %r %r axis %r"
          % (v[140:161].min(), v[90], v[210], t[5], t[295], t[140], t[160], t[150]))
    assert (v[140:161] > 3).all()
    assert v[90] < 0.01 and v[210] < 0.01
    assert t[5] > 4 and t[295] > 4
    assert t[140] < 1 and t[160] < 1


def test_default_levels_and_slope_threshold():
    for shape, want in (((1, 1), 2), ((12, 100), 3), ((243, 300), 5), ((9, 100), 2), ((36, 36), 4), ((27, 36), 3),
                        ((10 ** 6, 10 ** 6), 10)):
        assert mrvbf.default_levels(shape) == R.default_levels(shape) == want, shape
    assert mrvbf.slope_threshold(25) == R.slope_threshold(25) == 16
    assert mrvbf.slope_threshold(25 / 3) == pytest.approx(32, rel=1e-15)
    assert mrvbf.slope_threshold(7.3) == R.slope_threshold(7.3)
    assert mrvbf.LEVELS_MAX == R.LEVELS_MAX == 10 and mrvbf.PERCENTILE_RADIUS_MAX == 16
    assert mrvbf.OUTPUTS == ("mrvbf", "mrrtf")
    assert list(mrvbf._exponents(10)) == R.exponents(10) and list(mrvbf._gauss_weights()) == R.gauss_weights()


@pytest.mark.parametrize("shape,seed", [((130, 200), 130 * 7 + 200), ((67, 131), 67 * 7 + 131)])
def test_pow_as_exp_log_moves_no_cell(shape, seed):
    """the perturbation the GPU tolerance is derived from (tests/test_gpu_mrvbf.py): pow(q, p) -> exp(p log q)"""
    dem = R.terrain(shape[0], shape[1], seed)
    a = R.indices(dem, 30.0, ("mrvbf", "mrrtf"), levels=10)
    b = R.indices(dem, 30.0, ("mrvbf", "mrrtf"), levels=10, power=R.pow_exp_log)
    for n in a:
        assert not np.isnan(b[n]).any()
        moved = a[n].view(np.int32).astype(np.int64) - b[n].view(np.int32).astype(np.int64)
        print(shape, n, "moved", int((moved != 0).sum()), "by at most", int(np.abs(moved).max()))
        assert not moved.any()


def test_percentile_and_coarsen_of_the_reference_on_cases_done_by_hand():
    d = np.array([[1, 2, 3], [4, 5, 6], [7, 8, np.nan]], np.float32)
    lo, hi = R.elevation_percentile(d, 1, "lower"), R.elevation_percentile(d, 1, "higher")
    assert lo[1, 1] == np.float32(2 / 5) and hi[1, 1] == np.float32(2 / 5)       # 2, 4 below; 6, 8 above
    assert lo[0, 0] == 0 and hi[0, 0] == np.float32(2 / 3) and lo[2, 2] == -100 and hi[2, 2] == -100
    assert lo[1, 2] == np.float32(2 / 3) and hi[2, 1] == 0                       # the NaN cell is not counted
    z3, s3 = R.coarsen(np.full((7, 4), 12.5, np.float32), 10.0)
    assert z3.shape == s3.shape == (3, 2) and (z3 == 12.5).all()
    assert (s3 >= 0).all() and (s3 < 1e-12).all()    # num / den rounds: the smoothed constant is level to 1e-16 only
    y, x = np.mgrid[0:40, 0:40]
    z3, s3 = R.coarsen((0.5 * x).astype(np.float32), 10.0)                       # a plane of 5 %
    assert np.allclose(s3[:, 2:-3], 5.0, rtol=1e-6)
    assert np.allclose(z3[5, 2:-3], 0.5 * (3 * np.arange(2, 11) + 1), rtol=1e-6)
    z3, s3 = R.coarsen(np.full((6, 6), -100, np.float32), 10.0)
    assert (z3 == -100).all() and (s3 == -100).all()


# ---- the argument checks ---------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from descriptools_amd import _lib

    def refuse():
        raise AssertionError("a bad argument reached the library")
    monkeypatch.setattr(_lib, "lib", refuse)


DEM = np.zeros((9, 11), np.float32)


@pytest.mark.parametrize("kw", [dict(outputs=("mrvbf", "vbf")), dict(outputs=("mrvbf", "mrvbf")), dict(outputs="mrvbf"),
                                dict(outputs=()), dict(outputs=None), dict(levels=1), dict(levels=11),
                                dict(levels=3.0), dict(levels=True), dict(px=0), dict(px=-1.0),
                                dict(px=float("nan")), dict(px=float("inf")), dict(slope_threshold=0),
                                dict(slope_threshold=float("nan")), dict(slope_threshold=-4.0),
                                dict(pctl_valley=0), dict(pctl_valley=1.01), dict(pctl_valley=float("nan")),
                                dict(pctl_ridge=0.0), dict(pctl_ridge=2), dict(pctl_ridge=None),
                                dict(dem=np.zeros(5, np.float32)), dict(dem=np.full((3, 3), 0.1, np.float64))],
                         ids=lambda kw: "-".join("%s=%r" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_indices_refuses_before_any_library_call(no_library, kw):
    args = dict(dem=DEM, px=10.0)
    args.update(kw)
    with pytest.raises(ValueError):
        mrvbf.indices(**args)


def test_the_other_ops_refuse_before_any_library_call(no_library):
    f64 = np.full((3, 3), 0.1, np.float64)
    for bad in (0, 17, 3.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            mrvbf.elevation_percentile(DEM, bad)
    for bad in ("low", "Lower", None, 1):
        with pytest.raises(ValueError, match="kind"):
            mrvbf.elevation_percentile(DEM, 3, bad)
    with pytest.raises(ValueError, match="float32"):
        mrvbf.elevation_percentile(f64, 3)
    for bad in (0, -2.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="px"):
            mrvbf.coarsen(DEM, bad)
        with pytest.raises(ValueError, match="px"):
            mrvbf.slope_threshold(bad)
        with pytest.raises(ValueError, match="px"):
            mrvbf.mrvbf(DEM, bad)
    with pytest.raises(ValueError, match="float32"):
        mrvbf.coarsen(f64, 10.0)
    with pytest.raises(ValueError, match="2-D"):
        mrvbf.coarsen(np.zeros((2, 2, 2), np.float32), 10.0)
    with pytest.raises(ValueError, match="levels"):
        mrvbf.mrrtf(DEM, 10.0, levels=0)
    with pytest.raises(ValueError, match="float32"):
        mrvbf.mrrtf(f64, 10.0)


def test_alias_module_serves_the_same_functions():
    import descriptools.mrvbf as alias
    assert alias.indices is mrvbf.indices and alias.coarsen is mrvbf.coarsen
    assert alias.elevation_percentile is mrvbf.elevation_percentile and alias.LEVELS_MAX == 10
    assert "indices" in alias.__all__ and not [n for n in alias.__all__ if n.startswith("_")]


def test_no_cpu_fallback_without_gpu():
    from descriptools_amd import _lib
    if _lib.lib().dt_device_count() > 0:
        return  # tests/test_gpu_mrvbf.py has the calls that succeed
    with pytest.raises(RuntimeError, match="no HIP device"):
        mrvbf.indices(DEM, 10.0, ("mrvbf", "mrrtf"))
    with pytest.raises(RuntimeError):
        mrvbf.elevation_percentile(DEM, 3)
    with pytest.raises(RuntimeError):
        mrvbf.coarsen(DEM, 10.0)
