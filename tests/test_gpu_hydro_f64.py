"""GPU (-m gpu): conditioning on float64 heights (dt_hydro.hip k_fill_relax_f64 / k_flat_init_f64, then the float32
tier's flat rounds): against the rank construction of test_hydro_f64_host.expected_f64 on genuinely float64 DEMs, bit
for bit against the float32 tier on heights both tiers hold, the asynchronous budget, and run_host's resident
recipe."""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import load_example
from test_hydro_f64_host import expected_f64, rough_f64

pytestmark = pytest.mark.gpu

SHAPES = [(300, 417, 1), (64, 64, 2), (129, 1000, 3), (1, 77, 4), (50, 1, 5), (150, 211, 6)]


def _check64(dem, px):
    from descriptools_amd import flowacc, flowdir
    fdr, filled = flowdir.d8_conditioned(dem, px, return_filled=True, heights="float64")
    fdr_e, filled_e = expected_f64(dem, px)
    assert filled.dtype == np.float64
    assert np.array_equal(filled, filled_e), "filled surface: %d cells differ" % int((filled != filled_e).sum())
    assert np.array_equal(fdr, fdr_e), "conditioned D8: %d cells differ" % int((fdr != fdr_e).sum())
    valid = dem != -100
    assert (fdr[valid] != 0).all(), "every valid cell has a code"
    acc = flowacc.accumulate(fdr, np.where(valid, 0, -100).astype(np.float32))  # (the nodata mask: heights need not fit)
    assert (acc[valid] >= 0).all(), "no D8 cycle"
    return fdr, filled


def _async64(dem, px, rounds):
    """dt_dev_condition_d8_f64_async on a fresh context: (fdr, filled, status)"""
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    H, W = dem.shape
    ctx = Context()
    d, f, c = ctx.to_device(np.ascontiguousarray(dem, np.float64)), ctx.empty((H, W), np.float64), ctx.empty((H, W), np.uint8)
    try:
        _lib.check(_lib.lib().dt_dev_condition_d8_f64_async(ctx.h, d.ptr, H, W, px, f.ptr, c.ptr, rounds))
        st = ctx.status()
        return c.to_host(), f.to_host(), st
    finally:
        for b in (d, f, c):
            b.free()
        ctx.close()


@pytest.mark.parametrize("H,W,seed", SHAPES)
def test_float64_conditioning_against_the_rank_construction(H, W, seed):
    from descriptools_amd import flowdir
    dem = rough_f64(H, W, seed)
    fdr, filled = _check64(dem, 10.0)
    if min(H, W) >= 3:  # (on a 1-D raster every cell is an outlet: rounding changes no code there)
        r32 = flowdir.d8_conditioned(dem.astype(np.float32), 10.0)
        assert (r32 != fdr).sum() > 0, "rounding to float32 changes the routing of this DEM"


@pytest.fixture
def coloured_rounds():
    """debug key 8 = 1: the coloured rounds (dt_hydro.hip hy_tile_of_block) on rasters of any size"""
    from descriptools_amd import _lib
    L = _lib.lib()
    _lib.check(L.dt_debug_set(8, 1))
    yield
    _lib.check(L.dt_debug_set(8, 0))


@pytest.mark.parametrize("H,W,seed", SHAPES + [(700, 900, 6)])
def test_float64_coloured_rounds(coloured_rounds, H, W, seed):
    dem = rough_f64(H, W, seed)
    fdr, filled = _check64(dem, 10.0)
    a_fdr, a_filled, st = _async64(dem, 10.0, 60)
    assert st == 0
    assert np.array_equal(a_fdr, fdr) and np.array_equal(a_filled, filled)


def _same_as_float32(dem, px):
    """float64 conditioning of float32-exact heights is the float32 tier's, bit for bit (filled as values)"""
    from descriptools_amd import flowdir
    d32 = np.asarray(dem, np.float32)
    f32, w32 = flowdir.d8_conditioned(d32, px, return_filled=True)
    f64, w64 = flowdir.d8_conditioned(d32.astype(np.float64), px, return_filled=True, heights="float64")
    assert np.array_equal(f64, f32), "%d codes differ" % int((f64 != f32).sum())
    assert w64.dtype == np.float64 and np.array_equal(w64, w32.astype(np.float64))
    return f64


@pytest.mark.parametrize("n", [(300, 417), (2048, 2048)])
def test_integer_heights_equal_the_float32_tier_on_rough_terrain(n):
    from test_gpu_hydro import _rough
    _same_as_float32(_rough(n[0], n[1], 7), 10.0)


def test_integer_heights_equal_the_float32_tier_on_the_serpentine_and_the_spiral():
    """the DEMs of test_gpu_hydro's serpentine depression and spiral flat, built as those tests build them"""
    from test_gpu_hydro import _serpentine
    H = W = 192
    dem = np.full((H, W), 500.0, np.float32)
    chan, order = _serpentine(H, W)
    n = len(order)
    for k, (y, x) in enumerate(order):
        dem[y, x] = 10.0 + 0.01 * k - (3.0 if k % 7 == 3 else 0.0)
    ye, xe = order[-1]
    dem[ye:, xe] = np.minimum(dem[ye:, xe], 10.0 + 0.01 * n)
    _same_as_float32(dem, 10.0)
    spiral = np.full((H, W), 500.0, np.float32)
    spiral[chan] = 100.0
    spiral[ye + 1:, xe] = 50.0
    _same_as_float32(spiral, 10.0)


def test_integer_heights_equal_the_float32_tier_on_the_example():
    _same_as_float32(load_example()[0], 12.5)


def test_example_with_a_float64_perturbation():
    """the Example DEM (2178 x 1534: W not a multiple of 4, nor of 2 tiles) plus k * 1e-6, below float32's resolution
    at its heights: equals the rank construction"""
    dem = load_example()[0].astype(np.float64)
    rng = np.random.default_rng(12)
    valid = dem != -100
    dem[valid] += rng.integers(0, 4, int(valid.sum())) * 1e-6
    assert dem.shape == (2178, 1534)
    _check64(dem, 12.5)


def test_async_budget():
    """dt_dev_condition_d8_f64_async: the synchronous result when the budget suffices; one round sets NOT_CONVERGED,
    and reading the status clears it"""
    from descriptools_amd import _lib, flowdir
    from descriptools_amd.device import Context
    H, W, px = 300, 417, 10.0
    dem = rough_f64(H, W, 7)
    fdr, filled = flowdir.d8_conditioned(dem, px, return_filled=True, heights="float64")
    a_fdr, a_filled, st = _async64(dem, px, 64)
    assert st == 0 and np.array_equal(a_fdr, fdr) and np.array_equal(a_filled, filled)
    L = _lib.lib()
    ctx = Context()
    d, f, c = ctx.to_device(dem), ctx.empty((H, W), np.float64), ctx.empty((H, W), np.uint8)
    _lib.check(L.dt_dev_condition_d8_f64_async(ctx.h, d.ptr, H, W, px, f.ptr, c.ptr, 1))
    with pytest.raises(RuntimeError, match="NOT_CONVERGED"):
        ctx.raise_on_status()
    assert ctx.status() == 0
    info = (C.c_int32 * 3)()
    _lib.check(L.dt_dev_condition_d8_f64(ctx.h, d.ptr, H, W, px, f.ptr, c.ptr, info))
    assert info[0] == 0 and info[1] > 1 and info[2] > 1
    assert np.array_equal(c.to_host(), fdr) and np.array_equal(f.to_host(), filled)
    for b in (d, f, c):
        b.free()
    ctx.close()


def test_run_host_conditions_float64_heights():
    """run_host(heights="auto", condition=True) on a float64 DEM: the codes are d8_conditioned's in float64, and every
    other raster is the resident recipe's -- a Chain(heights="float64", external_fdr=True) fed those codes"""
    from descriptools_amd import chain, flowdir
    from test_gpu_chain_f64 import chain_once
    H, W, px = 384, 512, 10.0
    dem = rough_f64(H, W, 9)
    out = chain.run_host(dem, px, heights="auto", condition=True)
    fdr = flowdir.d8_conditioned(dem, px, heights="float64")
    assert np.array_equal(out["fdr"], fdr)
    ref = chain_once(dem, px, "float64", fdr=fdr)
    assert set(out) == set(ref)
    assert out["hand"].dtype == np.float64
    for k in ref:
        assert np.array_equal(out[k], ref[k].astype(out[k].dtype), equal_nan=True), k
    with pytest.raises(RuntimeError, match="NOT_CONVERGED"):
        chain.run_host(dem, px, heights="float64", condition=True, condition_rounds=1)
