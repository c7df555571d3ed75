"""GPU (-m gpu): the flood-map evaluation layer -- evaluation.minMaxScale / binary_map / avaliacao / calibration, the
device entries behind them, evaluate_resident and tiling.evaluate_rank -- against the numpy reference in
tests/_evaluation_ref.py, at the sizes where each mechanism can go wrong (one cell, the wave and block boundaries, exactly
4096 blocks, the grid-stride second trip and its ragged tail) and at the edges the goldens leave out: a valid first cell
shared with many cells, float16 / float32 / float64 descriptors with cells exactly on thresholds, NaN and infinities, every
threshold count of the 24-way kernel.  Every kernel here is exact, so every assertion is equality; every test first asserts
that the edge it is for occurs in its input."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from conftest import golden

import _evaluation_ref as R

pytestmark = pytest.mark.gpu

CAP = 4096 * 256                      # cells one trip of the capped grids covers
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, CAP, CAP + 257, 2 * CAP + 1]
SENTINEL = -0x0123456789ABCDEF
c_f64p = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ev():
    from descriptools_amd import _lib, evaluation
    assert _lib.lib().dt_device_count() >= 1, "no GPU visible: the HIP path cannot run"
    return evaluation


@pytest.fixture(scope="module")
def L():
    from descriptools_amd import _lib
    return _lib.lib()


@pytest.fixture()
def ctx():
    from descriptools_amd.device import Context
    c = Context()
    yield c
    c.close()


def check(rc):
    from descriptools_amd import _lib
    _lib.check(rc)


# ---- inputs, made once ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _uniform(n, seed):
    u = np.random.default_rng(seed).random(n)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def raw_raster(n, dtype, first):
    """a HAND-like raster of n cells: heights 0 .. 128 (so that 32, 64 and 96 scale to 0.25, 0.5, 0.75 exactly), a
    fifth of the cells 0 (river), nodata -100, NaN where the dtype has one; first cell NaN / nodata / a river cell"""
    dtype = np.dtype(dtype)
    u, w = _uniform(n, 1), _uniform(n, 2)
    raw = np.floor(u * 1024) / 8 if dtype.kind == "f" else np.floor(u * 129)
    raw = np.where(w < 0.2, 0, np.where(w < 0.25, -100, raw)).astype(dtype)
    if dtype.kind == "f":
        raw[(w >= 0.25) & (w < 0.27)] = np.nan
    if n > 3:
        raw[1:4] = (0, 1, 128)           # the extremes do not depend on the draw
    raw[0] = {"nan": np.nan if dtype.kind == "f" else -100, "nodata": -100, "valid": 0}[first]
    raw.setflags(write=False)
    return raw


def extremes_of(raw):
    e = R.extremes(raw)
    return e[1], e[2]


@functools.lru_cache(maxsize=None)
def descriptor(n, dtype, first):
    """the reference's scaling of raw_raster with cells planted exactly on thresholds (k / 100 for every k and random
    k / 10000, rounded to the descriptor's dtype as numpy rounds the thresholds it compares with), +-inf and NaN"""
    raw = raw_raster(n, dtype, first)
    if n < 8:
        desc = np.asarray([raw[0] / 128, 0.25, 0.5, 0.0, 0.75, 0.3, 1.0][:n]).astype(R.scale(raw, 0, 1, -100).dtype)
        desc.setflags(write=False)
        return desc
    mn, mx = extremes_of(raw)
    desc = R.scale(raw, mn, mx, -100)
    w = _uniform(n, 3)
    rng = np.random.default_rng(4)
    plant = np.flatnonzero((w < 0.3) & (np.arange(n) > 3))
    k = np.where(rng.random(plant.size) < 0.5, rng.integers(0, 101, plant.size) * 100, rng.integers(0, 10001, plant.size))
    desc[plant] = (k / 10000).astype(desc.dtype)
    odd = np.flatnonzero((w >= 0.3) & (w < 0.33) & (np.arange(n) > 3))
    desc[odd] = np.resize(np.array([np.inf, -np.inf, np.nan], desc.dtype), odd.size)
    desc[4:7] = (0.25, 0.5, 0.75)
    desc.setflags(write=False)
    return desc


@functools.lru_cache(maxsize=None)
def benchmark(n, dtype, first, direction, extra=False):
    """benchmark map {-100, 0, 1}: the descriptor's flooded side of 0.37 / 0.63 with a tenth of the cells flipped;
    extra: also 2, -1 and 3"""
    desc, w = descriptor(n, dtype, first), _uniform(n, 5)
    with np.errstate(invalid="ignore"):
        wet = (desc <= 0.37) if direction == "under" else (desc >= 0.63)
    flood = (wet ^ (w < 0.1)).astype(np.int8)
    flood[(w >= 0.1) & (w < 0.15)] = -100
    if extra:
        sel = np.flatnonzero((w >= 0.15) & (w < 0.21))
        flood[sel] = np.resize(np.array([2, -1, 3], np.int8), sel.size)
    flood.setflags(write=False)
    return flood


@functools.lru_cache(maxsize=None)
def reference_search(n, dtype, first, under):
    """(threshold, thresholds visited) of the reference's search; every direction but 'under' is one direction"""
    direction = "under" if under else "over"
    fit_at, asked = R.fit_of(descriptor(n, dtype, first), benchmark(n, dtype, first, direction), direction), []
    return R.search(lambda t: (asked.append(t), fit_at(t))[1]), tuple(asked)


# ---- host drop-ins ---------------------------------------------------------------------------------------------------
DTYPES = ["int16", "float32", "float64", "float16"]


@pytest.mark.parametrize("n", [257, CAP + 257])
@pytest.mark.parametrize("first", ["nan", "nodata", "valid"])
@pytest.mark.parametrize("direction", ["under", "over", "sideways"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_dropins_equal_reference(ev, dtype, direction, first, n):
    raw = raw_raster(n, dtype, first).reshape(1, n)
    mn, mx = extremes_of(raw)
    want_scaled = R.scale(raw, mn, mx, -100)
    got_scaled = ev.minMaxScale(raw.copy(), mn, mx, -100)
    assert np.isnan(want_scaled).sum() > n // 50 and want_scaled.dtype == (raw.dtype if raw.dtype.kind == "f" else np.float64)
    assert R.same(got_scaled, want_scaled)

    desc = descriptor(n, dtype, first).reshape(1, n)
    flood = benchmark(n, dtype, first, direction).reshape(1, n)
    th, asked = reference_search(n, dtype, first, direction == "under")
    on_threshold = np.isin(desc, np.asarray(asked).astype(desc.dtype))
    assert on_threshold.sum() > (1000 if n > CAP else 0), "cells exactly on thresholds the search visits"
    assert np.isinf(desc).sum() > 2 and np.isnan(desc).sum() > 2
    if first == "valid":
        assert desc[0, 0] == 0 and (desc == 0).sum() > n // 10, "the first cell is valid and shared"
    else:
        assert np.isnan(desc[0, 0])
    fl = flood.copy()
    assert ev.calibration(desc.copy(), fl, direction) == th
    assert R.same(fl, R.remap(flood)), "calibration leaves the benchmark map remapped"
    for t in (th, 0.25, 0.5, float(asked[7])):
        want = R.binary_map(desc, t, direction)
        if first == "valid":
            assert want[desc == 0].sum() == 0
        assert n < CAP or t == th or (desc == np.asarray(t).astype(desc.dtype)).sum() > 0
        assert R.same(ev.binary_map(desc.copy(), t, direction), want), t
    binary = R.binary_map(desc, th, direction)
    klass, counts = R.class_map(binary, flood)
    assert counts.min() > 0, "every class occurs"
    fl = flood.copy()
    c, f, cm = ev.avaliacao(binary.copy(), fl)
    assert R.same(cm, klass) and R.same(fl, R.remap(flood))
    assert (c, f) == R.indexes(counts)


def test_first_cell_rule_changes_the_answer():
    """the 'valid' rasters are no vacuous case: without the first-cell rule their maps would differ"""
    n = CAP + 257
    desc = descriptor(n, "float32", "valid")
    with np.errstate(invalid="ignore"):
        assert ((desc <= 0.37).astype(np.int64) != R.binary_map(desc, 0.37, "under")).sum() > n // 10


@pytest.mark.parametrize("n", [257, CAP + 257])
@pytest.mark.parametrize("dtype", ["float16", "float32", "float64", "int16"])
def test_minmaxscale_scalars_and_degenerate_ranges(ev, dtype, n):
    raw = raw_raster(n, dtype, "valid").copy()
    if raw.dtype.kind == "f":
        raw[5:8] = (np.inf, -np.inf, np.nan)
    tiny = np.float16(6e-8)   # a float16 denormal
    cases = [(0, 128, -100), (1.5, 100.25, -100), (7, 7, -100), (0, 0, -100), (0.1, 128.3, np.nan), (0, 128, 0.1),
             (np.float64(0.5), np.float64(99.5), -100), (np.float32(1), np.float32(3), -100.0),
             (np.float16(0), np.float16(128), np.float16(-100)), (np.int16(1), np.int16(128), -100),
             (tiny, 1e6, -100), (-65504, 65504, 0),
             # Python numbers are subtracted from each other in double before they meet the raster
             (0.37, 91.13, -100), (0.7, 259.3, -100),
             # the difference in the raster's dtype, the quotient in the wider one
             (0.1, np.float64(128.3), -100), (np.float32(0.1), 77.7, -100), (np.float64(0.3), 77, -100)]
    assert np.float32(91.13) - np.float32(0.37) != np.float32(91.13 - 0.37)
    assert np.float16(128.3) - np.float16(0.1) != np.float16(128.3 - 0.1)
    dtypes = set()
    for mn, mx, nodata in cases:
        want = R.scale(raw, mn, mx, nodata)
        got = ev.minMaxScale(raw.copy(), mn, mx, nodata)
        assert R.same(got, want), (mn, mx, nodata, got[:8], want[:8])
        dtypes.add(want.dtype)
        if float(mn) == float(mx):
            assert np.isinf(want).sum() > n // 4 and np.isnan(want).sum() > 0, "x / 0 and 0 / 0 as numpy gives them"
    if dtype == "float32":
        assert R.scale(raw, np.float64(0.5), np.float64(99.5), -100).dtype == np.float64
    assert dtypes == {"float16": {np.dtype(t) for t in (np.float16, np.float32, np.float64)},
                      "float32": {np.dtype(t) for t in (np.float32, np.float64)}}.get(dtype, {np.dtype(np.float64)})


@pytest.mark.parametrize("n", SIZES)
def test_binary_map_and_classes_at_every_size(ev, n):
    """the size sweep of k_classify through the drop-ins: float32 descriptor, valid first cell"""
    desc = descriptor(n, "float32", "valid").reshape(1, n)
    flood = benchmark(n, "float32", "valid", "under").reshape(1, n)
    want = R.binary_map(desc, 0.5, "under")
    assert R.same(ev.binary_map(desc.copy(), 0.5, "under"), want)
    assert want.reshape(-1)[0] == 0 and (n < 3 or want.sum() > 0) and (n < 8 or (desc == 0.5).sum() > 0)
    fl = flood.copy()
    c, f, cm = ev.avaliacao(want.copy(), fl)
    klass, counts = R.class_map(want, flood)
    assert R.same(cm, klass) and R.same(fl, R.remap(flood))
    assert np.array_equal([c, f], R.indexes(counts), equal_nan=True)


@pytest.mark.parametrize("bdtype", [np.int8, np.int64])
def test_avaliacao_remaps_in_place_and_counts_by_value(ev, bdtype):
    n = CAP + 257
    desc = descriptor(n, "float64", "valid").reshape(1, n)
    binary = R.binary_map(desc, 0.4, "under")
    # benchmark values {-100, 0, 1}: the indexes
    flood = benchmark(n, "float64", "valid", "under").reshape(1, n).astype(bdtype)
    assert set(np.unique(flood)) == {-100, 0, 1}
    klass, counts = R.class_map(binary, flood)
    fl = flood.copy()
    c, f, cm = ev.avaliacao(binary.copy(), fl)
    assert fl.dtype == bdtype and R.same(fl, R.remap(flood)) and not np.array_equal(fl, flood)
    assert R.same(cm, klass) and (c, f) == R.indexes(counts) and counts.min() > 0
    # a map that also holds 2, -1 and 3: the class map and the counts by value
    flood = benchmark(n, "float64", "valid", "under", extra=True).reshape(1, n).astype(bdtype)
    assert set(np.unique(flood)) == {-100, -1, 0, 1, 2, 3}
    klass, counts = R.class_map(binary, flood)
    assert klass.min() == -1 and klass.max() == 4, "sums outside 0..3 occur"
    fl = flood.copy()
    _, _, cm = ev.avaliacao(binary.copy(), fl)
    assert R.same(cm, klass) and R.same(fl, R.remap(flood))
    assert np.array_equal(np.bincount(np.clip(cm.reshape(-1), -1, 4) + 1, minlength=6)[1:5], counts)


def _edge_cases():
    g = golden("eval_edge")
    return {str(n): {k[len(n) + 1:]: g[k] for k in g.files if k.startswith(str(n) + "_")} for n in g["names"]}


@pytest.mark.parametrize("name", list(_edge_cases()))
def test_edge_golden_through_the_dropins(ev, name):
    c = _edge_cases()[name]
    under, flood = str(c["under"]), c["flood"]
    desc = ev.minMaxScale(c["raw"], c["mn"][()], c["mx"][()], -100)
    assert R.same(desc, c["desc"])
    fl = flood.copy()
    if "error" in c:
        with pytest.raises(UnboundLocalError):
            ev.calibration(desc, fl, under)
        return
    th = ev.calibration(desc, fl, under)
    assert th == float(c["th"]) and np.array_equal(fl, c["flood_after"])
    binary = ev.binary_map(desc, th, under)
    assert binary.dtype == np.int64 and np.array_equal(binary, c["binary"])
    fl = flood.copy()
    cor, fit, cm = ev.avaliacao(binary, fl)
    assert np.array_equal(cm, c["class"]) and np.array_equal(fl, c["flood_after"])
    assert np.array_equal([cor, fit], [float(c["c"]), float(c["f"])], equal_nan=True)


# ---- device entries --------------------------------------------------------------------------------------------------
def dev_extremes(L, ctx, x):
    x = np.ascontiguousarray(x, np.float32)
    d_x, d_e = ctx.to_device(x if x.size else np.zeros(1, np.float32)), ctx.to_device(np.full(3, 77.0, np.float32))
    try:
        check(L.dt_dev_unique_extremes_f32(ctx.h, d_x.ptr, x.size, d_e.ptr))
        return d_e.to_host()
    finally:
        d_x.free()
        d_e.free()


DENORMAL = np.float32(1e-45)
SPECIAL = {
    "negative values": [-3.5, -100, 2, -0.25, -3.5, -1e30],
    "only negative values": [-2, -7.5, -1e-3, -7.5],
    "both infinities": [5, np.inf, -np.inf, 0, np.nan],
    "-inf and one value": [-np.inf, 3, -np.inf],
    "inf only": [np.inf, np.inf],
    "-0.0 beside +0.0": [0.0, -0.0, 0.0, -0.0, 4],
    "-0.0 beside +0.0, nothing else": [-0.0, 0.0],
    "denormals": [DENORMAL, -DENORMAL, 0.0, 1e-40, -1e-40, 2 * DENORMAL],
    "all equal": [2.5] * 700,
    "all NaN": [np.nan] * 700,
    "N = 0": [],
    "N = 1": [-6.0],
    "N = 1, NaN": [np.nan],
    "N = 2": [9.0, -9.0],
    "N = 2, equal": [9.0, 9.0],
    "N = 2, one NaN": [np.nan, 1.0],
}


@pytest.mark.parametrize("name", list(SPECIAL))
def test_extremes_special_values(L, ctx, name):
    x = np.asarray(SPECIAL[name], np.float32)
    want = R.extremes(x)
    got = dev_extremes(L, ctx, x)
    assert R.same(got, want), (got, want)
    if name == "denormals":
        assert want[0] == -1e-40 and want[1] == -DENORMAL and 0 < abs(float(want[1])) < np.finfo(np.float32).tiny
    if name.startswith("-0.0"):
        assert want[0] == 0 and (np.isnan(want[1]) or want[1] == 4), "the two zeros are one value"


@pytest.mark.parametrize("n", SIZES)
def test_extremes_at_every_size(L, ctx, n):
    x = raw_raster(n, "float32", "nodata") - np.float32(30)   # negative and positive values, NaN, -130 many times
    want = R.extremes(x)
    assert n < 255 or (np.isnan(x).sum() > 0 and (x == want[0]).sum() > 1 and want[0] < want[1] < 0)
    assert R.same(dev_extremes(L, ctx, x), want)


PLACES = [0, 2 * CAP, 63, 64, CAP + 300, CAP - 1, CAP, 255, 256]


@pytest.mark.parametrize("turn", range(len(PLACES)))
def test_extremes_wherever_they_sit(L, ctx, turn):
    """minimum, second and maximum planted one cell each at the first cell, the last, a wave boundary, a block boundary,
    the last cell of the first grid-stride trip, the first of the second and beyond"""
    n = 2 * CAP + 1
    x = (10 + 10 * _uniform(n, 6)).astype(np.float32)
    x[::1000] = np.nan
    at = [PLACES[(turn + k) % len(PLACES)] for k in range(3)]
    x[at] = (-7.25, -7.0, 31.5)
    assert max(at) >= CAP or turn in (6, 7)   # (two turns keep all three inside the first trip)
    assert R.same(dev_extremes(L, ctx, x), np.array([-7.25, -7.0, 31.5], np.float32))
    assert R.same(R.extremes(x), np.array([-7.25, -7.0, 31.5], np.float32))


def test_extremes_second_trip_only_and_repeated_minimum(L, ctx):
    n = 2 * CAP + 1
    x = np.full(n, 5.0, np.float32)
    x[CAP + 7], x[2 * CAP], x[CAP + 64] = -1.0, -0.5, 6.0     # all three beyond the first trip
    assert R.same(dev_extremes(L, ctx, x), np.array([-1.0, -0.5, 6.0], np.float32))
    x = (1 + _uniform(n, 7)).astype(np.float32)
    x[::1777] = -100.0                                        # the minimum in every block's reach, over a thousand times
    assert (x == -100).sum() > 1000
    assert R.same(dev_extremes(L, ctx, x), R.extremes(x))


def test_extremes_after_a_larger_call_and_on_a_fresh_context(L):
    """the scratch words of the call are initialised by the call: what a larger earlier op left there does not count"""
    from descriptools_amd.device import Context
    big = (100 * _uniform(2 * CAP + 1, 8) - 300).astype(np.float32)    # extremes far below the small raster's
    small = np.asarray([4, np.nan, 2, 9, 2], np.float32)
    used = Context()
    try:
        assert R.same(dev_extremes(L, used, big), R.extremes(big))
        d_d, d_f = used.to_device(big.astype(np.float64)), used.to_device(np.ones(big.size, np.int8))
        d_c = used.empty(4, np.int64)
        check(L.dt_dev_classify(used.h, d_d.ptr, d_f.ptr, big.size, np.nan, -250.0, 1, 0, None, None, d_c.ptr))
        for b in (d_d, d_f, d_c):
            b.free()
        assert R.same(dev_extremes(L, used, small), R.extremes(small))
    finally:
        used.close()
    fresh = Context()
    try:
        assert R.same(dev_extremes(L, fresh, small), np.array([2, 4, 9], np.float32))
    finally:
        fresh.close()


@pytest.mark.parametrize("n", [1, 257, CAP + 257])
def test_device_scaling_entries(L, ctx, n):
    x = raw_raster(n, "float32", "valid").copy()
    if n > 8:
        x[5:8] = (np.inf, -np.inf, np.nan)
        x[8:] += np.float32(0.3)    # float32 heights that are no short binary fractions: the rounding is visible
    d_x, d_o = ctx.to_device(x), ctx.empty(n, np.float64)
    try:
        for mn, mx, nodata in [(0.3, 128.3, -99.7), (1.0, 1.0, -99.7), (2.5, 77.0, np.nan)]:
            mn, mx, nodata = np.float32(mn), np.float32(mx), np.float32(nodata)
            check(L.dt_dev_minmax_scale_f32(ctx.h, d_x.ptr, n, mn, mx, nodata, d_o.ptr))
            want32 = R.scale(x, mn, mx, nodata)
            assert want32.dtype == np.float32 and R.same(d_o.to_host(), want32.astype(np.float64))
            check(L.dt_dev_minmax_scale_f32_f64(ctx.h, d_x.ptr, n, float(mn), float(mx), float(nodata), d_o.ptr))
            want64 = R.scale(x.astype(np.float64), float(mn), float(mx), float(nodata))
            assert R.same(d_o.to_host(), want64)
            if n > CAP and mn != mx:
                assert (want64 != want32).sum() > n // 4, "float32 and float64 arithmetic differ on this raster"
                assert np.isnan(want64).sum() > n // 50
    finally:
        d_x.free()
        d_o.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_c_entry_with_both_scalars_in_the_rasters_type(L, dtype):
    """dt_minmax_scale, the C entry that takes mn and mx: numpy with both scalars of the raster's dtype"""
    n = CAP + 257
    x = raw_raster(n, dtype.__name__, "valid") + dtype(0.3)
    out = np.empty_like(x)
    for mn, mx in [(0.37, 91.13), (0.7, 259.3), (5.0, 5.0)]:
        check(L.dt_minmax_scale(x.ctypes.data_as(C.c_void_p), int(dtype == np.float32), n, mn, mx, -99.7,
                                out.ctypes.data_as(C.c_void_p)))
        want = R.scale(x, dtype(mn), dtype(mx), dtype(-99.7))
        assert np.isnan(want).sum() > n // 50 and R.same(out, want)


def _thresholds(nth):
    return np.ascontiguousarray(np.linspace(0.02, 0.94, 24)[:nth] if nth <= 24 else np.linspace(0.01, 0.99, nth))


def _ref_counts(desc, flood, nodata, th, under):
    """counts by value at every threshold; the nodata value is given, not read from the first cell"""
    with np.errstate(invalid="ignore"):
        live = np.where(desc == nodata, np.nan, desc)
        side = np.less_equal if under else np.greater_equal
        g = R.remap(flood).astype(np.int64)
        return np.array([R._counts(side(live, t) + g) for t in th], np.int64)


@pytest.mark.parametrize("under", [1, 0])
@pytest.mark.parametrize("nth", [1, 23, 24])
def test_dev_confusion_multi_threshold_counts(L, ctx, nth, under):
    n = CAP + 257
    desc = descriptor(n, "float64", "valid")
    flood = benchmark(n, "float64", "valid", "under", extra=(nth == 23))
    th = _thresholds(nth)
    th[0] = 0.25                                   # a threshold many cells equal
    assert (desc == 0.25).sum() > 100 and (desc == 0.0).sum() > n // 10
    want = _ref_counts(desc, flood, 0.0, th, under)
    assert want.min() > 0 and (nth == 1 or (want[0] != want[-1]).all())
    d_d, d_f = ctx.to_device(desc), ctx.to_device(flood)
    d_c = ctx.to_device(np.full(96, SENTINEL, np.int64))
    try:
        check(L.dt_dev_confusion_multi(ctx.h, d_d.ptr, d_f.ptr, n, 0.0, th.ctypes.data_as(c_f64p), nth, under, d_c.ptr))
        got = d_c.to_host()
        assert np.array_equal(got[:4 * nth].reshape(nth, 4), want)
        assert (got[4 * nth:] == SENTINEL).all(), "slots from 4 * nth on are not touched"
        assert np.array_equal(d_f.to_host(), flood), "the benchmark map is read only"
    finally:
        for b in (d_d, d_f, d_c):
            b.free()


@pytest.mark.parametrize("nth", [0, 25])
def test_dev_confusion_multi_refuses_other_counts(L, ctx, nth):
    n = 257
    d_d, d_f = ctx.to_device(descriptor(n, "float64", "valid")), ctx.to_device(benchmark(n, "float64", "valid", "under"))
    d_c = ctx.to_device(np.full(104, SENTINEL, np.int64))
    th = _thresholds(25)
    try:
        rc = L.dt_dev_confusion_multi(ctx.h, d_d.ptr, d_f.ptr, n, 0.0, th.ctypes.data_as(c_f64p), nth, 1, d_c.ptr)
        assert rc == -1, "DT_EINVAL"
        ctx.sync()
        assert (d_c.to_host() == SENTINEL).all(), "a refused call launches nothing"
    finally:
        for b in (d_d, d_f, d_c):
            b.free()


@pytest.mark.parametrize("nth", [25, 48, 49])
def test_host_confusion_multi_passes(L, nth):
    from descriptools_amd._lib import c_i8p, c_i64p, ptr
    n = CAP + 257
    desc, flood = descriptor(n, "float64", "valid"), benchmark(n, "float64", "valid", "over")
    th = _thresholds(nth)
    counts = np.full(4 * nth + 8, SENTINEL, np.int64)
    check(L.dt_confusion_multi(ptr(desc, c_f64p), ptr(flood, c_i8p), n, 0.0, th.ctypes.data_as(c_f64p), nth, 0,
                               ptr(counts, c_i64p)))
    want = _ref_counts(desc, flood, 0.0, th, 0)
    assert want.min() > 0 and len({tuple(r) for r in want}) == nth, "every threshold its own counts"
    assert np.array_equal(counts[:4 * nth].reshape(nth, 4), want) and (counts[4 * nth:] == SENTINEL).all()


@pytest.mark.parametrize("n", [257, 2 * CAP + 1])
@pytest.mark.parametrize("outputs", range(8))
def test_dev_classify_every_output_combination(L, ctx, outputs, n):
    want_binary, want_klass, remap = bool(outputs & 1), bool(outputs & 2), bool(outputs & 4)
    desc = descriptor(n, "float64", "valid")
    flood = benchmark(n, "float64", "valid", "under", extra=True)
    th, under = 0.25, outputs & 1
    binary = _ref_binary = (np.less_equal if under else np.greater_equal)(np.where(desc == 0.0, np.nan, desc), th)
    klass, counts = R.class_map(binary.astype(np.int64), flood)
    assert (desc == th).sum() > 0 and counts.min() > 0 and not np.array_equal(R.remap(flood), flood)
    d_d, d_f, d_c = ctx.to_device(desc), ctx.to_device(flood), ctx.to_device(np.full(8, SENTINEL, np.int64))
    d_b, d_k = ctx.to_device(np.full(n, 9, np.uint8)), ctx.to_device(np.full(n, 9, np.int32))
    try:
        check(L.dt_dev_classify(ctx.h, d_d.ptr, d_f.ptr, n, 0.0, th, under, int(remap),
                                d_b.ptr if want_binary else None, d_k.ptr if want_klass else None, d_c.ptr))
        got = d_c.to_host()
        assert np.array_equal(got[:4], counts) and (got[4:] == SENTINEL).all()
        assert np.array_equal(d_f.to_host(), R.remap(flood) if remap else flood), "remapped only when asked to"
        assert np.array_equal(d_b.to_host(), _ref_binary.astype(np.uint8) if want_binary else np.full(n, 9, np.uint8))
        assert np.array_equal(d_k.to_host(), klass.astype(np.int32) if want_klass else np.full(n, 9, np.int32))
    finally:
        for b in (d_d, d_f, d_c, d_b, d_k):
            b.free()


# ---- evaluate_resident against the reference's host pipeline --------------------------------------------------------
def reference_pipeline(raw, flood, under):
    """Example/example.py:113-147 in the reference's terms, with the NaN rule of the extremes"""
    mn, mx = extremes_of(raw)
    desc = R.scale(raw, mn, mx, -100)
    th = R.calibrate(desc, flood, under)
    binary = R.binary_map(desc, th, under)
    klass, counts = R.class_map(binary, flood)
    return {"mn": float(mn), "mx": float(mx), "desc": desc, "threshold": th, "binary": binary, "klass": klass,
            "counts": counts, "indexes": R.indexes(counts)}


def _agrees(res, want):
    assert (res["mn"], res["mx"], res["threshold"]) == (want["mn"], want["mx"], want["threshold"])
    assert np.array_equal(res["counts"], want["counts"])
    assert (res["correctness"], res["fit"]) == want["indexes"]


@functools.lru_cache(maxsize=None)
def hand_and_flood(n, first, kind):
    """kind 'int': integer heights (the example's int16 HAND); 'real': float32 heights with fractions"""
    raw = raw_raster(n, "int16" if kind == "int" else "float32", first)
    if kind == "real":
        raw = np.where((raw > 0) & (np.arange(n) > 3), raw + np.float32(0.3), raw).astype(np.float32)
    with np.errstate(invalid="ignore"):
        wet = (raw >= 0) & (raw <= 40)
    flood = (wet ^ (_uniform(n, 9) < 0.1)).astype(np.int8)
    flood[_uniform(n, 10) < 0.05] = -100
    return raw, flood


@pytest.mark.parametrize("first", ["nodata", "valid"])
@pytest.mark.parametrize("n", [257, CAP + 257])
def test_evaluate_resident_integer_valued_equals_reference_on_int16(ev, ctx, n, first):
    raw, flood = hand_and_flood(n, first, "int")
    want = reference_pipeline(raw.reshape(1, n), flood.reshape(1, n), "under")
    assert want["desc"].dtype == np.float64 and want["counts"].min() > 0
    assert (first == "valid") == (want["desc"][0, 0] == 0.0)
    d_h, d_f = ctx.to_device(raw.astype(np.float32)), ctx.to_device(flood)
    d_b, d_k = ctx.empty(n, np.uint8), ctx.empty(n, np.int32)
    try:
        _agrees(ev.evaluate_resident(ctx, d_h.ptr, d_f.ptr, n, "under", integer_valued=True), want)
        assert np.array_equal(d_f.to_host(), flood)
        res = ev.evaluate_resident(ctx, d_h.ptr, d_f.ptr, n, "under", integer_valued=True, binary_ptr=d_b.ptr,
                                   class_ptr=d_k.ptr, remap_flood=True)
        _agrees(res, want)
        assert np.array_equal(d_b.to_host(), want["binary"].reshape(-1))
        assert np.array_equal(d_k.to_host(), want["klass"].reshape(-1))
        assert np.array_equal(d_f.to_host(), R.remap(flood)) and not np.array_equal(flood, R.remap(flood))
    finally:
        for b in (d_h, d_f, d_b, d_k):
            b.free()


@pytest.mark.parametrize("under", ["under", "over"])
@pytest.mark.parametrize("first", ["nan", "nodata", "valid"])
def test_evaluate_resident_float32_equals_reference(ev, ctx, first, under):
    n = CAP + 257
    raw, flood = hand_and_flood(n, first, "real")
    want = reference_pipeline(raw.reshape(1, n), flood.reshape(1, n), under)
    assert want["desc"].dtype == np.float32 and want["counts"].min() > 0 and np.isnan(raw).sum() > 1000
    if first == "valid":
        assert want["desc"][0, 0] == 0.0 and (want["desc"] == 0.0).sum() > n // 10
        assert want["binary"][want["desc"] == 0.0].sum() == 0, "every river cell drops out of the map"
    d_h, d_f, d_k = ctx.to_device(raw), ctx.to_device(flood), ctx.empty(n, np.int32)
    try:
        _agrees(ev.evaluate_resident(ctx, d_h.ptr, d_f.ptr, n, under, class_ptr=d_k.ptr), want)
        assert np.array_equal(d_k.to_host(), want["klass"].reshape(-1)) and np.array_equal(d_f.to_host(), flood)
    finally:
        for b in (d_h, d_f, d_k):
            b.free()


def test_evaluate_resident_nodata_first_constant_and_callable(ev, ctx):
    """the tail of a raster whose first cell (a river cell) lies on another rank: the scaled value of that cell comes in
    as a constant or from a callable evaluated after the extremes are known"""
    n, cut = CAP + 257, 1000
    raw, flood = hand_and_flood(n, "valid", "real")
    tail, tail_flood = raw[cut:], flood[cut:]
    mn, mx = extremes_of(tail)
    assert raw[0] == 0 and tail[0] > 0 and (tail == 0).sum() > n // 10 and mn == 0
    desc = R.scale(tail, mn, mx, -100)
    first_scaled = float((raw[0] - mn) / (mx - mn))
    th = R.search(lambda t: R.indexes(_ref_counts(desc, tail_flood, first_scaled, [t], 1)[0])[1])
    counts = _ref_counts(desc, tail_flood, first_scaled, [th], 1)[0]
    own = _ref_counts(desc, tail_flood, float(desc[0]), [th], 1)[0]
    assert not np.array_equal(counts, own), "the rank's own first cell would give other counts"
    d_h, d_f = ctx.to_device(tail), ctx.to_device(tail_flood)
    calls = []
    try:
        for first in (first_scaled, lambda: (calls.append(1), first_scaled)[1]):
            res = ev.evaluate_resident(ctx, d_h.ptr, d_f.ptr, tail.size, "under", nodata_first=first)
            assert res["threshold"] == th and np.array_equal(res["counts"], counts)
        assert calls == [1]
    finally:
        d_h.free()
        d_f.free()


class _Cells:
    """the little of a device tensor tiling.evaluate_rank touches, over a device.DeviceArray"""

    def __init__(self, arr, shape, dtype, first=None):
        self.arr, self.shape, self.dtype, self._first = arr, shape, dtype, first

    def data_ptr(self):
        return self.arr.ptr.value

    def contiguous(self):
        return self

    def is_contiguous(self):
        return True

    def __getitem__(self, at):
        assert at == (0, 0)
        return np.float32(self._first)


class _FlatTile:
    """what tiling.evaluate_rank reads of a RankTile, for one flat chunk of a raster (no torch: the rasters are
    device.DeviceArrays, `torch` is this object)"""
    wide, dev, int8, int32 = False, None, np.int8, np.int32

    def __init__(self, ctx, chunk, start):
        self.ctx, self.torch = ctx, self
        self.H, self.W, self.gy0, self.gx0 = 1, chunk.size, 0, start
        self._x = _Cells(ctx.to_device(chunk), (1, chunk.size), np.float32, chunk[0])

    def on_stream(self):
        import contextlib
        return contextlib.nullcontext()

    def core(self, name):
        return self._x

    def empty(self, shape, dtype, device):
        return _Cells(self.ctx.empty(shape[0] * shape[1], dtype), shape, dtype)


def test_evaluate_rank_four_uneven_chunks(ev):
    """the first-cell-valid raster as four uneven flat chunks, every logical rank in its own thread: every rank finds the
    single raster's threshold, the summed counts are the reference's, and only the owner of the first cell knows it"""
    from descriptools_amd import tiling
    from descriptools_amd.device import Context
    n = 2 * CAP + 1
    raw, flood = hand_and_flood(n, "valid", "real")
    want = reference_pipeline(raw.reshape(1, n), flood.reshape(1, n), "under")
    cuts = [0, 257, 257 + 64, CAP // 2 + int(np.flatnonzero(raw[CAP // 2:] > 0)[0]), n]   # the last chunk: two trips
    assert n - cuts[3] > CAP and want["desc"][0, 0] == 0.0 and want["binary"][want["desc"] == 0.0].sum() == 0
    tiles, floods = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        tiles.append(_FlatTile(Context(), raw[a:b], a))
        floods.append(_Cells(tiles[-1].ctx.to_device(flood[a:b]), (1, b - a), np.int8))
        assert a == 0 or raw[a] > 0, "the other chunks start on cells that are not the global first cell's value"
    comms = tiling.LocalComm.create(4)
    results, errors = [None] * 4, []

    def work(r):
        try:
            results[r] = tiling.evaluate_rank(tiles[r], floods[r], comms[r], class_map=True)
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append(e)
            comms[r].sh.barrier.abort()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for res in results:
        _agrees(res, want)
    got = np.concatenate([res["class_map"].arr.to_host() for res in results])
    assert np.array_equal(got, want["klass"].reshape(-1))
    assert [t.gx0 == 0 for t in tiles] == [True, False, False, False]
    for t in tiles:
        t.ctx.close()
