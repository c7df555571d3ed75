"""GPU (-m gpu): the one-pass threshold histogram (k_threshold_hist behind dt_dev_threshold_hist / dt_threshold_hist) and
the curve functions of descriptools_amd.evaluation on top of it, against the numpy reference in tests/_curve_ref.py: at the
raster sizes where a lane tail, a workgroup's tail or the grid-stride second trip can go wrong, at every threshold count
where the kernel's layout changes (the coarse index's stride, the number of passes over bin ranges), against the 24-way
kernel it stands beside, and at the edges of the comparison itself.  Everything is integer counting, so every assertion is
equality; every test first asserts that the edge it is for occurs in its input."""
import ctypes as C
import functools

import numpy as np
import pytest

import _curve_ref as CR
import _evaluation_ref as R

pytestmark = pytest.mark.gpu

# mirrored from csrc/dt_curve.hip
TILE = 1024 * 4                 # DT_CURVE_TILE: cells of one workgroup's trip
TRIP = 256 * TILE               # DT_CURVE_GRID_MAX workgroups: cells of one trip of the whole grid
COARSE_MAX = 2048               # DT_CURVE_COARSE_MAX: the coarse index holds every threshold up to this K, every 2nd .. 32nd above
BINS_MAX = 18432                # DT_CURVE_BINS_MAX: bins per pass; K + 1 bins
K_MAX = 65535                   # DT_CURVE_K_MAX
SIDES = ("under", "over")
c_f64p, c_i8p, c_i64p = C.POINTER(C.c_double), C.POINTER(C.c_int8), C.POINTER(C.c_int64)


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


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same_curve(got, ref):
    return all(same(g, r) for g, r in zip(got, ref)) and got._fields == ref._fields


# ---- the two entries ------------------------------------------------------------------------------------------------
def dev_hist(L, ctx, desc, flood, nodata, th, under):
    K = len(th)
    bufs = [ctx.to_device(np.ascontiguousarray(desc, np.float64)), ctx.to_device(np.ascontiguousarray(flood, np.int8)),
            ctx.to_device(np.ascontiguousarray(th, np.float64)), ctx.to_device(np.full(2 * K + 3, -7, np.int64))]
    try:
        check(L.dt_dev_threshold_hist(ctx.h, bufs[0].ptr, bufs[1].ptr, len(desc), nodata, bufs[2].ptr, K,
                                      1 if under == "under" else 0, bufs[3].ptr))
        return bufs[3].to_host()
    finally:
        for b in bufs:
            b.free()


def host_hist(L, desc, flood, nodata, th, under):
    d, f, t = np.ascontiguousarray(desc, np.float64), np.ascontiguousarray(flood, np.int8), np.ascontiguousarray(th, np.float64)
    hist = np.full(2 * len(t) + 3, -7, np.int64)
    check(L.dt_threshold_hist(d.ctypes.data_as(c_f64p), f.ctypes.data_as(c_i8p), d.size, nodata, t.ctypes.data_as(c_f64p),
                              len(t), 1 if under == "under" else 0, hist.ctypes.data_as(c_i64p)))
    return hist


# ---- inputs, made once ----------------------------------------------------------------------------------------------
NODATA = 0.3125  # a valid-looking value: what a raster whose first cell is valid gives


@functools.lru_cache(maxsize=None)
def scaled(n, seed=1):
    """a scaled HAND-like float64 descriptor of n cells in 0..1: a fifth exactly 0, a fifth NODATA in runs (so that whole
    waves are dead), NaN, +-inf, cells on the lattice k / 100"""
    rng = np.random.default_rng(seed)
    d = rng.random(n)
    w = rng.random(n)
    d[w < 0.2] = 0.0
    d[(w >= 0.2) & (w < 0.4)] = np.round(d[(w >= 0.2) & (w < 0.4)] * 100) / 100
    d[(w >= 0.4) & (w < 0.43)] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0]), np.count_nonzero((w >= 0.4) & (w < 0.43)))
    runs = (np.arange(n) // 97) % 5 == 3
    d[runs] = NODATA
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def bench_map(n, seed=2):
    rng = np.random.default_rng(seed)
    b = (rng.random(n) < 0.35).astype(np.int8)
    b[rng.random(n) < 0.1] = -100
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def table(K, seed=3):
    """K sorted thresholds over -0.05 .. 1.05 with equal neighbours"""
    rng = np.random.default_rng(seed + K)
    t = np.sort(rng.random(K) * 1.1 - 0.05)
    if K > 3:
        t[K // 2] = t[K // 2 - 1]
    t.setflags(write=False)
    return t


LATTICE = np.arange(101) / 100
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, TRIP + 257, 2 * TRIP + 1]


@pytest.mark.parametrize("n", SIZES)
def test_hist_sizes_both_entries(L, ctx, n):
    d, b = scaled(n), bench_map(n)
    if n >= TILE - 1:
        assert np.isin(d, LATTICE).any() and (d == NODATA).any() and np.isnan(d).any() and (d == 0).mean() > 0.1
    for under in SIDES:
        ref = CR.hist(d, b, LATTICE, under, nodata=NODATA)
        assert ref.sum() == n and ref[-1] == 0
        assert np.array_equal(dev_hist(L, ctx, d, b, NODATA, LATTICE, under), ref), under
        assert np.array_equal(host_hist(L, d, b, NODATA, LATTICE, under), ref), under


def passes(K):
    return -(-(K + 1) // BINS_MAX)


def stride_log2(K):
    s = 0
    while -(-K // (1 << s)) > COARSE_MAX:
        s += 1
    return s


K_LIST = sorted({1, 2, 24, 25, 63, 64, 65, 10001, K_MAX,
                 COARSE_MAX - 1, COARSE_MAX, COARSE_MAX + 1,            # stride 1 | 2
                 2 * COARSE_MAX, 2 * COARSE_MAX + 1, 4 * COARSE_MAX, 4 * COARSE_MAX + 1,   # 2 | 4, 4 | 8
                 8 * COARSE_MAX, 8 * COARSE_MAX + 1, 16 * COARSE_MAX, 16 * COARSE_MAX + 1,  # 8 | 16, 16 | 32
                 BINS_MAX - 2, BINS_MAX - 1, BINS_MAX, BINS_MAX + 1,    # K + 1 = BINS_MAX bins: one pass | two
                 2 * BINS_MAX - 1, 2 * BINS_MAX, 3 * BINS_MAX - 1, 3 * BINS_MAX,   # two | three, three | four
                 K_MAX - 1})


def test_k_list_stands_on_both_sides_of_every_switch():
    assert {stride_log2(K) for K in K_LIST} == {0, 1, 2, 3, 4, 5} and {passes(K) for K in K_LIST} == {1, 2, 3, 4}
    for K in K_LIST:
        if K < K_MAX and (stride_log2(K) != stride_log2(K + 1) or passes(K) != passes(K + 1)):
            assert K + 1 in K_LIST, K
    assert stride_log2(COARSE_MAX) == 0 and stride_log2(COARSE_MAX + 1) == 1
    assert passes(BINS_MAX - 1) == 1 and passes(BINS_MAX) == 2 and passes(K_MAX) == 4


@pytest.mark.parametrize("under", SIDES)
@pytest.mark.parametrize("K", K_LIST)
def test_hist_threshold_counts(L, ctx, K, under):
    n = 70001
    th = table(K)
    d = scaled(n).copy()
    rng = np.random.default_rng(K)
    plant = rng.choice(n, n // 4, replace=False)
    d[plant] = th[rng.integers(0, K, plant.size)]       # cells exactly on thresholds, the duplicated one included
    d[plant[:16]] = th[np.resize([0, K - 1], 16)]
    b = bench_map(n)
    ref = CR.hist(d, b, th, under, nodata=NODATA)
    live = ~np.isnan(d) & (d != NODATA)
    assert n > 16 * TILE and np.isin(d[live], th).sum() > n // 8
    if K > 3:
        assert th[K // 2] == th[K // 2 - 1]
    two = ref[:K + 1] + ref[K + 1:2 * K + 2]
    for p in range(passes(K)):                              # every pass has cells to count
        assert two[p * BINS_MAX:(p + 1) * BINS_MAX].sum() > 0, p
    got = dev_hist(L, ctx, d, b, NODATA, th, under)
    assert np.array_equal(got, ref)
    if K > 3:  # equal neighbours give equal rows
        c = CR.counts_of(got, K, under)
        assert np.array_equal(c[K // 2], c[K // 2 - 1])


@pytest.mark.parametrize("K", [0, K_MAX + 1, -1])
def test_hist_refuses_other_threshold_counts(L, ctx, K):
    n = 100
    d, f = ctx.to_device(scaled(n)), ctx.to_device(bench_map(n))
    t, h = ctx.to_device(np.zeros(8)), ctx.to_device(np.full(19, -7, np.int64))
    try:
        assert L.dt_dev_threshold_hist(ctx.h, d.ptr, f.ptr, n, 0.0, t.ptr, K, 1, h.ptr) != 0
        assert b"thresholds" in L.dt_last_error()
        assert (h.to_host() == -7).all()
    finally:
        for x in (d, f, t, h):
            x.free()
    hist = np.zeros(19, np.int64)
    dd, ff, tt = np.array(scaled(n)), np.array(bench_map(n)), np.zeros(8)
    assert L.dt_threshold_hist(dd.ctypes.data_as(c_f64p), ff.ctypes.data_as(c_i8p), n, 0.0, tt.ctypes.data_as(c_f64p), K, 1,
                               hist.ctypes.data_as(c_i64p)) != 0


@pytest.mark.parametrize("th", [[0.5, 0.25], [0.1, np.nan], [np.nan], [0.0, 0.1, np.nan, 0.3]])
def test_host_entry_checks_the_table(L, th):
    n = 100
    dd, ff, tt = np.array(scaled(n)), np.array(bench_map(n)), np.array(th, np.float64)
    hist = np.zeros(2 * len(tt) + 3, np.int64)
    assert L.dt_threshold_hist(dd.ctypes.data_as(c_f64p), ff.ctypes.data_as(c_i8p), n, 0.0, tt.ctypes.data_as(c_f64p),
                               len(tt), 1, hist.ctypes.data_as(c_i64p)) != 0
    assert b"NaN" in L.dt_last_error()


# ---- old kernel against new -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("under", SIDES)
@pytest.mark.parametrize("K", [1, 7, 24])
def test_counts_equal_the_24_way_kernel_on_the_same_buffers(L, ctx, K, under):
    n = 3 * TILE + 77
    d, b = scaled(n), bench_map(n)
    th = np.ascontiguousarray(np.linspace(0, 1, K + 2)[1:-1] if K > 1 else [0.5])
    assert np.isin(d, th).any() or K == 7
    dd, df, dt = ctx.to_device(d), ctx.to_device(b), ctx.to_device(th)
    dh, dc = ctx.empty(2 * K + 3, np.int64), ctx.empty(4 * K, np.int64)
    u = 1 if under == "under" else 0
    try:
        check(L.dt_dev_confusion_multi(ctx.h, dd.ptr, df.ptr, n, NODATA, th.ctypes.data_as(c_f64p), K, u, dc.ptr))
        check(L.dt_dev_threshold_hist(ctx.h, dd.ptr, df.ptr, n, NODATA, dt.ptr, K, u, dh.ptr))
        old, hist = dc.to_host().reshape(K, 4), dh.to_host()
    finally:
        for x in (dd, df, dt, dh, dc):
            x.free()
    assert old.sum() == K * n and hist[-1] == 0
    assert np.array_equal(CR.counts_of(hist, K, under), old)


@pytest.mark.parametrize("under", SIDES)
def test_counts_equal_the_host_tier_passes_at_100_thresholds(L, under):
    n, K = 3 * TILE + 77, 100
    d, b, th = np.array(scaled(n)), np.array(bench_map(n)), np.ascontiguousarray(LATTICE[:K])
    old = np.zeros((K, 4), np.int64)
    u = 1 if under == "under" else 0
    check(L.dt_confusion_multi(d.ctypes.data_as(c_f64p), b.ctypes.data_as(c_i8p), n, NODATA, th.ctypes.data_as(c_f64p), K, u,
                               old.ctypes.data_as(c_i64p)))
    assert K > 4 * 24 and old.sum() == K * n
    assert np.array_equal(CR.counts_of(host_hist(L, d, b, NODATA, th, under), K, under), old)


# ---- the edges of the comparison ----------------------------------------------------------------------------------------
def _edge_cases():
    n = 5 * TILE + 13
    rng = np.random.default_rng(9)
    u = rng.random(n)
    mixed = (rng.random(n) < 0.4).astype(np.int8)
    mixed[::11] = -100
    th5 = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    on = th5[rng.integers(0, 5, n)]
    zeros = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    wild = np.resize(np.array([np.nan, np.inf, -np.inf, 0.5, NODATA, 0.2]), n)
    cases = {
        # name: (descriptor, benchmark, thresholds, the edge occurs)
        "cells_on_thresholds": (on, mixed, th5, np.isin(on, th5).all()),
        "duplicate_thresholds": (u, mixed, np.array([0.2, 0.5, 0.5, 0.5, 0.9]), True),
        "thresholds_below_the_data": (u + 2, mixed, th5, (u + 2).min() > th5.max()),
        "thresholds_above_the_data": (u - 2, mixed, th5, (u - 2).max() < th5.min()),
        "infinite_thresholds": (wild, mixed, np.array([-np.inf, -np.inf, 0.3, np.inf, np.inf]), np.isinf(wild).any()),
        "negative_zero_cells_positive_zero_threshold": (zeros, mixed, np.array([0.0, 1.0]), np.signbit(zeros).any()),
        "positive_zero_cells_negative_zero_threshold": (zeros, mixed, np.array([-1.0, -0.0]), (~np.signbit(zeros)).any()),
        "both_zeros_in_the_table": (zeros, mixed, np.array([0.0, -0.0, 0.0]), True),
        "nan_inf_and_nodata_cells": (wild, mixed, th5, np.isnan(wild).any() and (wild == NODATA).any()),
        "one_repeated_value": (np.full(n, 0.5), mixed, th5, True),
        "one_repeated_value_off_the_table": (np.full(n, 0.6), mixed, LATTICE, True),
        "all_dead_nodata": (np.full(n, NODATA), mixed, th5, True),
        "all_dead_nan": (np.full(n, np.nan), mixed, th5, True),
        "benchmark_all_dry": (u, np.zeros(n, np.int8), th5, True),
        "benchmark_all_flooded": (u, np.ones(n, np.int8), th5, True),
        "benchmark_all_outside": (u, np.full(n, -100, np.int8), th5, True),
    }
    return cases


EDGES = _edge_cases()


@pytest.mark.parametrize("under", SIDES)
@pytest.mark.parametrize("name", sorted(EDGES))
def test_hist_edge(L, ctx, name, under):
    d, b, th, occurs = EDGES[name]
    assert occurs and len(d) > 5 * TILE
    ref = CR.hist(d, b, th, under, nodata=NODATA)
    K = len(th)
    if name.startswith("all_dead"):
        assert ref[K if under == "under" else 0] + ref[K + 1 + (K if under == "under" else 0)] == len(d)
    if "zero" in name:  # the two zeros are one value: every cell in one bin
        assert np.count_nonzero(ref) == 2
    if name == "thresholds_below_the_data":
        assert ref[K] + ref[2 * K + 1] == len(d)
    if name == "thresholds_above_the_data":
        assert ref[0] + ref[K + 1] == len(d)
    assert ref.sum() == len(d) and ref[-1] == 0
    got = dev_hist(L, ctx, d, b, NODATA, th, under)
    assert np.array_equal(got, ref)
    # and the reference's histogram is what the single-threshold reference counts, so the kernel is held to that too
    k = K // 2
    with np.errstate(all="ignore"):
        live = np.where(d == NODATA, np.nan, d)
        wet = (live <= th[k]) if under == "under" else (live >= th[k])
    assert np.array_equal(CR.counts_of(got, K, under)[k], R.class_map(wet.astype(np.int64), b)[1])


@pytest.mark.parametrize("under", SIDES)
def test_unknown_benchmark_value_is_counted_and_refused(L, ctx, ev, under):
    n = 2 * TILE + 5
    d, b = np.array(scaled(n)), np.array(bench_map(n))
    b[5::9] = 3
    b[7::31] = -1
    nod = float(d[0])
    ref = CR.hist(d, b, LATTICE, under, nodata=nod)
    assert ref[-1] == np.count_nonzero((b == 3) | (b == -1)) > 100
    assert np.array_equal(dev_hist(L, ctx, d, b, nod, LATTICE, under), ref)
    assert np.array_equal(host_hist(L, d, b, nod, LATTICE, under), ref)
    with pytest.raises(ValueError, match="other than -100, 0 and 1"):
        ev.threshold_counts(d, b, LATTICE, under)
    with pytest.raises(ValueError, match="other than -100, 0 and 1"):
        ev.curve(d, b, under, steps=100)


# ---- the Python layer -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raster(dtype, first, n=203 * 61):
    """(scaled descriptor, benchmark map): a HAND-like raw raster of heights 0..128 (a fifth 0, nodata -100, NaN in the
    float dtypes) scaled by the reference; first cell NaN / nodata / valid; P > 0"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(11)
    u, w = rng.random(n), rng.random(n)
    raw = np.floor(u * 1024) / 8 if dtype.kind == "f" else np.floor(u * 129)
    raw = np.where(w < 0.2, 0, np.where(w < 0.25, -100, raw)).astype(dtype)
    if dtype.kind == "f":
        raw[(w >= 0.25) & (w < 0.27)] = np.nan
    raw[1:4] = (0, 1, 128)
    raw[0] = {"nan": np.nan if dtype.kind == "f" else -100, "nodata": -100, "valid": 0}[first]
    desc = R.scale(raw, 0, 128, -100)
    with np.errstate(invalid="ignore"):
        flood = ((desc <= 0.37) ^ (rng.random(n) < 0.1)).astype(np.int8)
    flood[rng.random(n) < 0.05] = -100
    desc, flood = desc.reshape(-1, 61), flood.reshape(-1, 61)
    desc.setflags(write=False)
    flood.setflags(write=False)
    return desc, flood


@pytest.mark.parametrize("under", SIDES)
@pytest.mark.parametrize("first", ["nan", "nodata", "valid"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64, np.int16])
def test_threshold_counts_and_curve(ev, dtype, first, under):
    desc, flood = raster(dtype, first)
    want = {np.float16: np.float16, np.float32: np.float32}.get(dtype, np.float64)
    assert desc.dtype == want and (flood == 1).sum() > 0
    if first == "valid":
        assert desc[0, 0] == 0 and (desc == 0).sum() > desc.size // 10
    else:
        assert np.isnan(desc[0, 0])
    steps = 200
    th = np.arange(steps + 1) / steps
    if dtype in (np.float16, np.float32):  # cells between a threshold and its rounding: the rounding decides
        r = th.astype(dtype).astype(np.float64)
        assert (r != th).any()
    assert (np.asarray(desc, np.float64).reshape(-1)[:, None] == CR.compared(desc, th)[None, ::40]).any()
    kept = flood.copy()
    ref = CR.curve(desc, flood, under, steps)
    assert np.array_equal(ev.threshold_counts(desc, flood, th, under), ref.counts)
    got = ev.curve(desc, flood, under, steps=steps)
    assert same_curve(got, ref) and 0 < got.auc < 1
    assert same_curve(ev.curve(desc, flood, under, thresholds=th[::7]), CR.curve(desc, flood, under, thresholds=th[::7]))
    assert np.array_equal(flood, kept)
    # the counts are avaliacao's on binary_map's map
    k = 74
    assert np.array_equal(got.counts[k], R.class_map(R.binary_map(desc, float(th[k]), under), flood)[1])


@pytest.mark.parametrize("objective", ["fit", "tss", "kappa"])
@pytest.mark.parametrize("under", SIDES)
def test_calibration_exhaustive_is_the_reference_argmax(ev, under, objective):
    for dtype, first in ((np.float32, "nan"), (np.int16, "valid")):
        desc, flood = raster(dtype, first)
        kept = flood.copy()
        assert ev.calibration_exhaustive(desc, flood, under, objective=objective) == CR.exhaustive(desc, flood, under, 10000, objective)
        assert ev.calibration_exhaustive(desc, flood, under, steps=37, objective=objective) == CR.exhaustive(desc, flood, under, 37, objective)
        assert np.array_equal(flood, kept)


@pytest.mark.parametrize("under", SIDES)
@pytest.mark.parametrize("dtype,first", [(np.float16, "nodata"), (np.float32, "valid"), (np.float64, "nan"), (np.int16, "nodata")])
def test_calibration_exhaustive_is_never_below_the_search(ev, dtype, first, under):
    desc, flood = raster(dtype, first)
    assert (flood == 1).sum() > 0
    fit_at = R.fit_of(desc, flood, under)
    searched = ev.calibration(desc, flood.copy(), under)
    assert searched == R.calibrate(desc, flood, under) and 0 <= searched <= 1
    assert fit_at(ev.calibration_exhaustive(desc, flood, under)) >= fit_at(searched)


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("seed", range(5))
def test_calibration_exhaustive_beats_the_search_where_it_is_out_of_reach(ev, seed, mirrored):
    u = np.random.default_rng(seed).random(4096)
    d = np.floor(u * 4096) / 4096
    d[0] = -1
    b = (((d >= 0) & (d < 0.03)) | ((d > 0.8) & (d < 0.97))).astype(np.int8)
    d, under = (1 - d, "over") if mirrored else (d, "under")
    fit_at = R.fit_of(d, b, under)
    searched, best = ev.calibration(d, b.copy(), under), ev.calibration_exhaustive(d, b, under)
    assert abs(best - searched) > 0.25
    assert fit_at(best) > fit_at(searched)


def test_calibration_exhaustive_refuses_an_objective_that_is_nan_everywhere(ev):
    d = np.linspace(-1, 1, 500)
    b = np.zeros(500, np.int8)  # no flooded benchmark cell: correctness, tss are 0 / 0 everywhere
    assert np.isnan(CR.curve(d, b, "under").tss).all()
    with pytest.raises(ValueError, match="NaN at every threshold"):
        ev.calibration_exhaustive(d, b, "under", objective="tss")


# ---- resident ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("under", SIDES)
def test_curve_resident_pieces_sum_to_the_whole(ev, ctx, under):
    n = 4 * TILE + 333
    d, b = np.array(scaled(n)), np.array(bench_map(n))
    cuts = [0, TILE + 101, 3 * TILE + 7, n]  # unequal, and the later pieces start at odd addresses
    nod = float(d[0])
    assert nod == d[0] and all((d[a:z] == nod).any() and d[a] != nod for a, z in zip(cuts[1:-1], cuts[2:]))
    th = np.arange(1001) / 1000
    dd, df = ctx.to_device(d), ctx.to_device(b)
    try:
        def piece(a, z, reduce_hist):
            return ev.curve_resident(ctx, C.c_void_p(dd.ptr.value + 8 * a), C.c_void_p(df.ptr.value + a), z - a, th, under,
                                     nod, reduce_hist=reduce_hist)
        others = []
        for a, z in zip(cuts[1:-1], cuts[2:]):
            piece(a, z, lambda h: others.append(h.copy()) or h)
        assert len(others) == 2 and all(h.dtype == np.int64 and h.sum() == z - a for h, a, z in zip(others, cuts[1:], cuts[2:]))
        summed = piece(cuts[0], cuts[1], lambda h: h + others[0] + others[1])
        whole = ev.curve_resident(ctx, dd.ptr, df.ptr, n, th, under, nod)
    finally:
        dd.free()
        df.free()
    ref = CR.curve_of(th, CR.hist(d, b, th, under, nodata=nod), under)
    assert same_curve(whole, ref) and same_curve(summed, ref)
    assert whole.counts[0].sum() == n
