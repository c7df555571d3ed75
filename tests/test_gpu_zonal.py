"""GPU (-m gpu): zonal statistics (zonal.py, dt_zonal_*, the device tier; k_zn_* in dt_zonal.hip) against the pure-numpy
reference (tests/_zonal_ref.py), bit for bit and for every table entry, zone, label and painted cell -- the derived
floats too, since the float stage is the same numpy association on identical integers.  No tolerances anywhere.

Shapes are chosen where the kernels can go wrong (1 x 1, one row, one column, W % 4 != 0 with partial tiles on both axes,
whole aligned tiles, a strided view), zonings where the LDS table can (one zone, half the cells without one, stripes
that change zone inside a lane's run, blocks that straddle four tiles, a zone per cell, real regions), and every parity
case runs with the LDS table at its default, capped at 1 and 3 slots and absent (DT_DBG_RC_SLOTS)."""
import ctypes as C

import numpy as np
import pytest

import _zonal_ref as Z

pytestmark = pytest.mark.gpu

DT_STATUS_BAD_HEIGHT = 64
DT_STATUS_ZONE_RANGE = 128
DT_DBG_RC_SLOTS = 10
DT_SCAN_CHUNK = 2048
SLOTS = [0, 1, 3, -1]
SHAPES = [(1, 1), (1, 257), (257, 1), (67, 131), (128, 192), (130, 257)]


def _same(name, g, r):
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    if g.tobytes() != r.tobytes():
        bad = np.argwhere(~((g == r) | ((g != g) & (r != r))))
        i = tuple(bad[0]) if len(bad) else None
        raise AssertionError("%s: %d entries differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i] if i else None, r[i] if i else None))


class slots:
    """DT_DBG_RC_SLOTS for the block, restored at its end"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from descriptools_amd import _lib
        _lib.check(_lib.lib().dt_debug_set(DT_DBG_RC_SLOTS, self.n))

    def __exit__(self, *exc):
        from descriptools_amd import _lib
        _lib.check(_lib.lib().dt_debug_set(DT_DBG_RC_SLOTS, 0))


def strided(a):
    """a as a strided view of a larger array (the product makes it contiguous)"""
    big = np.zeros((a.shape[0] * 2, a.shape[1] * 3), a.dtype)
    big[::2, ::3] = a
    v = big[::2, ::3]
    assert not v.flags.c_contiguous or a.size <= 1
    return v


def zonings(H, W, rng):
    """name -> (zones, n_zones)"""
    yy, xx = np.mgrid[0:H, 0:W]
    nbx = (W + 17) // 64 + 1
    half = np.where(rng.random((H, W)) < 0.5, 0, -100)
    out = {"one": (np.zeros((H, W)), 1), "half": (half, 1), "stripes3": (xx // 3, (W + 2) // 3),
           "blocks": (((yy + 31) // 64) * nbx + (xx + 17) // 64, ((H + 31) // 64 + 1) * nbx)}
    if (H, W) == (67, 131):
        out["cells"] = (rng.permutation(H * W).reshape(H, W), H * W)
    return {k: (np.ascontiguousarray(z, np.int32), n) for k, (z, n) in out.items()}


def values(H, W, rng, dtype):
    """finite values from -60 to 940 with NaN, +-inf and -100 cells, and -0.0 beside +0.0"""
    v = (rng.random((H, W)) * 1000 - 60).astype(dtype)
    r = rng.random((H, W))
    v[r < 0.04] = np.nan
    v[(r >= 0.04) & (r < 0.06)] = np.inf
    v[(r >= 0.06) & (r < 0.08)] = -np.inf
    v[(r >= 0.08) & (r < 0.12)] = -100.0
    if W >= 2:
        v[0, 0], v[0, 1] = -0.0, 0.0
    return v


def check_tables(zones, v, nz, nodata=-100.0, frac_bits=None, origin=None):
    """tables with every accumulator and statistics with every output against the reference; returns the tables"""
    from descriptools_amd import zonal
    t = zonal.tables(zones, v, nz, frac_bits=frac_bits, origin=origin, nodata=nodata)
    o, s = Z.default_scale(zones, v, nz, nodata, frac_bits, origin)
    assert (t.origin, t.frac_bits) == (o, s)
    r = Z.tables(zones, v, nz, o, s, nodata)
    assert r["out"] == 0
    for name, g in (("count", t.count), ("s1", t.s1), ("s2_lo", t.s2_lo), ("s2_hi", t.s2_hi), ("vmin", t.vmin),
                    ("vmax", t.vmax)):
        _same(name, g, r[name])
    st = zonal.statistics(zones, v, nz, zonal.OUTPUTS, frac_bits=frac_bits, origin=origin, nodata=nodata)
    ref = Z.statistics(r, o, s)
    assert list(st) == list(zonal.OUTPUTS)
    for name in zonal.OUTPUTS:
        _same(name, st[name], ref[name])
    return t


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_slots", SLOTS)
def test_tables_parity(n_slots, dtype):
    """every shape x zoning, in both LDS modes, with capped slots and without the LDS table"""
    rng = np.random.default_rng(11)
    overflowed = 0
    for H, W in SHAPES:
        v = values(H, W, rng, dtype)
        for k, (name, (zones, nz)) in enumerate(sorted(zonings(H, W, rng).items())):
            if n_slots > 0 and name in ("stripes3", "cells") and H >= 67 and W >= 131:
                assert Z.ids_per_tile(zones, nz) > n_slots   # the capped table overflows: the fall-through path runs
                overflowed += 1
            zz, vv = (strided(zones), strided(v)) if (H, W) == (130, 257) else (zones, v)
            with slots(n_slots):
                # nodata and None alternate; every second case has its origin inside the values: negative q
                check_tables(zz, vv, nz, nodata=None if k % 2 else -100.0, origin=300.5 if k % 2 else None)
    assert n_slots <= 0 or overflowed >= 4
    # the two sides of the threshold between the direct and the claimed LDS table
    z = (np.arange(64 * 64, dtype=np.int32) % 256).reshape(64, 64)
    with slots(n_slots):
        check_tables(z, values(64, 64, rng, dtype), 256)            # direct, all slots in use
        check_tables(z + 1, values(64, 64, rng, dtype), 257)        # claimed: 257 zones, 64 slots


@pytest.mark.parametrize("shape", [(1, 140001), (2200 * 64, 3)])
def test_more_tiles_than_workgroups(shape):
    """a launch with a direct LDS table has at most 2048 workgroups, each taking tile after tile: rasters of more
    tiles than that, in both table modes"""
    from descriptools_amd import zonal
    H, W = shape
    assert ((H + 63) // 64) * ((W + 63) // 64) > 2048
    rng = np.random.default_rng(31)
    v = values(H, W, rng, np.float32)
    classes = rng.integers(-1, 10, (H, W)).astype(np.int32)
    for zones, nz in ((classes, 10), (np.zeros((H, W), np.int32), 1), ((classes + 1) * 40, 401)):
        check_tables(zones, v, nz)
    edges = np.linspace(-60, 940, 8)
    _same("histogram", zonal.histogram(classes, v, 10, edges), Z.histogram(classes, v, 10, edges))
    b = (v > 300).astype(np.int32)
    _same("crosstab", zonal.crosstab(classes, b, 10, 2), Z.crosstab(classes, b, 10, 2))
    wide = (classes + 1) * 40                            # 401 rows of 64 columns: beyond the direct table
    _same("crosstab, claimed", zonal.crosstab(wide, b, 401, 64), Z.crosstab(wide, b, 401, 64))


def test_minus_zero_and_empty_zones():
    from descriptools_amd import zonal
    zones = np.array([[0, 0, 2, -100, 2]], np.int32)
    for dtype in (np.float32, np.float64):
        v = np.array([[-0.0, 0.0, 5.0, 1.0, np.nan]], dtype)
        t = check_tables(zones, v, 4)
        assert t.count.tolist() == [2, 0, 1, 0]
        assert t.vmin[0] == 0 and not np.signbit(t.vmin[0]) and not np.signbit(t.vmax[0])
        assert np.isnan(t.vmin[1]) and np.isnan(t.vmax[3])
        v = np.array([[0.0, -0.0, 5.0, 1.0, np.nan]], dtype)       # the other order
        assert not np.signbit(check_tables(zones, v, 4).vmin[0])
    only = zonal.tables(zones, v, 4, want=("s1", "max"))
    assert only.count is None and only.s2_lo is None and only.vmin is None and only.s1 is not None
    _same("vmax", only.vmax, Z.tables(zones, v, 4, only.origin, only.frac_bits)["vmax"])
    empty = zonal.tables(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.float32), 3)
    assert empty.count.tolist() == [0, 0, 0] and np.isnan(empty.vmin).all() and np.isnan(empty.vmax).all()
    assert zonal.tables(zones, v, 4, want=("count",)).count.tolist() == [2, 0, 1, 0]
    none = zonal.tables(np.full((3, 3), -100, np.int32), np.ones((3, 3)), 0)
    assert none.count.size == 0 and none.vmax.dtype == np.float64


def test_quantisation_bound():
    """|q| = 2^31 - 1 is within the contract; 2^31 raises DT_STATUS_BAD_HEIGHT, is left out, and fails the host call"""
    from descriptools_amd import _lib, device, zonal
    L = _lib.lib()
    top = float(2 ** 31 - 1)
    zones = np.zeros((2, 4), np.int32)
    v = np.array([[top, -top, 1.0, 2.0], [3.0, 4.0, 5.0, 6.0]], np.float64)
    t = check_tables(zones, v, 1, frac_bits=0, origin=0.0)
    assert int(t.s2_hi[0]) * 2 ** 32 + int(t.s2_lo[0]) == 2 * (2 ** 31 - 1) ** 2 + 91
    over = v.copy()
    over[1, 1] = float(2 ** 31)
    with pytest.raises(ValueError, match="too fine"):
        zonal.tables(zones, over, 1, frac_bits=0, origin=0.0)
    out = [np.zeros(1, dt) for dt in (np.int64, np.int64, np.uint64, np.uint64, np.float64, np.float64)]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    args = lambda val: (zones.ctypes.data_as(_lib.c_i32p), vp(val), 8, 2, 4, 1, 0.0, 0, 1, -100.0,
                        out[0].ctypes.data_as(_lib.c_i64p), out[1].ctypes.data_as(_lib.c_i64p)) + tuple(vp(a) for a in out[2:])
    assert L.dt_zonal_tables(*args(v)) == 0
    with pytest.raises(RuntimeError, match=r"2\^31 - 1"):
        _lib.check(L.dt_zonal_tables(*args(over)))
    assert L.dt_zonal_tables(*args(v)) == 0                          # the next call starts clean
    ctx = device.Context()
    bufs = [ctx.to_device(zones), ctx.to_device(over)] + [ctx.empty(1, a.dtype) for a in out]
    try:
        assert ctx.status() == 0
        _lib.check(L.dt_dev_zonal_tables(ctx.h, bufs[0].ptr, bufs[1].ptr, 8, 2, 4, 1, 0.0, 0, 1, -100.0,
                                         *[b.ptr for b in bufs[2:]]))
        assert ctx.status() == DT_STATUS_BAD_HEIGHT
        assert ctx.status() == 0
        got = [b.to_host() for b in bufs[2:]]
    finally:
        for b in bufs:
            b.free()
        ctx.close()
    r = Z.tables(zones, over, 1, 0.0, 0)                             # the reference leaves the cell out too
    assert r["out"] == 1
    for g, name in zip(got, ("count", "s1", "s2_lo", "s2_hi", "vmin", "vmax")):
        _same(name, g, r[name])
    assert got[5][0] == top                                          # 2^31 took no part in the maximum either


@pytest.mark.parametrize("n_slots", [0, -1])
def test_sum_of_squares_passes_64_bits(n_slots):
    """300 x 300 cells of one zone with |q| close to 2^31: the sum of q^2 needs s2_hi"""
    rng = np.random.default_rng(5)
    q = (2 ** 31 - 1 - rng.integers(0, 1000, (300, 300))) * rng.choice([-1, 1], (300, 300))
    v = q.astype(np.float64)
    zones = np.zeros((300, 300), np.int32)
    ref = Z.tables(zones, v, 1, 0.0, 0)
    assert int(ref["s2"][0]) > 2 ** 64 and int(ref["s2_hi"][0]) > 2 ** 32
    with slots(n_slots):
        t = check_tables(zones, v, 1, frac_bits=0, origin=0.0)
    assert int(t.s2_hi[0]) * 2 ** 32 + int(t.s2_lo[0]) == int(ref["s2"][0])


def check_compact(labels, limit=None):
    from descriptools_amd import zonal
    got = zonal.compact(labels, limit)
    zones, labels_of = Z.compact(labels, limit)
    _same("zones", got.zones, zones)
    _same("labels_of", got.labels_of, labels_of)
    return got


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_compact(dtype, monkeypatch):
    from descriptools_amd import zonal
    rng = np.random.default_rng(7)
    limit = 32 * DT_SCAN_CHUNK * 2 + 77                 # two blocks of bitmap words and a partial third
    edge = [0, 31, 32, 63, 64, limit - 1, DT_SCAN_CHUNK - 1, DT_SCAN_CHUNK, 32 * DT_SCAN_CHUNK - 1,
            32 * DT_SCAN_CHUNK, 64 * DT_SCAN_CHUNK - 1, 64 * DT_SCAN_CHUNK, limit, limit + 5, -1, -100]
    labels = rng.choice(edge, (67, 131)).astype(dtype)
    got = check_compact(labels, limit)
    assert got.labels_of.tolist() == sorted(e for e in edge if 0 <= e < limit)
    check_compact(labels)                               # limit = the number of cells
    check_compact(labels[:1, :1], limit)
    check_compact(np.full((33, 65), 4242, dtype), 5000)                         # one label
    none = check_compact(np.full((33, 65), -100, dtype))                        # all invalid
    assert none.labels_of.size == 0 and (none.zones == -100).all()
    check_compact(np.full((5, 5), 25, dtype))                                   # the default limit itself is invalid
    every = check_compact(rng.permutation(130 * 257).reshape(130, 257).astype(dtype))   # all distinct
    assert every.labels_of.size == 130 * 257
    check_compact(strided(labels), limit)
    check_compact(np.zeros((0, 7), dtype))
    check_compact(rng.integers(0, 2 ** 31 - 1, (64, 64)).astype(dtype), 2 ** 31 - 1)   # the largest bitmap
    monkeypatch.setattr(zonal, "_ZONES_CAP", 5)         # more zones than the first call asks for: the second call runs
    assert check_compact(labels, limit).labels_of.size > 5
    monkeypatch.setattr(zonal, "_ZONES_CAP", 12)        # exactly as many
    assert check_compact(labels, limit).labels_of.size == 12


@pytest.mark.parametrize("n_slots", SLOTS)
def test_histogram(n_slots):
    from descriptools_amd import zonal
    rng = np.random.default_rng(13)
    for (H, W), K, dtype in (((67, 131), 1, np.float32), ((67, 131), 7, np.float64), ((128, 192), 1024, np.float32),
                             ((1, 257), 7, np.float32), ((130, 257), 64, np.float64)):
        edges = np.sort(rng.random(K + 1) * 900 - 50)
        assert (np.diff(edges) > 0).all()
        v = values(H, W, rng, dtype)
        flat = v.reshape(-1)
        on = edges.astype(dtype)                        # values exactly on the edges (as far as the dtype holds them)
        pos = rng.choice(flat.size, min(flat.size, 3 * on.size + 4), replace=False)
        fill = np.r_[on, on, on, np.nextafter(on[0], -np.inf), np.nextafter(on[-1], np.inf),
                     np.nextafter(edges[0], -np.inf), np.nextafter(edges[-1], np.inf)].astype(dtype)
        flat[pos] = fill[:pos.size]
        if dtype == np.float64:
            assert (v == edges[-1]).any() and (v == edges[0]).any()
        for name, (zones, nz) in sorted(zonings(H, W, rng).items()):
            if nz * K * 8 > 1 << 24:
                continue                                 # the per-cell zoning at K = 1024 is a table of 72 MB: no
            with slots(n_slots):
                _same("%s K=%d" % (name, K), zonal.histogram(zones, v, nz, edges, nodata=-100.0),
                      Z.histogram(zones, v, nz, edges))
        with slots(n_slots):
            zones, nz = zonings(H, W, rng)["stripes3"]
            _same("nodata=None", zonal.histogram(zones, v, nz, edges, nodata=None),
                  Z.histogram(zones, v, nz, edges, None))
    # the closed last edge and both open ends, by hand
    e = np.array([0.0, 1.0, 2.0])
    v = np.array([[0.0, 1.0, 2.0, -0.0, np.nextafter(2.0, 3.0), np.nextafter(0.0, -1.0), 0.5, np.nan]])
    with slots(n_slots):
        assert zonal.histogram(np.zeros((1, 8), np.int32), v, 1, e).tolist() == [[3, 2]]


@pytest.mark.parametrize("n_slots", SLOTS)
def test_crosstab(n_slots):
    from descriptools_amd import zonal
    rng = np.random.default_rng(17)
    H, W = 130, 257
    a = rng.integers(-1, 10, (H, W)).astype(np.int32)                # a 10-class raster
    a = np.where(rng.random((H, W)) < 0.7, np.sort(a, axis=1), a).astype(np.int32)   # with runs
    b = (rng.random((H, W)) < 0.4).astype(np.int32)                  # against flooded / dry
    with slots(n_slots):
        ct = zonal.crosstab(a, b, 10, 2)
        _same("crosstab", ct, Z.crosstab(a, b, 10, 2))
        _same("row sums", ct.sum(axis=1), zonal.tables(a, np.ones((H, W), np.float32), 10, want=("count",)).count)
        wide = rng.integers(-2, 1024, (67, 131)).astype(np.int32)
        wide[0, :4] = [0, 1023, 1023, -100]
        rows = (np.arange(67 * 131, dtype=np.int32) % 37).reshape(67, 131)
        _same("n_b = 1024", zonal.crosstab(rows, wide, 37, 1024), Z.crosstab(rows, wide, 37, 1024))
        _same("n_b = 1024, per cell", zonal.crosstab(wide, rows, 1024, 37), Z.crosstab(wide, rows, 1024, 37))
        _same("int64 input", zonal.crosstab(a.astype(np.int64), b.astype(np.uint8), 10, 2), ct)
    with pytest.raises(ValueError, match="n_b is 2"):
        zonal.crosstab(a, b + 1, 10, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_paint(dtype):
    from descriptools_amd import zonal
    rng = np.random.default_rng(19)
    fills = [np.nan, -100.0] if np.dtype(dtype).kind == "f" else [-100, np.iinfo(dtype).min]
    for H, W in SHAPES:
        nt = 50
        zones = rng.integers(-3, nt + 3, (H, W)).astype(np.int32)    # out of range on both sides
        if W >= 4:
            zones[0, :4] = [-100, -1, nt, 2 ** 31 - 1]
        if np.dtype(dtype).kind == "f":
            table = (rng.random(nt) * 1e6 - 5e5).astype(dtype)
            table[:3] = [np.inf, -0.0, np.nan]
        else:
            table = rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max, nt, dtype=dtype)
        for fill in fills:
            _same("paint %s" % (fill,), zonal.paint(table, zones, fill), Z.paint(table, zones, fill))
        _same("strided", zonal.paint(table, strided(zones), fills[0]), Z.paint(table, zones, fills[0]))
    _same("empty table", zonal.paint(np.zeros(0, dtype), zones, fills[1]), np.full(zones.shape, fills[1], dtype))


def test_regions_compact_statistics_paint():
    """a real case: regions.label of a random mask -> compact -> tables; painting the counts back gives the region
    size of every foreground cell"""
    from descriptools_amd import regions, zonal
    rng = np.random.default_rng(23)
    H, W = 130, 257
    mask = (rng.random((H, W)) < 0.3).astype(np.uint8)   # below the percolation threshold: thousands of regions
    lab = regions.label(mask, sizes=True)
    c = check_compact(lab.label)
    nz = c.labels_of.size
    assert nz > 64 and (c.zones >= 0).sum() == mask.sum()
    v = values(H, W, rng, np.float32)
    for n in SLOTS:
        with slots(n):
            t = check_tables(c.zones, v, nz, nodata=None)
    ones = zonal.tables(c.zones, np.ones((H, W), np.float32), nz, want=("count",))
    size = zonal.paint(ones.count, c.zones, 0)
    _same("region size", size, np.where(mask != 0, lab.size, 0))
    # a descriptor normalised by its own region
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = v / zonal.paint(zonal.statistics_from_tables(t, ("range",))["range"], c.zones, np.nan)
    assert rel.shape == (H, W) and np.isnan(rel[c.zones < 0]).all()


def test_device_tier_and_status():
    """the dt_dev_* entries on device buffers give the host tier's bits, twice; a zone id >= n_zones raises
    DT_STATUS_ZONE_RANGE and the cell is left out; the status is clean after every passing call"""
    from descriptools_amd import _lib, device, zonal
    L = _lib.lib()
    rng = np.random.default_rng(29)
    H, W, K = 67, 131, 7
    labels = (rng.integers(0, 40, (H, W)) * 97).astype(np.int64)
    labels[rng.random((H, W)) < 0.1] = -100
    v = values(H, W, rng, np.float32)
    edges = np.linspace(-60, 940, K + 1)
    host_c = zonal.compact(labels)
    nz = host_c.labels_of.size
    host_t = zonal.tables(host_c.zones, v, nz)
    host_h = zonal.histogram(host_c.zones, v, nz, edges)
    host_x = zonal.crosstab(host_c.zones, (v > 300).astype(np.int32), nz, 2)
    host_p = zonal.paint(host_t.vmax, host_c.zones, np.float32(np.nan))
    ctx = device.Context()
    bufs = []

    def dev(a):
        bufs.append(ctx.to_device(a))
        return bufs[-1]

    def new(shape, dtype, fill=0x5A):
        bufs.append(ctx.to_device(np.full(shape, fill, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype).reshape(shape)))
        return bufs[-1]

    try:
        lb_d, v_d, b_d = dev(labels), dev(v), dev((v > 300).astype(np.int32))
        runs = []
        for _ in range(2):
            z_d, lo_d, n_d = new((H, W), np.int32), dev(np.full(nz + 3, -7, np.int64)), new(1, np.int64)
            _lib.check(L.dt_dev_zonal_compact(ctx.h, lb_d.ptr, 8, H, W, H * W, z_d.ptr, lo_d.ptr, nz + 3, n_d.ptr))
            assert int(n_d.to_host()[0]) == nz
            tab = [new(nz, dt) for dt in (np.int64, np.int64, np.uint64, np.uint64, np.float32, np.float32)]
            _lib.check(L.dt_dev_zonal_tables(ctx.h, z_d.ptr, v_d.ptr, 4, H, W, nz, host_t.origin, host_t.frac_bits, 1,
                                             -100.0, *[t.ptr for t in tab]))
            h_d, x_d, p_d = new((nz, K), np.int64), new((nz, 2), np.int64), new((H, W), np.float32)
            _lib.check(L.dt_dev_zonal_counts(ctx.h, z_d.ptr, v_d.ptr, 4, H, W, nz, edges.ctypes.data_as(_lib.c_f64p), K,
                                             1, -100.0, h_d.ptr))
            _lib.check(L.dt_dev_zonal_counts(ctx.h, z_d.ptr, b_d.ptr, 0, H, W, nz, None, 2, 0, 0.0, x_d.ptr))
            fill = np.array([np.nan], np.float32)
            _lib.check(L.dt_dev_zonal_paint(ctx.h, tab[5].ptr, 4, nz, z_d.ptr, H, W, fill.ctypes.data_as(C.c_void_p),
                                            p_d.ptr))
            assert ctx.status() == 0
            runs.append([z_d.to_host(), lo_d.to_host()] + [t.to_host() for t in tab]
                        + [h_d.to_host(), x_d.to_host(), p_d.to_host()])
        for a, b in zip(runs[0], runs[1]):
            assert a.tobytes() == b.tobytes()
        zones, labels_of, count, s1, lo, hi, vmin, vmax, hist, xt, painted = runs[0]
        _same("zones", zones, host_c.zones)
        _same("labels_of", labels_of, np.r_[host_c.labels_of, [-7] * 3])      # entries from n_zones on are left alone
        for name, g, r in (("count", count, host_t.count), ("s1", s1, host_t.s1), ("s2_lo", lo, host_t.s2_lo),
                           ("s2_hi", hi, host_t.s2_hi), ("vmin", vmin, host_t.vmin), ("vmax", vmax, host_t.vmax),
                           ("histogram", hist, host_h), ("crosstab", xt, host_x), ("paint", painted, host_p)):
            _same(name, g, r)
        # only the tables that are asked for are touched
        cnt = new(nz, np.int64)
        _lib.check(L.dt_dev_zonal_tables(ctx.h, dev(host_c.zones).ptr, v_d.ptr, 4, H, W, nz, 0.0, 0, 1, -100.0, cnt.ptr,
                                         None, None, None, None, None))
        _same("count alone", cnt.to_host(), host_t.count)
        assert ctx.status() == 0
        # a zone id >= n_zones
        over = host_c.zones.copy()
        over[3, 5] = nz
        over[40, 100] = 2 ** 31 - 1
        o_d = dev(over)
        tab = [new(nz, dt) for dt in (np.int64, np.int64, np.uint64, np.uint64, np.float32, np.float32)]
        _lib.check(L.dt_dev_zonal_tables(ctx.h, o_d.ptr, v_d.ptr, 4, H, W, nz, host_t.origin, host_t.frac_bits, 1,
                                         -100.0, *[t.ptr for t in tab]))
        assert ctx.status() == DT_STATUS_ZONE_RANGE
        r = Z.tables(over, v, nz, host_t.origin, host_t.frac_bits)            # the reference leaves them out too
        for name, t in zip(("count", "s1", "s2_lo", "s2_hi", "vmin", "vmax"), tab):
            _same(name, t.to_host(), r[name])
        h_d = new((nz, K), np.int64)
        _lib.check(L.dt_dev_zonal_counts(ctx.h, o_d.ptr, v_d.ptr, 4, H, W, nz, edges.ctypes.data_as(_lib.c_f64p), K, 1,
                                         -100.0, h_d.ptr))
        assert ctx.status() == DT_STATUS_ZONE_RANGE
        _same("histogram", h_d.to_host(), Z.histogram(over, v, nz, edges))
        assert ctx.status() == 0
    finally:
        for b in bufs:
            b.free()
        ctx.close()
    # through the host tier the same raster is an error: ValueError from the maximum, RuntimeError from the library
    with pytest.raises(ValueError, match="n_zones is %d" % nz):
        zonal.tables(over, v, nz)
    out = np.zeros(nz, np.int64)
    with pytest.raises(RuntimeError, match="number of zones"):
        _lib.check(L.dt_zonal_tables(over.ctypes.data_as(_lib.c_i32p), v.ctypes.data_as(C.c_void_p), 4, H, W, nz, 0.0,
                                     0, 1, -100.0, out.ctypes.data_as(_lib.c_i64p), None, None, None, None, None))
    _same("the next call", zonal.tables(host_c.zones, v, nz).count, host_t.count)


def test_basins_of_bench_terrain():
    """2048 x 2048 synthetic terrain: the drainage basins made dense (a few hundred zones), and the regions of its
    one-metre elevation bands (thousands, the claimed LDS table); every accumulator of the heights per zone"""
    import oracle
    from descriptools_amd import flowdir, regions, watershed
    H = W = 2048
    dem = np.ascontiguousarray(oracle.synth_dem(7, H, W), np.float32)
    fdr = flowdir.d8(dem, 10.0)
    c = check_compact(watershed.basins(fdr))
    nz = c.labels_of.size
    assert nz > 1
    t = check_tables(c.zones, dem, nz)
    assert int(t.count.sum()) == int((c.zones >= 0).sum())
    bands = check_compact(regions.label(np.floor(dem) % 2 == 0, connectivity=4))
    assert bands.labels_of.size > 256
    check_tables(bands.zones, dem, bands.labels_of.size)
