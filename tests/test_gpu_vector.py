"""GPU (-m gpu): vector.rasterize / mask / burn (dt_rasterize, dt_dev_rasterize, k_vr_* in dt_vector.hip) against
tests/_vector_ref.py, every comparison on the int32 bits, shape and dtype included.  The cases are those of
tests/_vector_cases.py: rasters of 70 x 130 unless stated; trivial shapes; a triangle, a concave polygon, holes, an
overlapping multipolygon, a bow-tie; vertices on cell centres, edges on centre lines; a ring of zero area; overlapping
features with scrambled ids, ids up to 2^30; a 60-triangle tessellation; geometry outside, partly outside and with
vertices at +-10^12; the empty geometry; a comb of 10,000 teeth whose 20,000 crossings per row take the sort through
global memory; 3,000 small polygons and a 20,000-vertex star on 1500 x 2300.  Lines in all octants at both
connectivities, a segment from -10^12 to 10^12, a 5,000-vertex random walk; points on corners and outside.
all_touched, the device tier against the host tier, a capacity one short of the count, guard bands around the label and
around the key scratch, burn, and two recipes end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import _vector_cases as K
import _vector_ref as R

pytestmark = pytest.mark.gpu

KIND = {"polygon": 0, "line": 1, "point": 2}


def _G(case):
    from descriptools_amd import vector
    return vector.Geometry(*case[:4])


@functools.lru_cache(maxsize=None)
def _ref(group, name, connectivity=8, all_touched=False):
    case = {"polygon": K.polygon_cases, "line": K.line_cases, "point": K.point_cases}[group]()[name]
    out = R.rasterize(*case, connectivity=connectivity, all_touched=all_touched)
    out.setflags(write=False)
    return out


# ---- polygons -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.polygon_cases()))
def test_polygons(name):
    from descriptools_amd import vector
    case = K.polygon_cases()[name]
    got, info = vector.rasterize(_G(case), case[4], return_info=True)
    R.same(name, got, _ref("polygon", name))
    assert (info["crossings"], info["largest_row"]) == R.count(*case), name
    assert info["slow_rows"] == 0 and info["overflow"] == 0
    if name.startswith("outside") or name == "empty":
        assert (got == -1).all()
    elif name != "zero area":
        assert (got >= 0).any()


def test_tessellation_labels_every_covered_cell_once():
    from descriptools_amd import vector
    rings, (x0, y0, x1, y1) = K.tessellation()
    case = K.polygon_cases()["tessellation"]
    H, W = case[4]
    lab = vector.rasterize(_G(case), case[4])
    cover = np.zeros((H, W), np.int64)
    for k, ring in enumerate(rings):
        m = vector.mask(_G(K.geom("polygon", [ring], [0])), (H, W))
        assert m.dtype == np.uint8 and (lab[m == 1] == case[3][k]).all()
        cover += m
    yc, xc = np.mgrid[0:H, 0:W] + 0.5
    inside = (xc >= x0) & (xc < x1) & (yc >= y0) & (yc < y1)
    assert np.array_equal(cover, inside.astype(np.int64)) and np.array_equal(lab >= 0, inside)


def test_largest_id_wins_in_any_order():
    from descriptools_amd import vector
    kind, coords, parts, ids, shape = K.polygon_cases()["five overlapping"]
    want = _ref("polygon", "five overlapping")
    order = [3, 1, 4, 0, 2]
    rings = [coords[parts[k]:parts[k + 1]] for k in order]
    R.same("reordered", vector.rasterize(_G(K.geom(kind, rings, ids[order])), shape), want)


def test_slow_sort_path_is_taken_and_reported():
    """20,000 crossings on every one of 40 rows: more than the 8,192 keys of a row that fit LDS, so every row is sorted
    in global memory, and info says so"""
    from descriptools_amd import vector
    case = K.comb_case()
    want = R.rasterize(*case)
    got, info = vector.rasterize(_G(case), case[4], return_info=True)
    R.same("comb", got, want)
    assert info == {"crossings": 40 * 20000, "largest_row": 20000, "slow_rows": 40, "overflow": 0}
    assert 0 < (got == 7).sum() < got.size // 2
    # 3,000 teeth: 6,000 crossings per row fit the large LDS kernel, 400 teeth the small one
    for teeth in (3000, 400):
        case = K.comb_case(teeth)
        got, info = vector.rasterize(_G(case), case[4], return_info=True)
        R.same("comb %d" % teeth, got, R.rasterize(*case))
        assert info == {"crossings": 80 * teeth, "largest_row": 2 * teeth, "slow_rows": 0, "overflow": 0}


@functools.lru_cache(maxsize=None)
def _large_ref():
    out = R.rasterize(*K.large_case())
    out.setflags(write=False)
    return out


def test_many_small_polygons_beside_a_large_star():
    from descriptools_amd import vector
    case = K.large_case()
    got, info = vector.rasterize(_G(case), case[4], return_info=True)
    R.same("large", got, _large_ref())
    assert (info["crossings"], info["largest_row"]) == R.count(*case) and info["overflow"] == 0
    assert info["largest_row"] > 1024 and (got == 0).sum() > 100000 and len(np.unique(got)) > 2500


# ---- lines and points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(K.line_cases()))
def test_lines(name, connectivity):
    from descriptools_amd import vector
    case = K.line_cases()[name]
    got, info = vector.rasterize(_G(case), case[4], connectivity, return_info=True)
    R.same("%s at %d" % (name, connectivity), got, _ref("line", name, connectivity))
    assert info == {"crossings": 0, "largest_row": 0, "slow_rows": 0, "overflow": 0}
    if name == "far segment":
        assert (got == 1).sum() >= 60 and (got == 3).sum() >= 70


@pytest.mark.parametrize("name", list(K.point_cases()))
def test_points(name):
    from descriptools_amd import vector
    case = K.point_cases()[name]
    R.same(name, vector.rasterize(_G(case), case[4]), _ref("point", name))


@pytest.mark.parametrize("name", ["concave", "two holes", "partly outside", "far vertices", "on centres"])
def test_all_touched_is_interior_and_connectivity_4_boundary(name):
    from descriptools_amd import vector
    case = K.polygon_cases()[name]
    kind, coords, parts, ids, shape = case
    rings = [list(map(tuple, coords[parts[k]:parts[k + 1]])) for k in range(len(ids))]
    closed = K.geom("line", [r + [r[0]] for r in rings], ids)
    inner = vector.rasterize(_G(case), shape)
    edge = vector.rasterize(_G(closed), shape, connectivity=4)
    for conn in (4, 8):
        got = vector.rasterize(_G(case), shape, connectivity=conn, all_touched=True)
        R.same(name, got, np.maximum(inner, edge))
        R.same(name + " reference", got, _ref("polygon", name, conn, True))


# ---- tiers and plumbing ---------------------------------------------------------------------------------------------------
def _dev(ctx, case, connectivity=8, all_touched=False, capacity=None):
    """dt_dev_rasterize on device arrays -> (label, info)"""
    from descriptools_amd import _lib
    kind, coords, parts, ids, (H, W) = case
    if capacity is None:
        capacity = R.count(*case)[0]
    arrays = [ctx.to_device(coords), ctx.to_device(parts), ctx.to_device(ids), ctx.empty((H, W), np.int32),
              ctx.empty((4,), np.int64)]
    try:
        _lib.check(_lib.lib().dt_dev_rasterize(ctx.h, KIND[kind], arrays[0].ptr, arrays[1].ptr, arrays[2].ptr, len(ids),
                                               len(coords), H, W, connectivity, int(all_touched), capacity,
                                               arrays[3].ptr, arrays[4].ptr))
        return arrays[3].to_host(), arrays[4].to_host().tolist()
    finally:
        for a in arrays:
            a.free()


def test_device_tier_equals_the_host_tier():
    from descriptools_amd import _lib, vector
    from descriptools_amd.device import Context
    ctx = Context()
    try:
        for case, kw in ((K.polygon_cases()["two holes"], {}), (K.polygon_cases()["far vertices"], {"all_touched": True}),
                         (K.large_case(), {}), (K.line_cases()["random walk"], {"connectivity": 4}),
                         (K.line_cases()["octants"], {}), (K.point_cases()["points"], {})):
            host, info = vector.rasterize(_G(case), case[4], return_info=True, **kw)
            got, dinfo = _dev(ctx, case, **kw)
            R.same("device tier", got, host)
            assert dinfo == [info["crossings"], info["largest_row"], info["slow_rows"], 0]
        # more capacity than crossings changes nothing
        case = K.polygon_cases()["concave"]
        R.same("roomy", _dev(ctx, case, capacity=R.count(*case)[0] + 1000)[0], _ref("polygon", "concave"))
        assert ctx.status() == 0
        L = _lib.lib()
        assert L.dt_dev_rasterize(ctx.h, 0, None, None, None, 1, 3, 4, 4, 8, 0, 10, None, None) == -1
        assert L.dt_last_error() == b"invalid argument: NULL label or info"
        assert L.dt_dev_rasterize(ctx.h, 0, None, None, None, 1, 3, 4, 4, 6, 0, 10, None, None) == -1
        assert L.dt_last_error() == b"invalid argument: connectivity must be 4 or 8"
        assert L.dt_dev_rasterize(ctx.h, 0, None, None, None, 1, 3, 4, 4, 8, 0, -1, None, None) == -1
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["concave", "tessellation"])
def test_capacity_one_short_leaves_the_label_empty_and_says_so(name):
    from descriptools_amd.device import Context
    case = K.polygon_cases()[name]
    total, largest = R.count(*case)
    ctx = Context()
    try:
        for touched in (False, True):
            got, info = _dev(ctx, case, all_touched=touched, capacity=total - 1)
            assert got.dtype == np.int32 and (got == -1).all()
            assert info == [total, largest, 0, 1]
        got, info = _dev(ctx, case, capacity=0)
        assert (got == -1).all() and info == [total, largest, 0, 1]
        got, info = _dev(ctx, case, capacity=total)
        R.same("exact capacity", got, _ref("polygon", name))
        assert info == [total, largest, 0, 0] and ctx.status() == 0
    finally:
        ctx.close()


GUARD = 4096


@pytest.mark.parametrize("group, name, kw", [("polygon", "partly outside", {}), ("polygon", "far vertices", {"all_touched": 1}),
                                             ("polygon", "trivial 1x200", {}), ("line", "far segment", {"connectivity": 4}),
                                             ("line", "random walk", {}), ("point", "points", {})])
def test_c_entry_writes_nothing_outside_label(group, name, kw):
    from descriptools_amd import _lib
    case = {"polygon": K.polygon_cases, "line": K.line_cases, "point": K.point_cases}[group]()[name]
    kind, coords, parts, ids, (H, W) = case
    raw = np.full(2 * GUARD + 4 * H * W, 0xA5, np.uint8)
    label = raw[GUARD:raw.size - GUARD].view(np.int32).reshape(H, W)
    conn, touched = kw.get("connectivity", 8), kw.get("all_touched", 0)
    _lib.check(_lib.lib().dt_rasterize(KIND[kind], _lib.ptr(coords, _lib.c_f64p), _lib.ptr(parts, _lib.c_i64p),
                                       _lib.ptr(ids, _lib.c_i32p), len(ids), H, W, conn, touched,
                                       _lib.ptr(label, _lib.c_i32p), None))
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    R.same(name, label, _ref(group, name, conn, bool(touched)))


@pytest.mark.parametrize("name", ["partly outside", "far vertices", "tessellation"])
def test_device_tier_writes_nothing_outside_its_scratch(name):
    """The context's scratch holds 4 H bytes of row counters and 8 bytes per crossing, each rounded up to 256.  Grown by
    a roomy call and filled with a pattern, then used by a call with the exact capacity: the pad after the counters and
    everything after the last key keep the pattern."""
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    case = K.polygon_cases()[name]
    H, W = case[4]
    total = R.count(*case)[0]
    L = _lib.lib()
    ctx = Context()
    try:
        _dev(ctx, case, capacity=total + 4096)
        nbytes, base = L.dt_ctx_scratch_bytes(ctx.h), L.dt_ctx_scratch_ptr(ctx.h)
        rows_end, keys_at = 4 * H, (4 * H + 255) // 256 * 256
        keys_end = keys_at + 8 * total
        assert base and nbytes >= keys_end + 8 * 4096 and rows_end < keys_at
        pattern = np.full(nbytes, 0xA5, np.uint8)
        _lib.check(L.dt_dev_h2d(ctx.h, base, pattern.ctypes.data_as(C.c_void_p), nbytes))
        got, info = _dev(ctx, case, all_touched=True, capacity=total)
        assert L.dt_ctx_scratch_ptr(ctx.h) == base and L.dt_ctx_scratch_bytes(ctx.h) == nbytes
        after = np.empty(nbytes, np.uint8)
        _lib.check(L.dt_dev_d2h(ctx.h, after.ctypes.data_as(C.c_void_p), base, nbytes))
        assert (after[rows_end:keys_at] == 0xA5).all(), "the pad between the row counters and the keys"
        assert (after[keys_end:] == 0xA5).all(), "past the last key"
        # the counters hold the rows' ends after the emit, the last of them the total
        assert after[:rows_end].view(np.uint32)[-1] == total
        R.same(name, got, _ref("polygon", name, 8, True))
        assert info[0] == total and info[3] == 0
    finally:
        ctx.close()


def test_burn_is_values_of_label_with_fill():
    from descriptools_amd import vector
    case = K.polygon_cases()["five overlapping"]
    lab = _ref("polygon", "five overlapping")
    for values, fill in ((np.array([1.5, -2.0, 7.25, 0.0, 9.0], np.float32), np.float32(-100.0)),
                         (np.array([10, 20, 30, 40, 50], np.int64), -7), (np.array([0.5, 1.5, 2.5], np.float64), np.nan)):
        got = vector.burn(_G(case), case[4], values, fill)
        ok = (lab >= 0) & (lab < len(values))
        want = np.where(ok, values[np.where(ok, lab, 0)], fill).astype(values.dtype)
        assert got.dtype == values.dtype and got.shape == lab.shape
        assert np.array_equal(got, want, equal_nan=True)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_rasterised_river_feeds_flow_hand_index():
    import oracle
    from descriptools_amd import flowdir, flowhand, vector
    H, W, px = 96, 128, 10.0
    dem = oracle.synth_dem(11, H, W)
    fdr = flowdir.d8_conditioned(dem, px)
    line = vector.Geometry("line", [(3.2, 90.4), (40.7, 60.3), (70.1, 55.8), (125.6, 8.9), (60.2, 20.4), (70.1, 55.8)], [0, 4, 6], [0, 1])
    river = vector.mask(line, (H, W))
    R.same("river", river, (R.rasterize("line", line.coords, line.parts, line.ids, (H, W)) >= 0).astype(np.uint8))
    assert 150 < river.sum() < 400
    fdist, idx, hand = flowhand.flow_hand_index(dem, fdr, river, px)
    on = river == 1
    assert fdist.shape == (H, W) and (fdist[on] == 0).all() and (hand[on] == 0).all()
    assert np.array_equal(idx[on], np.flatnonzero(on))
    drained = idx >= 0
    assert drained.sum() > on.sum() and on.ravel()[idx[drained]].all(), "every index names a rasterised river cell"


def test_connectivity_4_ring_holds_water():
    """A closed ring at connectivity 4 as a nodata wall: no water outside, exactly.  (The thin ring of the same vertices
    is 8-connected, which still separates 4-neighbour faces; what it does not stop is a diagonal step -- D8, cost
    distance at connectivity 8 -- and the 4-connected wall stops that too.)"""
    import oracle
    from descriptools_amd import inundation, vector
    H, W, px = 64, 64, 10.0
    dem = oracle.synth_dem(7, H, W)
    diamond = [(32.3, 6.4), (57.6, 31.7), (31.8, 58.2), (6.7, 32.4)]
    inside = vector.mask(vector.Geometry("polygon", diamond, [0, 4], [0]), (H, W)) == 1
    ring = vector.Geometry("line", diamond + diamond[:1], [0, 5], [0])
    diagonal_steps = {}
    for conn in (4, 8):
        wall = vector.mask(ring, (H, W), connectivity=conn) == 1
        pond, outside = inside & ~wall, ~inside & ~wall
        assert pond.sum() > 800
        diagonal_steps[conn] = int((pond[:-1, :-1] & outside[1:, 1:]).sum() + (pond[1:, 1:] & outside[:-1, :-1]).sum() +
                                   (pond[:-1, 1:] & outside[1:, :-1]).sum() + (pond[1:, :-1] & outside[:-1, 1:]).sum())
        res = inundation.simulate(np.where(wall, np.float32(-100.0), dem), px, 600.0, depth=np.where(pond, 5.0, 0.0))
        assert res.info["steps"] > 10 and (res.depth[pond] >= 0).all() and res.depth[pond].sum() > 0
        assert not np.array_equal(res.depth[pond], np.full(pond.sum(), 5.0)), "the water moved"
        if conn == 4:
            assert float(res.depth[outside].sum()) == 0.0, "a 4-connected wall has no face through it"
    assert diagonal_steps[4] == 0 and diagonal_steps[8] > 20
