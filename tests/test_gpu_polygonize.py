"""GPU (-m gpu): vector.polygonize (dt_polygonize, dt_dev_polygonize, k_pg_* in dt_polygonize.hip) against
tests/_polygonize_ref.py, every comparison on the bytes of coords, parts, ids and shell, shapes and dtypes included, and
info on the reference's counts.  The cases are those of tests/_polygonize_cases.py: trivial shapes, all background, one
label, a checkerboard, diagonal pairs, a pinched ring, nested islands and holes, holes that inherit their shell from
one another, walks of more than 64 and 128 cells, a hole and a shell that start at one vertex, a 65 x 67 spiral whose
one cycle of 4,488 edges takes 14 rounds of doubling, a staircase, labels 0 and 2^30 and negatives, noise, a 1 x 5000
strip and 600 x 900 of local relief.  The round trip through vector.rasterize is bit-exact on every case and on the
landform, catchment and flood-extent rasters of a 96 x 128 chain.  The device tier equals the host tier; every capacity
one short, and 0, leaves the outputs untouched and says what is needed; guard bands around the four outputs and around
the scratch; two calls on one context give the same bytes; the refusals and their messages."""
import ctypes as C
import functools

import numpy as np
import pytest

import _polygonize_cases as K
import _polygonize_ref as P
import _vector_ref as R

pytestmark = pytest.mark.gpu

NAMES = list(K.cases()) + ["terrain"]
INFO = ("edges", "vertices", "rings", "holes", "rounds")
GUARD = 4096


def _raster(name):
    return K.terrain() if name == "terrain" else K.cases()[name]


@functools.lru_cache(maxsize=None)
def _ref(name, background=None):
    if name.startswith("mask: "):
        raster = {n: a for n, a, _ in K.masks()}[name[6:]]
    else:
        raster = _raster(name)
    out = P.polygonize(P.normalise(raster, background))
    for a in out[:4]:
        a.setflags(write=False)
    return out


def _same(what, got, want):
    """coords, parts, ids, shell on their bytes"""
    for field, g, w in zip(("coords", "parts", "ids", "shell"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s%s, expected %s%s" % (
            what, field, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), "%s: %s differs, first at %s" % (
            what, field, np.argwhere(np.atleast_1d(g != w))[:1].tolist())


def _fields(pg):
    return pg.geometry.coords, pg.geometry.parts, pg.geometry.ids, pg.shell


@pytest.mark.parametrize("name", NAMES)
def test_cases(name):
    from descriptools_amd import vector
    raster = _raster(name)
    want = _ref(name)
    pg, info = vector.polygonize(raster, return_info=True)
    assert pg.geometry.kind == "polygon" and list(info) == list(INFO)
    _same(name, _fields(pg), want[:4])
    assert info == want[4], name
    back = vector.rasterize(pg.geometry, raster.shape)
    R.same(name + " round trip", back, np.where(raster >= 0, raster, -1).astype(np.int32))


@pytest.mark.parametrize("name, background", [(n, b) for n, _, b in K.masks()])
def test_background_value(name, background):
    from descriptools_amd import vector
    raster = {n: a for n, a, _ in K.masks()}[name]
    want = _ref("mask: " + name, background)
    pg = vector.polygonize(raster, background=background)
    _same(name, _fields(pg), want[:4])
    assert want[4]["rings"] > 0 and background not in pg.geometry.ids.tolist()
    keep = P.normalise(raster, background)
    R.same(name, vector.rasterize(pg.geometry, raster.shape), keep.astype(np.int32))


def test_round_trip_on_the_rasters_of_a_chain():
    """landforms, reach catchments and the river-connected flood extent of a 96 x 128 synthetic terrain: what the package
    itself produces comes back from rasterize(polygonize(.)) bit for bit"""
    import oracle
    from descriptools_amd import flowacc, flowdir, flowhand, horizon, reaches, regions, streams, vector
    H, W, px = 96, 128, 10.0
    dem = oracle.synth_dem(11, H, W)
    fdr = flowdir.d8_conditioned(dem, px)
    river = (flowacc.accumulate(fdr) > 60).astype(np.int8)
    _, idx, hand = flowhand.flow_hand_index(dem, fdr, river, px)
    rasters = {"landform": horizon.geomorphons(dem, px, radius=6),
               "catchment": reaches.catchments(streams.stream_network(fdr, river).link, idx).catchment,
               "extent": regions.connected((hand >= 0) & (hand <= 3.0), river == 1)}
    for name, raster in rasters.items():
        background = 0 if name == "extent" else None
        pg, info = vector.polygonize(raster, background=background, return_info=True)
        want = P.polygonize(P.normalise(raster, background))
        _same(name, _fields(pg), want[:4])
        assert info == want[4] and info["rings"] >= 1, name
        R.same(name, vector.rasterize(pg.geometry, (H, W)), P.normalise(raster, background).astype(np.int32))
    assert len(np.unique(rasters["landform"])) >= 4 and len(np.unique(rasters["catchment"])) >= 4


# ---- the device tier ------------------------------------------------------------------------------------------------------
def _guarded(ctx, nbytes):
    """a device block of nbytes between two guard bands, all 0xA5 -> (array, pointer to the inside)"""
    a = ctx.to_device(np.full(nbytes + 2 * GUARD, 0xA5, np.uint8))
    return a, C.c_void_p(a.ptr.value + GUARD)


def _dev(ctx, raster, cap_edges, cap_vertices, cap_rings):
    """dt_dev_polygonize on device arrays filled with 0xA5 -> (coords, parts, ids, shell as the whole capacity, info);
    the guard bands around the four outputs must keep their pattern"""
    from descriptools_amd import _lib
    lab = np.ascontiguousarray(np.where(raster >= 0, raster, -1), np.int32)
    H, W = lab.shape
    sizes = (16 * cap_vertices, 8 * (cap_rings + 1), 4 * cap_rings, 4 * cap_rings)
    dtypes = (np.float64, np.int64, np.int32, np.int32)
    d_lab, d_info = ctx.to_device(lab), ctx.to_device(np.full(8, -7, np.int64))
    blocks = [_guarded(ctx, n) for n in sizes]
    try:
        _lib.check(_lib.lib().dt_dev_polygonize(ctx.h, d_lab.ptr, H, W, cap_edges, cap_vertices, cap_rings,
                                                *[p for _, p in blocks], d_info.ptr))
        out = []
        for (a, _), n, dt in zip(blocks, sizes, dtypes):
            raw = a.to_host()
            assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + n:] == 0xA5).all(), "a guard band was written"
            out.append(raw[GUARD:GUARD + n].view(dt))
        out[0] = out[0].reshape(-1, 2)
        return out, d_info.to_host().tolist()
    finally:
        for a in [d_lab, d_info] + [a for a, _ in blocks]:
            a.free()


def _cut(out, info):
    """the used part of the outputs of a call that fitted"""
    V, n = info[1], info[2]
    return out[0][:V], out[1][:n + 1], out[2][:n], out[3][:n]


@pytest.mark.parametrize("name", ["nested", "holes in a row", "long walks", "tie", "noise with background", "spiral 65x67",
                                  "all background", "1x5000 strip", "terrain"])
def test_device_tier_equals_the_host_tier_and_the_reference(name):
    from descriptools_amd import vector
    from descriptools_amd.device import Context
    raster = _raster(name)
    want = _ref(name)
    counts = [want[4][k] for k in INFO]
    pg, hinfo = vector.polygonize(raster, return_info=True)
    ctx = Context()
    try:
        out, info = _dev(ctx, raster, counts[0], counts[1], counts[2])       # exact capacities succeed
        assert info[:6] == counts + [0], name
        _same(name, _cut(out, info), want[:4])
        _same(name + " host tier", _cut(out, info), _fields(pg))
        assert info[:5] == [hinfo[k] for k in INFO]
        for a, used in zip(out, (2 * counts[1], counts[2] + 1, counts[2], counts[2])):
            assert (a.reshape(-1).view(np.uint8)[used * a.itemsize:] == 0xA5).all(), "written past what is used"
        roomy, rinfo = _dev(ctx, raster, counts[0] + 1000, counts[1] + 77, counts[2] + 300)
        assert rinfo == info
        _same(name + " roomy", _cut(roomy, rinfo), want[:4])
        again, ainfo = _dev(ctx, raster, counts[0], counts[1], counts[2])    # the same bytes the second time
        assert ainfo == info and all(a.tobytes() == b.tobytes() for a, b in zip(again, out))
        assert ctx.status() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["nested", "noise of 8 labels", "holes in a row"])
def test_a_capacity_too_small_leaves_the_outputs_untouched_and_says_so(name):
    from descriptools_amd.device import Context
    raster = _raster(name)
    want = _ref(name)
    E, V, n, holes, rounds = (want[4][k] for k in INFO)
    ctx = Context()
    try:
        for caps, flags in (((E - 1, V, n), 1), ((0, V, n), 1), ((E, V - 1, n), 2), ((E, 0, n), 2), ((E, V, n - 1), 4),
                            ((E, V, 0), 4), ((E, V - 1, n - 1), 6), ((E - 1, V - 1, n - 1), 3), ((0, 0, 0), 3)):
            out, info = _dev(ctx, raster, *caps)
            for a in out:
                assert (a.reshape(-1).view(np.uint8) == 0xA5).all(), (name, caps)
            assert info[0] == E and info[1] == V and info[5] == flags, (name, caps, info)
            # the rings are counted whenever the edges fit
            assert info[2] == (-1 if flags & 1 else n) and info[3] == (-1 if flags & 1 else 0), (name, caps, info)
            if not flags & 1:
                assert info[4] == rounds
        out, info = _dev(ctx, raster, E, V, n)
        assert info[:6] == [E, V, n, holes, rounds, 0]
        _same(name, _cut(out, info), want[:4])
        assert ctx.status() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["tie", "long walks", "1x5000 strip", "all background", "1x1"])
def test_c_entry_writes_nothing_outside_its_outputs(name):
    from descriptools_amd import _lib
    raster = _raster(name)
    want = _ref(name)
    V, n = want[4]["vertices"], want[4]["rings"]
    lab = np.ascontiguousarray(np.where(raster >= 0, raster, -1), np.int32)
    H, W = lab.shape
    cap_v, cap_r = V + 5, V // 4 + 3       # roomier than needed: the unused tail stays untouched as well
    raws = [np.full(2 * GUARD + nbytes, 0xA5, np.uint8) for nbytes in (16 * cap_v, 8 * (cap_r + 1), 4 * cap_r, 4 * cap_r)]
    views = [raw[GUARD:raw.size - GUARD].view(dt) for raw, dt in zip(raws, (np.float64, np.int64, np.int32, np.int32))]
    info = np.zeros(8, np.int64)
    _lib.check(_lib.lib().dt_polygonize(_lib.ptr(lab, _lib.c_i32p), H, W, cap_v, cap_r, _lib.ptr(views[0], _lib.c_f64p),
                                        _lib.ptr(views[1], _lib.c_i64p), _lib.ptr(views[2], _lib.c_i32p),
                                        _lib.ptr(views[3], _lib.c_i32p), _lib.ptr(info, _lib.c_i64p)))
    assert info[:6].tolist() == [want[4][k] for k in INFO] + [0]
    for raw, view, used in zip(raws, views, (2 * V, n + 1, n, n)):
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
        assert (view.view(np.uint8)[used * view.itemsize:] == 0xA5).all()
    _same(name, (views[0][:2 * V].reshape(-1, 2), views[1][:n + 1], views[2][:n], views[3][:n]), want[:4])
    # one ring short: nothing comes back but info
    if n:
        for raw in raws:
            raw[:] = 0xA5
        _lib.check(_lib.lib().dt_polygonize(_lib.ptr(lab, _lib.c_i32p), H, W, cap_v, n - 1, _lib.ptr(views[0], _lib.c_f64p),
                                            _lib.ptr(views[1], _lib.c_i64p), _lib.ptr(views[2], _lib.c_i32p),
                                            _lib.ptr(views[3], _lib.c_i32p), _lib.ptr(info, _lib.c_i64p)))
        assert info[:3].tolist() == [want[4]["edges"], V, n] and info[5] == 4
        assert all((raw == 0xA5).all() for raw in raws)


def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("name", ["nested", "noise of 8 labels", "long walks"])
def test_device_tier_writes_nothing_outside_its_scratch(name):
    """The context's scratch holds 768 bytes of round flags, two arrays of 4 bytes per 1024 lattice vertices, 4 bytes per
    cell, two arrays of 8 bytes per edge and one of 4, each rounded up to 256.  Grown by a roomy call and filled with a
    pattern, then used by a call with the exact capacities: every pad and everything behind the last array keep it."""
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    raster = _raster(name)
    want = _ref(name)
    H, W = raster.shape
    E, V, n = (want[4][k] for k in INFO[:3])
    L = _lib.lib()
    ctx = Context()
    try:
        _dev(ctx, raster, E + 4096, V + 4096, n + 4096)
        nbytes, base = L.dt_ctx_scratch_bytes(ctx.h), L.dt_ctx_scratch_ptr(ctx.h)
        nb = (H * (W + 1) + 1023) // 1024
        arrays = [768, 4 * nb, 4 * nb, 4 * H * W, 8 * E, 8 * E, 4 * E]
        spans, at = [], 0
        for size in arrays:
            spans.append((at, at + size))
            at += _align(size)
        assert base and nbytes >= at + 20 * 4096
        pattern = np.full(nbytes, 0xA5, np.uint8)
        _lib.check(L.dt_dev_h2d(ctx.h, base, pattern.ctypes.data_as(C.c_void_p), nbytes))
        out, info = _dev(ctx, raster, E, V, n)
        assert L.dt_ctx_scratch_ptr(ctx.h) == base and L.dt_ctx_scratch_bytes(ctx.h) == nbytes
        after = np.empty(nbytes, np.uint8)
        _lib.check(L.dt_dev_d2h(ctx.h, after.ctypes.data_as(C.c_void_p), base, nbytes))
        for k, (lo, hi) in enumerate(spans):
            end = spans[k + 1][0] if k + 1 < len(spans) else nbytes
            assert (after[hi:end] == 0xA5).all(), "the pad behind array %d of the scratch" % k
        # the cells' first edges are there: the last cell's offset plus its edges is the total
        celloff = after[spans[3][0]:spans[3][1]].view(np.uint32)
        assert 0 < celloff.max() <= E and (np.diff(celloff.astype(np.int64)) >= 0).all()
        _same(name, _cut(out, info), want[:4])
    finally:
        ctx.close()


def test_refusals_and_their_messages():
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    L = _lib.lib()
    ctx = Context()
    try:
        lab = ctx.to_device(np.zeros((4, 5), np.int32))
        out = [ctx.empty((256,), np.int64) for _ in range(5)]     # room for 80 vertices and 20 rings
        ptrs = [a.ptr for a in out]
        for args, message in (((lab.ptr, 4, 5, 80, 80, 20, None) + tuple(ptrs[1:]), b"NULL coords, parts, ids, shell or info"),
                              ((lab.ptr, 4, 5, 80, 80, 20) + tuple(ptrs[:4]) + (None,), b"NULL coords, parts, ids, shell or info"),
                              ((None, 4, 5, 80, 80, 20) + tuple(ptrs), b"NULL labels"),
                              ((lab.ptr, 0, 5, 80, 80, 20) + tuple(ptrs), b"empty raster shape"),
                              ((lab.ptr, 2 ** 16, 2 ** 15, 80, 80, 20) + tuple(ptrs), b"raster of 2^31 cells or more"),
                              ((lab.ptr, 4, 5, -1, 80, 20) + tuple(ptrs), b"cap_edges must be in [0, 2^31) edges"),
                              ((lab.ptr, 4, 5, 80, -1, 20) + tuple(ptrs), b"cap_vertices must be in [0, 2^31) vertices"),
                              ((lab.ptr, 4, 5, 80, 80, -1) + tuple(ptrs), b"cap_rings must be in [0, 2^31) rings"),
                              ((lab.ptr, 4, 5, 2 ** 31, 80, 20) + tuple(ptrs), b"cap_edges must be in [0, 2^31) edges")):
            assert L.dt_dev_polygonize(ctx.h, *args) == -1
            assert L.dt_last_error() == b"invalid argument: " + message
        assert L.dt_dev_polygonize(None, lab.ptr, 4, 5, 80, 80, 20, *ptrs) == -1
        phases = (C.c_double * 7)()
        assert L.dt_dev_polygonize_timed(ctx.h, lab.ptr, 4, 5, 80, 80, 20, *ptrs, None) == -1
        assert L.dt_last_error() == b"invalid argument: phase_ms is NULL"
        _lib.check(L.dt_dev_polygonize_timed(ctx.h, lab.ptr, 4, 5, 80, 80, 20, *ptrs, phases))
        want = P.polygonize(np.zeros((4, 5), np.int32))[4]
        assert want["edges"] == 18 and want["vertices"] == 4
        assert all(t >= 0.0 for t in phases) and out[4].to_host()[:6].tolist() == [want[k] for k in INFO] + [0]
        assert ctx.status() == 0
        for a in [lab] + out:
            a.free()
    finally:
        ctx.close()
