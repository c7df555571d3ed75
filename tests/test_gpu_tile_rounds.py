"""GPU (-m gpu): the tile-round schedule (csrc/dt_tile_rounds.h) under the four ops that run on its scaffold -- the cost
distance, the modified catchment area, the D-infinity distance and the harmonic smoother -- at the shapes where the
schedule itself can go wrong, through the public Python functions, against the references and with the comparisons of
the ops' own tests (test_gpu_cost, test_gpu_wetness, test_gpu_dinf_dist: bit for bit; test_gpu_harmonic: the contract).

  1 x 1       one cell: nothing can change, so no round does anything and the one tile is visited once
  64 x 64     one tile of 64 (2 x 2 of 32): colours 1-3 launch nothing
  65 x 64     tiles 2 x 1: colours 1 and 3 empty, a tile of one row
  64 x 130    tiles 1 x 3: colours 2 and 3 empty
  129 x 193   tiles 3 x 4 (5 x 7 of 32): odd and even counts, ragged edges on both axes

The inputs send one front through every tile and back: the serpentine corridors of the cost and the wetness tests from
a single source in a corner and a snake of D-infinity angles that ends in a single stream cell; the smoother gets
scattered fixed cells in a domain with holes, so that every tile hands values to all its neighbours until the residual
is met.  So resting tiles wake up again, and every shape beyond one cell takes at least one round that does
something."""
import functools

import numpy as np
import pytest

import _cost_ref as CR
import _dinf_dist_ref as DR
import _dinf_ref as AR
import _harmonic_ref as HR
import _wetness_ref as WR
import test_gpu_cost as TC
import test_gpu_dinf_dist as TD
import test_gpu_harmonic as TH
import test_gpu_wetness as TW

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (64, 64), (65, 64), (64, 130), (129, 193)]
LARGE = (129, 193)
IDS = ["%dx%d" % s for s in SHAPES]
NOT_CONVERGED = 2  # DT_STATUS_NOT_CONVERGED


def _rounds(info, shape):
    print("%s: rounds %d, tile visits %d" % (shape, info["rounds"], info["tile_visits"]))
    if shape == (1, 1):
        # a single cell has no neighbour to take anything from: the first round visits the tile and changes nothing
        assert info["rounds"] == 0 and info["tile_visits"] == 1
    else:
        assert info["tile_visits"] >= info["rounds"] >= 1


# ---- cost distance --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cost_case(shape):
    f, s = CR.serpentine(shape)
    ref = CR.reference(f, s, TC.PX, 8)
    for a in (f, s) + ref[:3]:
        a.setflags(write=False)
    return f, s, ref


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_cost_distance(shape):
    f, s, ref = _cost_case(shape)
    assert ref[4] == int(CR.passable(f).sum()), "the corridor reaches every passable cell"
    got = TC.check(f, s, ref=ref)
    _rounds(got.info, shape)
    if shape == LARGE:
        assert got.info["rounds"] > 1


def test_cost_distance_device_tier_budget():
    from descriptools_amd.device import Context
    f, s, ref = _cost_case(LARGE)
    ctx = Context()
    try:
        c, i, b, st = TC._dev(ctx, f, s, 8, 0, 1)
        assert st & NOT_CONVERGED
        c, i, b, st = TC._dev(ctx, f, s, 8, 0, 4096)
        assert st == 0
        TC._same("cost", c, ref[0])
        TC._same("indices", i, ref[1])
        TC._same("backlink", b, ref[2])
    finally:
        ctx.close()


# ---- modified catchment area ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wetness_case(shape):
    a, s = WR.serpentine(shape, s=np.float32(0.999))
    M = WR.reference(a, s)
    for x in (a, s, M):
        x.setflags(write=False)
    return a, s, M


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_modified_catchment_area(shape):
    a, s, M = _wetness_case(shape)
    got = TW.check(a, s, ref=M)
    _rounds(got.info, shape)
    ok = WR.valid(a, s)
    assert got.info["raised"] == int(ok.sum()) - 1, "the peak in the corner raises every other valid cell"
    if shape == LARGE:
        assert got.info["rounds"] > 1


def test_modified_catchment_area_device_tier_budget():
    from descriptools_amd.device import Context
    a, s, M = _wetness_case(LARGE)
    ctx = Context()
    try:
        m, st = TW._dev_area(ctx, a, s, 0, 1)
        assert st & NOT_CONVERGED
        m, st = TW._dev_area(ctx, a, s, 0, 4096)
        assert st == 0
        TW._same("modified", m, M)
    finally:
        ctx.close()


# ---- D-infinity distance --------------------------------------------------------------------------------------------
def _snake(shape):
    """test_gpu_dinf_dist._snake on any shape: even rows run alternately east and west, joined by south connectors
    through the odd rows; the other cells are dead.  -> angle, river (the outlet alone), heights that fall along the path
    (0.25 per hop: every sum is exact)"""
    H, W = shape
    E, W_, S = AR.octant_angle(0), AR.octant_angle(4), AR.octant_angle(6)
    a = np.full(shape, -1, np.float32)
    a[1::2, 1::2] = E
    path = []
    for i, y in enumerate(range(0, H, 2)):
        a[y, :] = E if i % 2 == 0 else W_
        path.extend(y * W + x for x in (range(W) if i % 2 == 0 else range(W - 1, -1, -1)))
        if y + 2 < H:
            xe = W - 1 if i % 2 == 0 else 0
            a[y, xe] = a[y + 1, xe] = S
            path.append((y + 1) * W + xe)
    a.reshape(-1)[path[-1]] = -1  # the outlet has no receiver
    river = np.zeros(shape, np.int8)
    river.reshape(-1)[path[-1]] = 1
    hops = np.zeros(H * W, np.int64)
    hops[path] = np.arange(len(path) - 1, -1, -1)
    return a, river, (hops * 0.25).astype(np.float32).reshape(shape), len(path)


@functools.lru_cache(maxsize=None)
def _dinf_case(shape):
    a, river, dem, n = _snake(shape)
    want = DR.distance_down(a, river, 2.0, dem, "ave", True)
    for x in (a, river, dem) + tuple(want):
        x.setflags(write=False)
    return a, river, dem, n, want


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dinf_distance_down(shape):
    a, river, dem, n, want = _dinf_case(shape)
    # (beside the path an odd-row cell next to a connector in the last column drains into it)
    reach = int((want[0] != -100).sum())
    assert reach >= n and want[0].max() == 2.0 * (n - 1), "the whole path reaches the outlet"
    TD.check(a, river, 2.0, dem, "ave", True, (0,), want=want)
    rc, h, v, s, info = TD.call(a, river, 2.0, dem)
    assert rc == 0
    for name, g, r in zip(TD.NAMES, (h, v, s), want):
        TD._bits_equal(name + " (C entry)", g, r)
    H, W = shape
    assert info[1] == reach and info[2] == H * W - reach and info[3] == 0
    print("%s: rounds %d" % (shape, info[0]))
    assert (info[0] == 0) if shape == (1, 1) else (info[0] >= 1)  # (the entry reports no tile visits)
    if shape == LARGE:
        assert info[0] > 1


# ---- harmonic interpolation -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _harmonic_case(shape):
    """test_gpu_harmonic's random case on any shape: 10 % of the cells outside the domain and a hole of 5 x 5 on the
    corner of the first four tiles, 2 % of the domain fixed (and the cell (0, 0)), values from a seeded normal
    distribution: every tile has cells to solve and a value to pass on to each of its neighbours.  (One-cell walls with
    sparse fixed cells between them are no input for this test: they vanish on the coarser levels, the start is poor,
    and the smoother then needs more than the 4096 rounds of the budget on 129 x 193.)"""
    rng = np.random.default_rng(3)
    dom = rng.random(shape) >= 0.10
    dom[62:67, 62:67] = False
    dom[0, 0] = True
    fixed = dom & (rng.random(shape) < 0.02)
    fixed[0, 0] = True
    v = np.where(fixed, rng.normal(200.0, 50.0, shape), 0.0).astype(np.float32)
    for x in (v, fixed, dom):
        x.setflags(write=False)
    return v, fixed, dom


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_harmonic_interpolate(shape):
    from descriptools_amd import harmonic
    v, fixed, dom = _harmonic_case(shape)
    got = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TH.TOL)
    reach = TH._check(got, v, fixed, dom)
    assert reach.sum() >= 0.85 * v.size, "nearly every cell has a value"
    assert got.info["tile_visits"] >= got.info["rounds"] >= 1
    H, W = shape
    assert got.info["levels"] == (1 if max(H, W) <= 64 else (2 if max(H, W) <= 128 else 3))
    if H * W > 1:
        lo, hi = float(v[fixed].min()), float(v[fixed].max())
        assert got.field[reach].min() >= lo and got.field[reach].max() <= hi
    again = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TH.TOL)
    assert np.array_equal(TH._bits(got.field), TH._bits(again.field)) and again.info == got.info
