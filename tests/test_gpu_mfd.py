"""GPU (-m gpu): multiple-flow-direction shares and contributing area (descriptools_amd.mfd, dt_mfd_shares,
dt_mfd_accumulate and the device tier; k_mfd_shares / k_mf_* in dt_mfd.hip) against the numpy reference
(tests/_mfd_ref.py).  Shares with an integer exponent: bit for bit.  Shares with another exponent: the GPU's pow and
numpy's need not round alike, so the same nodata and no-receiver cells, every sum exactly 32768, every slot within one
unit, and at most 16 cells of a raster that differ at all (a 2-ulp error of pow moves r * 2^15 by less than 2^-36, so
fewer than 10^-3 cells of a 600 x 1000 raster are expected to sit that close to an integer).  Accumulation: bit for
bit, on the reference's shares."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import golden
from descriptools_amd import mfd

import _mfd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = 10.0
U = 32768


def _bits_equal(name, g, r):
    assert g.dtype == r.dtype and g.shape == r.shape, name
    if g.dtype.kind == "f":
        g, r = g.view(np.int64), r.view(np.int64)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        i = tuple(bad[0])
        raise AssertionError("%s: %d values differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i], r[i]))


@functools.lru_cache(maxsize=None)
def terrain(H, W, nodata_pct):
    dem = oracle.synth_dem(11, H, W, nodata_pct=nodata_pct)
    dem.setflags(write=False)
    return dem


def _cone(H=211, W=190):
    yy, xx = np.mgrid[0:H, 0:W]
    return (5000 - 7 * np.sqrt((yy - 100.0) ** 2 + (xx - 93.0) ** 2)).astype(np.float32)


def _plane(H, W):
    """tilted along the diagonal: every interior cell sends to E, S and SE and receives from W, N and NW"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (3000 - yy - xx).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ref_shares(kind, H, W, nodata_pct=0):
    """the reference's shares (exponent 1) of a terrain, the cone or the plane, read-only"""
    dem = terrain(H, W, nodata_pct) if kind == "terrain" else {"cone": _cone, "plane": _plane}[kind](H, W)
    s = R.flow_shares(dem, 1)
    s.setflags(write=False)
    return s


def check_shares(dem, exponent, contour=False, fdr=None):
    """GPU shares against the reference: bit for bit with an integer exponent, by the per-cell rule otherwise;
    returns the reference's"""
    got = mfd.flow_shares(dem, exponent, contour, fdr)
    ref = R.flow_shares(dem, exponent, contour, fdr)
    assert got.dtype == np.uint16 and got.shape == dem.shape + (8,) and got.flags.c_contiguous
    if float(exponent) == int(exponent):
        _bits_equal("shares, exponent %r, contour %r" % (exponent, contour), got, ref)
        return ref
    g, r = got.astype(np.int64), ref.astype(np.int64)
    assert np.array_equal((got == 0xFFFF).all(axis=2), (ref == 0xFFFF).all(axis=2)), "nodata cells differ"
    assert np.array_equal((got == 0).all(axis=2), (ref == 0).all(axis=2)), "cells without a receiver differ"
    live = ~(ref == 0xFFFF).all(axis=2)
    assert np.array_equal(g.sum(axis=2)[live], r.sum(axis=2)[live]), "a sum is not 32768"
    cells = int((g != r).any(axis=2).sum())
    worst = int(np.abs(g - r).max()) if g.size else 0
    print("shares %s exponent %r contour %r: %d cells differ from the reference, by at most %d"
          % (dem.shape, exponent, contour, cells, worst))
    assert worst <= 1
    assert cells <= 16
    return ref


def check_accumulate(shares, weights=None, frac_bits=None):
    got = mfd.accumulate(shares, weights, frac_bits)
    ref = R.accumulate(shares, weights, frac_bits)
    assert got.dtype == np.float64
    _bits_equal("accumulation", got, ref)
    return ref


# ---- shares --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contour", [False, True])
@pytest.mark.parametrize("exponent", [1, 2, 4, 0])
def test_shares_integer_exponents(exponent, contour):
    for H, W, nodata_pct in ((200, 333, 0), (200, 333, 2), (600, 1000, 0), (600, 1000, 2)):
        ref = check_shares(terrain(H, W, nodata_pct), exponent, contour)
        nod = (ref == 0xFFFF).all(axis=2)
        assert nod.any() == (nodata_pct > 0)
        assert np.isin(ref[~nod].sum(axis=1, dtype=np.int64), (0, U)).all()


@pytest.mark.parametrize("exponent", [1.1, 0.5])
def test_shares_non_integer_exponents(exponent):
    for H, W, nodata_pct in ((200, 333, 2), (600, 1000, 0), (600, 1000, 2)):
        check_shares(terrain(H, W, nodata_pct), exponent)
    check_shares(terrain(200, 333, 2), exponent, True)
    check_shares(_cone(), exponent)


def test_shares_cone_is_divergent():
    for exponent, contour in ((1, False), (1, True), (4, False), (0, True)):
        ref = check_shares(_cone(), exponent, contour)
        receivers = (ref > 0).sum(axis=2)
        assert receivers[receivers > 0].mean() > 3, "a cone spreads its flow"


@pytest.mark.parametrize("name", ["nonfinite", "nonfinite_f64"])
def test_shares_non_finite_heights(name):
    g = golden(name)
    dem = g["dem"].astype(np.float32)  # NaN, +inf, -inf and below-sentinel heights
    assert np.isnan(dem).any() and np.isinf(dem).any() and (dem < -100).any()
    for exponent in (1, 3, 1.1):
        ref = check_shares(dem, exponent)
        check_shares(dem, exponent, True, g["fdr"])
        odd = ~np.isfinite(dem) & ~(dem <= -100)
        assert (ref[odd] == 0).all() and (ref[dem <= -100] == 0xFFFF).all()
        assert ((ref == 0xFFFF).all(axis=2) == (dem <= -100)).all()


@pytest.mark.parametrize("shape", [(1, 37), (41, 1), (2, 2), (65, 1), (1, 1), (3, 130), (9, 129)])
def test_shares_odd_shapes(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    dem = rng.integers(0, 50, shape).astype(np.float32)
    dem[0, 0] = -100
    fdr = np.full(shape, 4, np.uint8)
    for exponent in (1, 1.1):
        check_shares(dem, exponent)
        ref = check_shares(dem, exponent, True, fdr)
        check_accumulate(ref)
    flat = np.full(shape, 7, np.float32)
    flat[-1, -1] = -100
    ref = check_shares(flat, 1)
    assert np.isin(ref, (0, 0xFFFF)).all()
    check_accumulate(ref)
    check_accumulate(check_shares(flat, 2, False, fdr))  # the whole flat runs south along the codes


def _pitted():
    """terrain with planted pits and a flat shelf"""
    dem = oracle.synth_dem(5, 150, 210, nodata_pct=1).copy()
    rng = np.random.default_rng(8)
    for _ in range(40):
        y, x = int(rng.integers(3, 147)), int(rng.integers(3, 207))
        if (dem[y - 2:y + 3, x - 2:x + 3] > -100).all():
            dem[y - 1:y + 2, x - 1:x + 2] -= 25
            dem[y, x] -= 10
    shelf = dem[60:90, 40:120]
    shelf[shelf > -100] = np.float32(np.median(shelf[shelf > -100]))
    return dem


@functools.lru_cache(maxsize=None)
def conditioned():
    """(filled surface, codes) of flowdir.d8_conditioned on the pitted terrain, read-only"""
    from descriptools_amd import flowdir
    fdr, filled = flowdir.d8_conditioned(_pitted(), PX, return_filled=True)
    filled = np.ascontiguousarray(filled, np.float32)
    filled.setflags(write=False)
    fdr.setflags(write=False)
    return filled, fdr


def test_shares_fallback_on_conditioned_surface():
    filled, fdr = conditioned()
    s0 = check_shares(filled, 1)
    s1 = check_shares(filled, 1, False, fdr)
    none0, none1 = (s0 == 0).all(axis=2), (s1 == 0).all(axis=2)
    assert (none0 & ~none1).sum() > 500, "the shelf and the filled pits take the D8 codes"
    _bits_equal("cells with a lower neighbour", s1[~none0], s0[~none0])
    # every valid cell that is not an outlet has a receiver: a cell without one holds a code that points off the
    # raster or at a cell that is not valid
    valid = np.isfinite(filled) & (filled > -100)
    for y, x in np.argwhere(none1 & valid):
        k = R.OCT_CODE.index(int(fdr[y, x]))
        ny, nx = y + R.OCT_DY[k], x + R.OCT_DX[k]
        assert not (0 <= ny < filled.shape[0] and 0 <= nx < filled.shape[1] and valid[ny, nx])
    # the drainage graph has no cycle: the reference's accumulation is complete
    acc = check_accumulate(s1)
    assert np.array_equal(acc == -100, filled <= -100)


# ---- accumulation on the reference's shares -----------------------------------------------------------------------
@pytest.mark.parametrize("H,W,nodata_pct", [(200, 333, 0), (200, 333, 2), (600, 1000, 0), (600, 1000, 2)])
def test_accumulate_terrain_unit_weights(H, W, nodata_pct):
    ref = check_accumulate(ref_shares("terrain", H, W, nodata_pct))
    assert ref.max() > 1000


def test_accumulate_float_weights():
    s = ref_shares("terrain", 600, 1000, 2)
    w = np.random.default_rng(1).uniform(0, 10, s.shape[:2])
    check_accumulate(s, w)
    check_accumulate(ref_shares("terrain", 200, 333, 2), w[:200, :333].astype(np.float32))


def test_accumulate_integer_weights_frac_bits_0():
    s = ref_shares("terrain", 600, 1000, 2)
    w = np.random.default_rng(2).integers(0, 1000, s.shape[:2])
    ref = check_accumulate(s, w, 0)
    assert (ref[ref != -100] == np.rint(ref[ref != -100])).all()


def test_accumulate_cone():
    s = ref_shares("cone", 211, 190)
    ref = check_accumulate(s)
    assert (ref != -100).all()
    check_accumulate(R.flow_shares(_cone(), 4, True))


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from descriptools_amd import mfd
acc, _, _, info = mfd._accumulate(np.load(sys.argv[1]), None, None)
np.save(sys.argv[2], acc)
print("INFO", info["rounds"], info["queued"], info["queue_high"])
"""


def test_accumulate_plane_and_forced_spill(tmp_path):
    """every interior cell has three donors and three receivers; a fresh process with DT_DBG_MFD_STACK=1 runs the
    spill queue and several rounds, and gives the same bytes"""
    s = ref_shares("plane", 300, 500)
    assert ((s[1:-1, 1:-1] > 0).sum(axis=2) == 3).all() and (s[1:-1, 1:-1][:, :, [0, 6, 7]] > 0).all()
    ref = check_accumulate(s)
    np.save(tmp_path / "s.npy", s)
    env = dict(os.environ, DT_DBG_MFD_STACK="1")
    out = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(tmp_path / "s.npy"), str(tmp_path / "acc.npy")],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rounds, queued, high = (int(v) for v in out.stdout.split("INFO")[1].split())
    print("forced spill: %d rounds, %d cells queued, largest round %d" % (rounds, queued, high))
    assert queued > 0 and rounds >= 2, "the spill path did not run"
    _bits_equal("forced spill", np.load(tmp_path / "acc.npy"), ref)


def test_accumulate_serpentine_depth():
    """one chain of single-receiver shares through every cell of 257 x 256 (65,791 moves): nothing depends on path
    depth"""
    H, W = 257, 256
    fdr = np.empty((H, W), np.uint8)
    fdr[0::2, :] = 1    # E
    fdr[1::2, :] = 16   # W
    fdr[0::2, -1] = 4   # S
    fdr[1::2, 0] = 4
    fdr[-1, -1] = 0
    s = mfd.d8_shares(fdr)
    order = np.arange(H * W).reshape(H, W)
    order[1::2] = order[1::2, ::-1]
    _bits_equal("serpentine", mfd.accumulate(s), order.astype(np.float64))
    w = np.random.default_rng(4).integers(0, 9, (H, W))
    got = mfd.accumulate(s, w, 0)
    flat = np.empty(H * W, np.int64)
    flat[order.reshape(-1)] = w.reshape(-1)
    want = np.empty(H * W, np.float64)
    want[order.reshape(-1)] = np.cumsum(flat) - flat
    _bits_equal("weighted serpentine", got, want.reshape(H, W))


def test_accumulate_d8_shares_equal_flowacc():
    from descriptools_amd import flowacc, flowdir
    dem = oracle.synth_dem(3, 600, 1001)
    fdr = flowdir.d8(dem, PX)
    got = mfd.accumulate(mfd.d8_shares(fdr), frac_bits=0)
    acc = flowacc.accumulate(fdr)
    assert (acc != -100).all()
    _bits_equal("D8 shares", got, acc.astype(np.float64))


def _short_path_d8(H, W, nodata_pct):
    """D8 codes down an egg-crate surface with basins of 16 x 16 cells (the lowest neighbour when it is strictly
    lower, so no cycle; 0 in the pits), `nodata_pct` % of the cells nodata -> (fdr, nodata mask).  Checked here: no
    flow path has more than 32 cells, the fewest either op lets a start complete in a round (MF_MOVES; DI_MOVES is
    128), and a D8 cell completes at most one receiver -- so nothing is queued, whatever the order of arrival."""
    yy, xx = np.mgrid[0:H, 0:W]
    z = np.cos(2 * np.pi * yy / 16) + np.cos(2 * np.pi * xx / 16)
    nod = np.random.default_rng(12).random((H, W)) < nodata_pct / 100
    steps = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))  # (dy, dx) by octant
    zp = np.pad(z, 1, constant_values=np.inf)
    nb = np.stack([zp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in steps])
    k = nb.argmin(axis=0)
    flows = nb.min(axis=0) < z
    fdr = np.where(flows, np.array(mfd.OCTANT_CODES, np.uint8)[k], 0).astype(np.uint8)
    cell = np.arange(H * W).reshape(H, W)
    to = cell + np.array([dy * W + dx for dy, dx in steps])[k]
    nxt = np.where(flows & ~nod, to, cell).reshape(-1)
    nxt = np.where(nod.reshape(-1)[nxt], cell.reshape(-1), nxt)  # a share into nodata leaves the domain
    pos = cell.reshape(-1)
    for _ in range(31):
        pos = nxt[pos]
    assert (nxt[pos] == pos).all(), "a flow path has more than 32 cells"
    return fdr, nod


def test_accumulate_d8_equals_dinf_byte_for_byte():
    """the two ops run one countdown (dt_countdown.h): on the same D8 raster, as float32(k pi / 4) angles and as
    single-receiver shares, they give the same bytes (the reference's) and neither queues a cell"""
    import _dinf_ref
    from descriptools_amd import dinf
    fdr, nod = _short_path_d8(33, 130, 5)
    assert 0.03 < nod.mean() < 0.07 and (fdr[~nod] != 0).mean() > 0.9
    a = _dinf_ref.d8_angles(fdr)
    a[nod] = -100
    s = mfd.d8_shares(fdr)
    s[nod] = mfd.NODATA_SLOT
    ref = R.accumulate(s, None, 0)
    assert (ref[nod] == -100).all() and (ref[~nod] >= 0).all() and ref.max() >= 16
    acc_d, _, _, info_d = dinf._accumulate(a, None, 0)
    acc_m, _, _, info_m = mfd._accumulate(s, None, 0)
    _bits_equal("MFD on D8 shares", acc_m, ref)
    _bits_equal("D-infinity on D8 angles against MFD on D8 shares", acc_d, acc_m)
    assert info_d["queued"] == 0 and info_m["queued"] == 0, (info_d, info_m)


def test_mass_conservation_with_nodata():
    """sum of q over the live cells = the totals held by the cells without an edge + what left the domain; the left
    side from the reference's bookkeeping, the right side from the device's raster"""
    s = ref_shares("terrain", 200, 333, 2)[20:180, 30:300].copy()  # cut out: shares along the rim point off the raster
    s[70:90, 100:140] = 0xFFFF                                      # and a lake: shares around it point into nodata
    w = np.random.default_rng(9).uniform(0, 5, s.shape[:2])
    fb = R.default_frac_bits(s.shape[0] * s.shape[1], float(w.max()))
    _, x = R.accumulate(s, w, fb, full=True)
    live = ~x["nodata"]
    assert x["done"][live].all()
    acc = mfd.accumulate(s, w, fb).reshape(-1)
    T = np.where(live, np.rint(np.ldexp(acc, fb)).astype(np.int64) + x["q"], 0)
    has_edge = x["edge"].any(axis=1)
    sent = R.split(T[live & has_edge], x["P"][live & has_edge])
    left = int(sent[x["gone"][live & has_edge]].sum())
    held = int(T[live & ~has_edge].sum())
    assert left > 0 and held > 0
    assert int(x["q"][live].sum()) == held + left


# 2 x 2 cycles; the second and the fourth lie across borders of the 128 x 8 tiles
CYCLES = ((10, 10), (63, 127), (150, 300), (127, 63))


def _with_cycles():
    s = ref_shares("terrain", 200, 333, 2).copy()
    for y, x in CYCLES:
        s[y:y + 2, x:x + 2] = 0
        s[y, x, 0] = s[y + 1, x + 1, 4] = s[y + 1, x, 2] = U  # E, then (below) S, W, N: clockwise
        s[y, x + 1, 6] = U
    y, x = CYCLES[1]
    s[y, x + 1, 6], s[y, x + 1, 0] = U - 9000, 9000  # part of this one leaks out to the east
    return s


def test_cycles_give_minus_100_on_and_below_them():
    s = _with_cycles()
    base = R.accumulate(ref_shares("terrain", 200, 333, 2))
    ref = check_accumulate(s)
    for y, x in CYCLES:
        assert (ref[y:y + 2, x:x + 2] == -100).all()
    y, x = CYCLES[1]
    assert ref[y, x + 2] == -100, "the cell the leak feeds never completes"
    lost = (ref == -100) & (base != -100)
    kept = (ref != -100) & (ref == base)
    assert lost.sum() > 16 and kept.sum() > 0.5 * ref.size, "cells elsewhere keep their values"


def test_two_runs_give_identical_bytes():
    dem = terrain(600, 1000, 2)
    runs = [mfd.flow_shares(dem, 1.1) for _ in range(2)]
    _bits_equal("shares, repeated", runs[1], runs[0])
    accs = [mfd.accumulate(runs[0]) for _ in range(2)]
    _bits_equal("accumulation, repeated", accs[1], accs[0])
    _bits_equal("the GPU's own shares", accs[0], R.accumulate(runs[0]))


# ---- the device tier ---------------------------------------------------------------------------------------------
def _pitted_large(H, W):
    dem = oracle.synth_dem(9, H, W, nodata_pct=1).copy()
    dem[100:140, 200:260][dem[100:140, 200:260] > -100] -= 30
    return np.ascontiguousarray(dem, np.float32)


def test_device_tier_on_a_chain():
    """dt_dev_mfd_shares on a conditioning Chain's filled surface and codes, dt_dev_mfd_accumulate on its shares, with
    no host synchronisation in between: equal to the host tier"""
    from descriptools_amd import _lib, chain, device
    H, W = 320, 448
    dem = _pitted_large(H, W)
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=PX, overlap=False, tune_placement=False, river_threshold=200, condition=True,
                     condition_rounds=500)
    d = ctx.to_device(dem)
    shr, acc = ctx.empty((H, W, 8), np.uint16), ctx.empty((H, W), np.float64)
    L = _lib.lib()
    try:
        ch.run(d.ptr)
        _lib.check(L.dt_dev_mfd_shares(ctx.h, ch.p("filled"), ch.p("fdr"), H, W, 2.0, 1, shr.ptr))
        _lib.check(L.dt_dev_mfd_accumulate(ctx.h, shr.ptr, None, H, W, 20, 256, acc.ptr))
        assert ctx.status() == 0
        info = np.zeros(4, np.int64)
        _lib.check(L.dt_dev_mfd_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
        g_shr, g_acc = shr.to_host(), acc.to_host()
        live = ~(g_shr == 0xFFFF).all(axis=2)
        assert info[3] == (((g_shr > 0).sum(axis=2) >= 2) & live).sum() and info[2] >= info[1] >= 0 and info[0] < 256
        filled, fdr = ch.buf["filled"].to_host(), ch.buf["fdr"].to_host()
        assert L.dt_dev_mfd_accumulate(ctx.h, None, None, 0, 0, 0, 1, None) == 0
        assert L.dt_dev_mfd_accumulate(ctx.h, shr.ptr, None, H, W, 20, 0, acc.ptr) != 0      # rounds 0
        assert L.dt_dev_mfd_shares(ctx.h, d.ptr, None, H, W, 65.0, 0, shr.ptr) != 0          # exponent
        assert L.dt_dev_mfd_shares(ctx.h, d.ptr, None, H, W, float("nan"), 0, shr.ptr) != 0
    finally:
        for b in (d, shr, acc):
            b.free()
        ch.free()
        ctx.close()
    host = mfd.flow_shares(filled, 2, True, fdr)
    _bits_equal("shares", g_shr, host)
    _bits_equal("shares against the reference", g_shr, R.flow_shares(filled, 2, True, fdr))
    _bits_equal("accumulation", g_acc, mfd.accumulate(host, frac_bits=20))
    assert np.array_equal(g_acc == -100, ~live), "conditioned: no cycle"


def test_device_tier_budget_of_rounds():
    """a budget of two rounds leaves queued work on the serpentine (a start completes a bounded number of cells in a
    round): DT_STATUS_NOT_CONVERGED; calls with a negative budget continue and finish it to the same bytes"""
    from descriptools_amd import _lib, device
    H, W = 65, 64
    fdr = np.empty((H, W), np.uint8)
    fdr[0::2, :], fdr[1::2, :] = 1, 16
    fdr[0::2, -1] = fdr[1::2, 0] = 4
    fdr[-1, -1] = 0
    s = mfd.d8_shares(fdr)
    ref = R.accumulate(s, None, 30)
    assert (ref != -100).all()
    ctx = device.Context()
    L = _lib.lib()
    d = ctx.to_device(s)
    out = ctx.empty((H, W), np.float64)
    try:
        _lib.check(L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, H, W, 30, 2, out.ptr))
        assert ctx.status() & 2, "DT_STATUS_NOT_CONVERGED"
        part = out.to_host()
        assert (part == -100).any() and ((part == ref) | (part == -100)).all()
        calls = 0
        while True:
            _lib.check(L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, H, W, 30, -8, out.ptr))
            calls += 1
            if not ctx.status() & 2:
                break
            assert calls < 100
        print("finished after %d further calls of 8 rounds" % calls)
        assert calls >= 2
        # a continuation names what it was started with
        assert L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, H, W, 29, -1, out.ptr) != 0
        assert L.dt_dev_mfd_accumulate(ctx.h, out.ptr, None, H, W, 30, -1, out.ptr) != 0
        assert L.dt_dev_mfd_accumulate(ctx.h, d.ptr, out.ptr, H, W, 30, -1, out.ptr) != 0
        assert L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, W, H, 30, -1, out.ptr) != 0      # another shape
        assert L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, H, W, 30, -1, out.ptr) == 0
        _bits_equal("continued", out.to_host(), ref)
        # another call on the context takes the scratch: nothing to continue
        other = ctx.to_device(np.ones((H, W), np.uint8))
        up = ctx.empty((H, W), np.float64)
        _lib.check(L.dt_dev_upslope_length(ctx.h, other.ptr, None, H, W, PX, up.ptr))
        assert L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, H, W, 30, -1, out.ptr) != 0
        info = np.zeros(4, np.int64)
        assert L.dt_dev_mfd_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)) != 0
        other.free()
        up.free()
    finally:
        d.free()
        out.free()
        ctx.close()


def test_bad_shares_on_the_device_tier():
    from descriptools_amd import _lib, device
    H, W = 70, 130
    good = ref_shares("terrain", 200, 333, 2)[:H, :W].copy()
    ctx = device.Context()
    L = _lib.lib()
    out = ctx.empty((H, W), np.float64)
    try:
        for y, x, word in ((33, 44, [U + 1, 0, 0, 0, 0, 0, 0, 0]), (7, 127, [20000, 0, 0, 0, 0, 12767, 0, 0]),
                           (8, 128, [0xFFFF] * 7 + [0]), (0, 0, [U, U, 0, 0, 0, 0, 0, 0])):
            b = good.copy()
            b[y, x] = word
            with pytest.raises(ValueError):
                mfd.accumulate(b)
            d = ctx.to_device(b)
            _lib.check(L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, H, W, 10, 64, out.ptr))
            assert ctx.status() & 32, "DT_STATUS_BAD_SHARES"
            got = out.to_host()
            d.free()
            b[y, x] = 0  # counted as a cell without a receiver
            _bits_equal("bad shares as no receiver", got, R.accumulate(b, None, 10))
        d = ctx.to_device(good)
        _lib.check(L.dt_dev_mfd_accumulate(ctx.h, d.ptr, None, H, W, 10, 64, out.ptr))
        assert ctx.status() == 0
        _bits_equal("good shares", out.to_host(), R.accumulate(good, None, 10))
        d.free()
    finally:
        out.free()
        ctx.close()


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_end_to_end_on_conditioned_terrain():
    filled, fdr = conditioned()
    s = mfd.flow_shares(filled, 1, False, fdr)
    rs = R.flow_shares(filled, 1, False, fdr)
    _bits_equal("shares", s, rs)
    acc = mfd.accumulate(s)
    racc = R.accumulate(rs)
    _bits_equal("accumulation", acc, racc)
    _bits_equal("sca", mfd.specific_catchment_area(s, PX), np.where(racc == -100, -100.0, (racc + 1.0) * PX))
    # with weights the cell's own quantised weight takes the place of the 1
    w = np.random.default_rng(6).uniform(0, 3, filled.shape)
    fb = R.default_frac_bits(filled.size, float(w.max()))
    accw = R.accumulate(rs, w, fb)
    own = np.ldexp(np.rint(np.ldexp(w, fb)), -fb)
    _bits_equal("weighted sca", mfd.specific_catchment_area(s, PX, w),
                np.where(accw == -100, -100.0, (accw + own) * PX))
