"""GPU (-m gpu): flowpath.downstream_sum / upslope_longest / travel_time / time_of_concentration
(dt_flowpath_downstream_sum, dt_flowpath_upslope_longest and the device tier; k_ps_dn_* and the raw-key k_fp_up_* in
dt_flowpath.hip) against the pure-numpy reference (tests/_pathsum_ref.py).  Everything is compared with
assert_array_equal, dtypes and -100 positions included: nothing here has a tolerance, because both sides are integer
sums scaled by a power of two.

Hand-built cases through both tiers, degenerate shapes, a serpentine path through every cell of six tiles with closed
forms (sums just under 2^52, a negative frac_bits, integer weights), D8 cycles across tile seams with their in-tile
twins, border rings, random fields with cycles, nodata and stops, identities on the GPU outputs, and the device tier's
contract."""
import numpy as np
import pytest

import oracle

import _pathsum_ref as R
import _watershed_ref as WR
from _watershed_ref import E, N, S, SE, SW, W_

pytestmark = pytest.mark.gpu


def _same(name, got, want):
    assert got.dtype == want.dtype == np.float64, name
    np.testing.assert_array_equal(got, want, err_msg=name)


def check(fdr, weights, dem=None, stop=None, frac_bits=None):
    """downstream_sum (with and without `stop` when one is given) and upslope_longest against the reference.
    Returns {"up": U, ("dn", stopped): T}"""
    from descriptools_amd import flowpath as fp
    out = {}
    ref = R.upslope_longest(fdr, weights, dem, frac_bits)
    _same("upslope_longest", fp.upslope_longest(fdr, weights, dem, frac_bits), ref)
    out["up"] = ref
    for st in ((None,) if stop is None else (None, stop)):
        ref = R.downstream_sum(fdr, weights, dem, st, frac_bits)
        _same("downstream_sum stop=%s" % (st is not None), fp.downstream_sum(fdr, weights, dem, st, frac_bits), ref)
        out["dn", st is not None] = ref
    return out


class Dev:
    """the device tier on host arrays: uploads, calls, downloads"""

    def __init__(self):
        from descriptools_amd import _lib, device
        self.lib, self.L, self.ctx = _lib, _lib.lib(), device.Context()

    def close(self):
        self.ctx.close()

    def run(self, fold, fdr, weights, frac_bits, dem=None, stop=None):
        H, W = fdr.shape
        held = [self.ctx.to_device(np.ascontiguousarray(fdr, np.uint8)),
                self.ctx.to_device(np.ascontiguousarray(weights, np.float64))]
        d = s = None
        if dem is not None:
            held.append(self.ctx.to_device(self.lib.nodata_mask(dem, fdr.shape)))
            d = held[-1].ptr
        if stop is not None:
            held.append(self.ctx.to_device(np.ascontiguousarray(np.asarray(stop) != 0, np.uint8)))
            s = held[-1].ptr
        o = self.ctx.empty((H, W), np.float64)
        held.append(o)
        try:
            if fold == "up":
                self.lib.check(self.L.dt_dev_flowpath_upslope_longest(self.ctx.h, held[0].ptr, d, held[1].ptr, H, W,
                                                                      frac_bits, o.ptr))
            else:
                self.lib.check(self.L.dt_dev_flowpath_downstream_sum(self.ctx.h, held[0].ptr, d, held[1].ptr, s, H, W,
                                                                     frac_bits, o.ptr))
            self.ctx.sync()
            return o.to_host()
        finally:
            for a in held:
                a.free()


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_built(name, dev):
    from descriptools_amd import flowpath as fp
    c = R.hand_cases()[name]
    fdr, w, dem, stop, s = c["fdr"], c["weights"], c["dem"], c["stop"], c["frac_bits"]
    _same("host down", fp.downstream_sum(fdr, w, dem, stop, s), c["dn"])
    _same("host up", fp.upslope_longest(fdr, w, dem, s), c["up"])
    _same("device down", dev.run("dn", fdr, w, s, dem, stop), c["dn"])
    _same("device up", dev.run("up", fdr, w, s, dem), c["up"])


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (64, 64), (65, 129), (130, 67), (0, 0), (0, 9), (9, 0)])
def test_shapes(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    fdr = rng.choice(np.array([E, W_, S, N, SE, 0], np.uint8), size=shape)
    if shape[0] == 1:
        fdr[:] = E
    if shape[1] == 1:
        fdr[:] = S
    stop = rng.random(shape) < 0.02
    out = check(fdr, rng.random(shape) * 12.5, None, stop)
    assert out["up"].shape == shape


def _serpentine(H, W):
    fdr = np.zeros((H, W), np.uint8)
    fdr[0::2, :] = E
    fdr[1::2, :] = W_
    fdr[0::2, -1] = S
    fdr[1::2, 0] = S
    fdr[-1, -1 if H % 2 else 0] = 0
    return fdr


@pytest.mark.parametrize("transposed", [False, True])
def test_serpentine(transposed):
    """one path through every cell of 128 x 192 (24,575 moves over 6 tiles, the seam crossed in every row): T is the
    reversed cumulative sum of q in path order and U the forward one, both computed here without the reference"""
    from descriptools_amd import flowpath as fp
    H, W = 128, 192
    fdr = _serpentine(H, W)
    order = np.arange(H * W).reshape(H, W)
    order[1::2] = order[1::2, ::-1]          # order[y, x] = the cell's position on the path
    if transposed:                           # the same path mirrored in the diagonal: E <-> S, W <-> N
        fdr = np.select([fdr.T == E, fdr.T == W_, fdr.T == S], [S, N, E], 0).astype(np.uint8)
        order = np.ascontiguousarray(order.T)
    cells = np.argsort(order.reshape(-1))    # cells[i] = the flat index of the path's i-th cell
    n = H * W
    rng = np.random.default_rng(3)
    top = np.full(fdr.shape, 1.999)          # every weight the largest the default scale allows for
    cases = [("random floats", rng.random(fdr.shape) * 3.0, None),
             ("all max", top, None),
             ("negative frac_bits", 1e9 * (0.5 + rng.random(fdr.shape)), -8),
             ("integers", rng.integers(0, 1000, fdr.shape, dtype=np.int32), 0)]
    for name, w, fb in cases:
        s = fp.path_frac_bits(w) if fb is None else fb
        q = np.rint(np.ldexp(np.asarray(w, np.float64), s)).astype(np.int64).reshape(-1)[cells]
        t_pos = np.r_[np.cumsum(q[:-1][::-1])[::-1], 0]       # the outlet's own weight is never counted
        u_pos = np.r_[0, np.cumsum(q[:-1])]
        assert int(t_pos[0]) <= 2 ** 52 and int(t_pos[0]) == int(u_pos[-1])
        if name == "all max":
            assert int(t_pos[0]) == (n - 1) * int(q[0]) > 2 ** 51  # 32-bit truncation or a lost carry would show
        want_t, want_u = np.empty(n, np.int64), np.empty(n, np.int64)
        want_t[cells], want_u[cells] = t_pos, u_pos
        _same(name + " T", fp.downstream_sum(fdr, w, frac_bits=fb),
              np.ldexp(want_t.astype(np.float64), -s).reshape(fdr.shape))
        _same(name + " U", fp.upslope_longest(fdr, w, frac_bits=fb),
              np.ldexp(want_u.astype(np.float64), -s).reshape(fdr.shape))


def _background(rng, H, W):
    """codes that only move east or down: no cycle"""
    return rng.choice(np.array([E, S, SE, SW], np.uint8), size=(H, W))


def _plant_pair(fdr, y, x):
    fdr[y, x], fdr[y, x + 1] = E, W_
    return [(y, x), (y, x + 1)]


def _plant_square(fdr, y, x):
    fdr[y, x], fdr[y, x + 1], fdr[y + 1, x + 1], fdr[y + 1, x] = E, S, W_, N
    return [(y, x), (y, x + 1), (y + 1, x + 1), (y + 1, x)]


@pytest.mark.parametrize("name, plant, at", [
    ("pair across a seam", _plant_pair, (10, 63)), ("pair in a tile", _plant_pair, (10, 20)),
    ("square round a corner", _plant_square, (63, 63)), ("square in a tile", _plant_square, (20, 20)),
])
def test_small_cycles(name, plant, at):
    rng = np.random.default_rng(sum(at))
    H, W = 100, 130
    fdr = _background(rng, H, W)
    cyc = plant(fdr, *at)
    w = rng.random((H, W)) * 5.0
    stop = rng.random((H, W)) < 0.01
    for c in cyc:
        stop[c] = False
    out = check(fdr, w, None, stop)
    into = WR.drainage(fdr)[0] < 0                        # the cycle and everything that drains into it
    assert into.sum() > len(cyc) and all(into[c] for c in cyc)
    for key in ("up", ("dn", False)):
        assert (out[key][into] == -100).all() and (out[key][~into] >= 0).all(), (name, key)
    stop[:] = False
    stop[cyc[-1]] = True                                  # a stop cell on the cycle
    out = check(fdr, w, None, stop)
    assert all(out["dn", True][c] >= 0 for c in cyc) and out["dn", True][cyc[-1]] == 0


@pytest.mark.parametrize("n", [130, 40])
def test_border_ring(n):
    """a D8 ring along the raster's border (n = 130: 516 cells over 9 tiles; n = 40: its in-tile twin) that the whole
    interior drains into: nothing has a value without a stop cell, everything has one with a stop cell on the ring"""
    rng = np.random.default_rng(n)
    fdr = np.full((n, n), N, np.uint8)
    fdr[0, :] = E
    fdr[:, -1] = S
    fdr[-1, :] = W_
    fdr[:, 0] = N
    fdr[0, 0], fdr[0, -1], fdr[-1, -1], fdr[-1, 0] = E, S, W_, N
    stop = np.zeros((n, n), np.int8)
    stop[n - 1, n // 2] = 1
    out = check(fdr, rng.random((n, n)) + 0.25, None, stop)
    assert (out["up"] == -100).all() and (out["dn", False] == -100).all()
    assert (out["dn", True] >= 0).all() and (out["dn", True] == 0).sum() == 1


@pytest.mark.parametrize("nodata", [False, True])
def test_random_fields(nodata):
    H, W = 200, 260
    fdr, dem = R.field(H, W, 17 + nodata, cycles=12, nodata=nodata)
    rng = np.random.default_rng(5)
    stop = (rng.random((H, W)) < 0.004).astype(np.int16) * 3
    if nodata:
        stop[dem == -100] = 1                                  # on nodata: ignored
    stop[np.argwhere(fdr == N)[0][0], np.argwhere(fdr == N)[0][1]] = 1
    out = check(fdr, rng.random((H, W)) * 40.0, dem, stop)
    t = out["dn", True]
    assert (t == -100).any() and (t > 0).any() and (out["up"] > 0).any() and (out["up"] == -100).any()
    zero = check(fdr, np.zeros((H, W)), dem, stop)
    for k in zero:
        np.testing.assert_array_equal(zero[k] == -100, out[k] == -100)
        assert (zero[k][zero[k] != -100] == 0).all()
    wide = np.ldexp(0.5 + rng.random((H, W)) / 2, rng.integers(0, 21, (H, W)))   # a 2^20 dynamic range
    check(fdr, wide, dem, stop)


def test_identities():
    from descriptools_amd import flowacc, flowdir, flowpath as fp, watershed as ws
    H, W = 200, 260
    rng = np.random.default_rng(8)
    cardinal = rng.choice(np.array([E, S], np.uint8), size=(H, W))   # acyclic, no diagonal move
    one = np.ones((H, W), np.uint8)
    np.testing.assert_array_equal(fp.downstream_sum(cardinal, one, frac_bits=0), ws.drainage(cardinal, 1.0).length)
    np.testing.assert_array_equal(fp.upslope_longest(cardinal, one, frac_bits=0), ws.upslope_length(cardinal, 1.0))
    # a conditioned DEM: every path reaches the edge
    sdem = oracle.synth_dem(13, 300, 280)
    fdr = flowdir.d8_conditioned(sdem, 10.0)
    w = rng.random(fdr.shape) * 7.0
    s = fp.path_frac_bits(w)
    q = R.quantise(w, s).reshape(-1)
    T, U = fp.downstream_sum(fdr, w), fp.upslope_longest(fdr, w)
    assert (T >= 0).all() and (U >= 0).all()
    Ti, Ui = np.ldexp(T, s).astype(np.int64).reshape(-1), np.ldexp(U, s).astype(np.int64).reshape(-1)
    np.testing.assert_array_equal(np.ldexp(Ti.astype(np.float64), -s), T.reshape(-1))
    M = Ti.copy()                                                  # the upslope max of T, by walking every source's path
    for cells, src, _, _ in R.walk_paths(fdr, q, None, None, R.sources(fdr, None, np.ones(fdr.size, bool))):
        np.maximum.at(M, cells, Ti[src])
    np.testing.assert_array_equal(Ui + Ti, M)
    acc = flowacc.accumulate(fdr).reshape(-1)
    moving = WR.graph(fdr)[1] >= 0
    assert sum(int(t) for t in Ti) == sum(int(a) * (int(b) + 1) for a, b in zip(q[moving], acc[moving]))
    # two runs give the same bits
    np.testing.assert_array_equal(fp.downstream_sum(fdr, w), T)
    np.testing.assert_array_equal(fp.upslope_longest(fdr, w), U)


def test_device_tier_contract():
    """on a Chain's own fdr the device tier equals the host tier and the reference; a dt_dev_upslope_length and a
    dt_dev_flowpath_upslope between two calls of ours (both take the context's scratch) do not disturb them; a NULL
    out leaves sentinel-filled buffers alone; a bad frac_bits is refused with its message; 0 x 0 succeeds"""
    from descriptools_amd import _lib, chain, device, flowpath as fp
    H, W = 320, 384
    dem = oracle.synth_dem(7, H, W)
    rng = np.random.default_rng(12)
    w = rng.random((H, W)) * 3.0 + 0.01
    s = fp.path_frac_bits(w)
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=10.0, overlap=False, tune_placement=False, river_threshold=200)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float32))
    w_d = ctx.to_device(w)
    t_d, u_d = ctx.empty((H, W), np.float64), ctx.empty((H, W), np.float64)
    keep = ctx.to_device(np.full((H, W), 12345.0, np.float64))
    len_d = ctx.empty((H, W), np.float64)
    v_d = ctx.empty((H, W), np.float32)
    L = _lib.lib()
    held = [d, w_d, t_d, u_d, keep, len_d, v_d]
    try:
        ch.run(d.ptr)
        f, hp = ch.p("fdr"), ctx.h
        fdr = ch.buf["fdr"].to_host()
        river = (ch.buf["river"].to_host() != 0).astype(np.uint8)
        r_d = ctx.to_device(river)
        held.append(r_d)
        runs = []
        for _ in range(2):
            _lib.check(L.dt_dev_flowpath_downstream_sum(hp, f, None, w_d.ptr, r_d.ptr, H, W, s, t_d.ptr))
            _lib.check(L.dt_dev_upslope_length(hp, f, None, H, W, 10.0, len_d.ptr))
            _lib.check(L.dt_dev_flowpath_upslope_longest(hp, f, None, w_d.ptr, H, W, s, u_d.ptr))
            _lib.check(L.dt_dev_flowpath_upslope(hp, f, None, d.ptr, H, W, 1, v_d.ptr, None))
            ctx.sync()
            runs.append((t_d.to_host(), u_d.to_host()))
        # a NULL out launches nothing (the scratch-using calls around it are undisturbed)
        _lib.check(L.dt_dev_flowpath_downstream_sum(hp, f, None, w_d.ptr, r_d.ptr, H, W, s, None))
        _lib.check(L.dt_dev_flowpath_upslope_longest(hp, f, None, w_d.ptr, H, W, s, None))
        ctx.sync()
        assert (keep.to_host() == 12345.0).all()
        np.testing.assert_array_equal(t_d.to_host(), runs[0][0])
        np.testing.assert_array_equal(u_d.to_host(), runs[0][1])
        # refusals
        for bad in (2201, -2201, 1 << 20):
            assert L.dt_dev_flowpath_downstream_sum(hp, f, None, w_d.ptr, None, H, W, bad, t_d.ptr) != 0
            assert b"frac_bits" in L.dt_last_error()
            assert L.dt_dev_flowpath_upslope_longest(hp, f, None, w_d.ptr, H, W, bad, u_d.ptr) != 0
            assert b"frac_bits" in L.dt_last_error()
        assert L.dt_dev_flowpath_downstream_sum(hp, None, None, None, None, 0, 0, 0, None) == 0
        assert L.dt_dev_flowpath_upslope_longest(hp, None, None, None, 0, 0, 0, None) == 0
        ctx.sync()
        np.testing.assert_array_equal(t_d.to_host(), runs[0][0])      # a refused call wrote nothing
    finally:
        for b in held:
            b.free()
        ch.free()
        ctx.close()
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)
    _same("device down", runs[0][0], fp.downstream_sum(fdr, w, stop=river))
    _same("device up", runs[0][1], fp.upslope_longest(fdr, w))
    _same("reference down", runs[0][0], R.downstream_sum(fdr, w, None, river))
    _same("reference up", runs[0][1], R.upslope_longest(fdr, w))
    assert (runs[0][0] == -100).any() and (runs[0][0] > 0).any()


@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf, 2.0 ** 50])
def test_the_library_refuses_a_weight_outside_the_contract(bad):
    """past the Python checks, through the C ABI: a weight that is negative, not finite or over the bound of frac_bits
    (70 * 2^50 > 2^52) is reported wherever it lies, here on a terminal, and a good call after it succeeds"""
    from descriptools_amd import _lib
    from descriptools_amd._lib import c_f64p, c_u8p, ptr
    L = _lib.lib()
    fdr = np.full((7, 10), E, np.uint8)
    w = np.ones((7, 10), np.float64)
    out = np.empty((7, 10), np.float64)
    w[3, 9] = bad
    assert L.dt_flowpath_downstream_sum(ptr(fdr, c_u8p), None, ptr(w, c_f64p), None, 7, 10, 0, ptr(out, c_f64p)) != 0
    assert b"weight" in L.dt_last_error()
    assert L.dt_flowpath_upslope_longest(ptr(fdr, c_u8p), None, ptr(w, c_f64p), 7, 10, 0, ptr(out, c_f64p)) != 0
    assert b"weight" in L.dt_last_error()
    w[3, 9] = 1.0
    _lib.check(L.dt_flowpath_downstream_sum(ptr(fdr, c_u8p), None, ptr(w, c_f64p), None, 7, 10, 0, ptr(out, c_f64p)))
    np.testing.assert_array_equal(out, np.tile(np.arange(9.0, -1.0, -1.0), (7, 1)))


def test_travel_time_and_time_of_concentration():
    """a 256^2 conditioned rough DEM with a nodata block, a speed derived from the slope along the path, and the
    river as the stop mask, against the reference on the same weights"""
    from descriptools_amd import flowacc, flowpath as fp
    n, px = 256, 10.0
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:n, 0:n]
    dem = (0.02 * yy + 0.01 * xx + rng.random((n, n)) * 1.0 + 5.0).astype(np.float32)
    dem[n // 3:n // 3 + 20, n // 2:n // 2 + 35] = -100
    fdr, filled = oracle.condition_d8(dem, px)
    valid, succ, _ = WR.graph(fdr, dem)
    step = R.step_length(fdr, px, dem).reshape(-1)
    z = filled.reshape(-1).astype(np.float64)
    slope = np.zeros(n * n)
    mv = succ >= 0
    slope[mv] = np.maximum(z[mv] - z[succ[mv]], 0.0) / step[mv]
    speed = (0.1 + 2.0 * np.sqrt(slope)).reshape(n, n)
    speed[~valid.reshape(n, n)] = np.nan                           # not looked at
    speed[(~mv & valid).reshape(n, n)] = -1.0                      # terminals: not looked at either
    river = flowacc.accumulate(fdr, dem) > 150
    assert river.sum() > 50
    wt = np.zeros(n * n)
    wt[mv] = step[mv] / speed.reshape(-1)[mv]
    wt = wt.reshape(n, n)
    np.testing.assert_array_equal(fp.step_length(fdr, px, dem), step.reshape(n, n))
    tt = fp.travel_time(fdr, px, speed, dem, stop=river)
    _same("travel_time", tt, R.downstream_sum(fdr, wt, dem, river))
    _same("travel_time to the outlet", fp.travel_time(fdr, px, speed, dem), R.downstream_sum(fdr, wt, dem))
    tc = fp.time_of_concentration(fdr, px, speed, dem)
    _same("time_of_concentration", tc, R.upslope_longest(fdr, wt, dem))
    assert (tt[river & valid.reshape(n, n)] == 0).all() and (tt > 0).any() and (tt == -100).any()
    assert (tc[valid.reshape(n, n)] >= 0).all() and (tc[~valid.reshape(n, n)] == -100).all() and tc.max() > 100
