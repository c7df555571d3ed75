"""GPU (-m gpu): flowpath.upslope_extreme / downstream_extreme and flowdir.d8_carved (dt_flowpath_*, dt_carve and the
device tier; k_fp_* and k_carve_blend in dt_flowpath.hip) against the pure-numpy reference (tests/_flowpath_ref.py).
Everything is compared with assert_array_equal, NaN positions and `where` included: nothing here has a tolerance,
because no arithmetic touches a value (the carving's one subtraction is the same float32 operation on both sides).

Hand-built cases through both tiers, degenerate shapes, a serpentine path through every cell of six tiles with closed
forms, D8 cycles across tile seams with their in-tile twins, random fields with cycles, nodata, ties and NaN, carving
on a rough DEM and on the bundled Example, identities, and the device tier's contract."""
import numpy as np
import pytest

import oracle
from conftest import load_example

import _flowpath_ref as R
import _watershed_ref as WR
from _watershed_ref import E, N, S, SE, SW, W_

pytestmark = pytest.mark.gpu

KINDS = ("max", "min")


def _same(name, got, want):
    for g, w, part in zip(got, want, ("value", "where")):
        assert g.dtype == w.dtype, (name, part)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (name, part))
    assert not np.signbit(got[0][got[0] == 0]).any(), name  # -0.0 comes back as +0.0


def check(fdr, values, dem=None, stop=None, kinds=KINDS):
    """both folds, with where, for each kind (and with and without `stop` when one is given) against the reference;
    the value alone must equal the value beside where.  Returns {(fold, kind, stopped): (value, where)}"""
    from descriptools_amd import flowpath as fp
    out = {}
    for kind in kinds:
        ref = R.upslope(fdr, values, kind, dem)
        got = fp.upslope_extreme(fdr, values, kind, dem, where=True)
        _same("upslope " + kind, got, ref)
        alone = fp.upslope_extreme(fdr, values, kind, dem)
        assert alone.where is None
        np.testing.assert_array_equal(alone.value, ref[0])
        out["up", kind, False] = ref
        for st in ((None,) if stop is None else (None, stop)):
            ref = R.downstream(fdr, values, kind, dem, st)
            _same("downstream %s stop=%s" % (kind, st is not None),
                  fp.downstream_extreme(fdr, values, kind, dem, st, where=True), ref)
            np.testing.assert_array_equal(fp.downstream_extreme(fdr, values, kind, dem, st).value, ref[0])
            out["dn", kind, st is not None] = ref
    return out


class Dev:
    """the device tier on host arrays: uploads, calls, downloads"""

    def __init__(self):
        from descriptools_amd import _lib, device
        self.lib, self.L, self.ctx = _lib, _lib.lib(), device.Context()

    def close(self):
        self.ctx.close()

    def run(self, fold, fdr, values, kind, dem=None, stop=None):
        H, W = fdr.shape
        held = [self.ctx.to_device(np.ascontiguousarray(fdr, np.uint8)),
                self.ctx.to_device(np.ascontiguousarray(values, np.float32))]
        d = s = None
        if dem is not None:
            held.append(self.ctx.to_device(self.lib.nodata_mask(dem, fdr.shape)))
            d = held[-1].ptr
        if stop is not None:
            held.append(self.ctx.to_device(np.ascontiguousarray(np.asarray(stop) != 0, np.uint8)))
            s = held[-1].ptr
        v, w = self.ctx.empty((H, W), np.float32), self.ctx.empty((H, W), np.int64)
        held += [v, w]
        k = KINDS.index(kind)
        try:
            if fold == "up":
                self.lib.check(self.L.dt_dev_flowpath_upslope(self.ctx.h, held[0].ptr, d, held[1].ptr, H, W, k, v.ptr,
                                                              w.ptr))
            else:
                self.lib.check(self.L.dt_dev_flowpath_downstream(self.ctx.h, held[0].ptr, d, held[1].ptr, s, H, W, k,
                                                                 v.ptr, w.ptr))
            self.ctx.sync()
            return v.to_host(), w.to_host()
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
    fdr, values, kind, dem, stop = c["fdr"], c["values"], c["kind"], c["dem"], c["stop"]
    _same("host up", fp.upslope_extreme(fdr, values, kind, dem, where=True), c["up"])
    _same("host down", fp.downstream_extreme(fdr, values, kind, dem, stop, where=True), c["dn"])
    _same("device up", dev.run("up", fdr, values, kind, dem), c["up"])
    _same("device down", dev.run("dn", fdr, values, kind, dem, stop), c["dn"])


def _values(rng, shape, nan=0.05, levels=7):
    """quantised to `levels` values (many ties), with NaN"""
    v = rng.integers(-(levels // 2), levels - levels // 2, shape).astype(np.float32)
    v[rng.random(shape) < nan] = np.nan
    return v


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (64, 64), (65, 129), (130, 67), (0, 0), (0, 9), (9, 0)])
def test_shapes(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    fdr = rng.choice(np.array([E, W_, S, N, SE, 0], np.uint8), size=shape)
    if shape[0] == 1:
        fdr[:] = E
    if shape[1] == 1:
        fdr[:] = S
    stop = rng.random(shape) < 0.02
    check(fdr, _values(rng, shape), None, stop)


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
    """one path through every cell of 128 x 192 (24,575 moves over 6 tiles, the seam crossed in every row): the
    upslope extreme is the running extreme in path order, the downstream one the running extreme of the reversed path,
    both computed here without the reference"""
    from descriptools_amd import flowpath as fp
    H, W = 128, 192
    fdr = _serpentine(H, W)
    order = np.arange(H * W).reshape(H, W)
    order[1::2] = order[1::2, ::-1]          # order[y, x] = the cell's position on the path
    if transposed:                           # the same path mirrored in the diagonal: E <-> S, W <-> N
        fdr = np.select([fdr.T == E, fdr.T == W_, fdr.T == S], [S, N, E], 0).astype(np.uint8)
        order = np.ascontiguousarray(order.T)
    cells = np.argsort(order.reshape(-1))    # cells[i] = the flat index of the path's i-th cell
    rng = np.random.default_rng(3)
    # a rise and a fall along the path plus noise, in whole numbers: many ties, and a running extreme that keeps moving
    values = (20 - np.abs(order * 40 // (H * W) - 20) + rng.integers(0, 3, fdr.shape)).astype(np.float32)
    v = values.reshape(-1)[cells]

    def running(vals, idx, kind):
        """per position i the best (value, then smallest flat index) among positions 0..i"""
        best_v, best_i = [], []
        bv, bi = vals[0], idx[0]
        for x, i in zip(vals.tolist(), idx.tolist()):
            if (x > bv if kind == "max" else x < bv) or (x == bv and i < bi):
                bv, bi = x, i
            best_v.append(bv)
            best_i.append(bi)
        return np.array(best_v, np.float32), np.array(best_i, np.int64)

    for kind in KINDS:
        for fold in ("up", "dn"):
            if fold == "up":
                pv, pi = running(v, cells, kind)
                got = fp.upslope_extreme(fdr, values, kind, where=True)
            else:
                pv, pi = running(v[::-1], cells[::-1], kind)
                pv, pi = pv[::-1], pi[::-1]
                got = fp.downstream_extreme(fdr, values, kind, where=True)
            want_v, want_w = np.empty(H * W, np.float32), np.empty(H * W, np.int64)
            want_v[cells], want_w[cells] = pv, pi
            _same("%s %s" % (fold, kind), got, (want_v.reshape(fdr.shape), want_w.reshape(fdr.shape)))
    assert np.unique(fp.upslope_extreme(fdr, values, "max").value).size > 10
    assert np.unique(fp.downstream_extreme(fdr, values, "max").value).size > 10


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
    values = _values(rng, (H, W))
    values[at[0] - 5, at[1]] = 50.0           # a cell above the cycle that may or may not drain into it
    stop = rng.random((H, W)) < 0.01
    stop[cyc[0]] = False
    out = check(fdr, values, None, stop)
    for key, (val, whr) in out.items():
        on = [(val[c], whr[c]) for c in cyc]
        if key[0] == "up" or not key[2]:
            assert all(o == on[0] or (np.isnan(o[0]) and np.isnan(on[0][0])) for o in on), (name, key, on)
    stop[:] = False
    stop[cyc[-1]] = True                      # a stop cell on the cycle
    check(fdr, values, None, stop)


@pytest.mark.parametrize("n", [130, 40])
def test_border_ring(n):
    """a D8 ring along the raster's border (n = 130: 516 cells over 9 tiles; n = 40: its in-tile twin) that the whole
    interior drains into, with the extreme placed on a tributary: every ring cell holds it upslope"""
    rng = np.random.default_rng(n)
    fdr = np.full((n, n), N, np.uint8)
    fdr[0, :] = E
    fdr[:, -1] = S
    fdr[-1, :] = W_
    fdr[:, 0] = N
    fdr[0, 0], fdr[0, -1], fdr[-1, -1], fdr[-1, 0] = E, S, W_, N
    values = _values(rng, (n, n))
    values[n // 2, n // 3] = 99.0
    values[n // 3, n // 2] = -99.0
    ring = np.zeros((n, n), bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    assert ring.sum() == 4 * (n - 1)
    stop = np.zeros((n, n), np.int8)
    stop[n - 1, n // 2] = 1
    out = check(fdr, values, None, stop)
    for kind, v, cell in (("max", 99.0, (n // 2, n // 3)), ("min", -99.0, (n // 3, n // 2))):
        val, whr = out["up", kind, False]
        assert (val[ring] == v).all() and (whr[ring] == cell[0] * n + cell[1]).all()
        val, whr = out["dn", kind, False]
        assert np.unique(val[ring]).size == 1 and np.unique(whr[ring]).size == 1
        assert not np.isnan(out["dn", kind, True][0]).any()


def _field(H, W, seed, cycles, nodata=False):
    """test_gpu_watershed.py's generator: random codes, planted 2 x 2 cycles, a long cycle across tiles, nodata"""
    rng = np.random.default_rng(seed)
    fdr = rng.choice(np.array([SW, S, SE, E], np.uint8), size=(H, W))
    fdr[rng.random((H, W)) < 0.002] = rng.choice(np.array([0, 3, 255], np.uint8))
    noisy = rng.random((H, W)) < 0.05
    fdr[noisy] = rng.choice(np.array([1, 2, 4, 8, 16, 32, 64, 128], np.uint8), size=int(noisy.sum()))
    for _ in range(cycles):
        y, x = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
        fdr[y, x], fdr[y, x + 1], fdr[y + 1, x + 1], fdr[y + 1, x] = E, S, W_, N
    y0, x0 = H // 3, W // 4
    fdr[y0, x0:x0 + 150] = E
    fdr[y0:y0 + 90, x0 + 150] = S
    fdr[y0 + 90, x0 + 1:x0 + 151] = W_
    fdr[y0 + 1:y0 + 91, x0] = N
    dem = None
    if nodata:
        dem = rng.random((H, W)).astype(np.float32) * 50
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(6):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(5, 40)
            dem[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = -100
        dem[rng.random((H, W)) < 0.01] = -150
    return fdr, dem


@pytest.mark.parametrize("nodata", [False, True])
def test_random_fields(nodata):
    H, W = 200, 260
    fdr, dem = _field(H, W, 17 + nodata, cycles=12, nodata=nodata)
    rng = np.random.default_rng(5)
    values = _values(rng, (H, W))
    stop = (rng.random((H, W)) < 0.004).astype(np.int16) * 3
    if nodata:
        stop[dem == -100] = 1                                  # on nodata: ignored
    stop[np.argwhere(fdr == N)[0][0], np.argwhere(fdr == N)[0][1]] = 1
    out = check(fdr, values, dem, stop)
    val = out["dn", "max", True][0]
    assert np.isnan(val).any() and (~np.isnan(val)).any()
    check(fdr, np.full((H, W), np.nan, np.float32), dem, stop, kinds=("max",))
    out = check(fdr, np.full((H, W), 2.5, np.float32), dem, stop, kinds=("min",))
    valid = np.ones((H, W), bool) if dem is None else dem > -100
    assert (out["up", "min", False][0][valid] == 2.5).all() and (out["dn", "min", False][0][valid] == 2.5).all()


def _rough_dem(n, seed):
    """a trend plus unit noise (a pit at most cells, as LiDAR behind embankments), with a nodata block"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    dem = (0.02 * yy + 0.01 * xx + rng.random((n, n)) * 1.0 + 5.0).astype(np.float32)
    dem[n // 3:n // 3 + 20, n // 2:n // 2 + 35] = -100
    return dem


@pytest.fixture(scope="module")
def rough():
    dem = _rough_dem(256, 21)
    fdr, filled = oracle.condition_d8(dem, 10.0)
    lowest = R.upslope(fdr, dem, "min", dem)[0]
    target = WR.drainage(fdr, 10.0, dem)[0]
    return dem, fdr, filled, lowest, target


def _edges(fdr, dem):
    valid, succ, _ = WR.graph(fdr, dem)
    c = np.flatnonzero(succ >= 0)
    return c, succ[c]


@pytest.mark.parametrize("max_cut", [None, 0, 0.5, 2])
def test_carved(rough, max_cut):
    from descriptools_amd import flowdir
    dem, fdr_o, filled_o, lowest, target = rough
    valid = dem > -100
    fdr, carved, filled = flowdir.d8_carved(dem, 10.0, max_cut, return_filled=True)
    np.testing.assert_array_equal(fdr, fdr_o)
    np.testing.assert_array_equal(filled, filled_o)
    want = lowest if max_cut is None else np.maximum(lowest, filled_o - np.float32(max_cut))
    want = np.where(valid, want, dem).astype(np.float32)
    assert carved.dtype == np.float32
    np.testing.assert_array_equal(carved, want)
    np.testing.assert_array_equal(carved, R.carved(dem, 10.0, max_cut)[1])
    np.testing.assert_array_equal(flowdir.d8_carved(dem, 10.0, max_cut)[1], carved)
    if max_cut == 0:
        np.testing.assert_array_equal(carved, filled)
    if max_cut is None:
        np.testing.assert_array_equal(flowdir.d8_carved(dem, 10.0, np.inf)[1], carved)
    assert (carved[valid] <= filled[valid]).all() and (carved[~valid] == dem[~valid]).all()
    a, b = _edges(fdr, dem)
    flat = carved.reshape(-1)
    assert (flat[a] >= flat[b]).all()                            # non-increasing along every edge
    tg = target.reshape(-1)
    ok = tg >= 0
    assert ok[valid.reshape(-1)].all()
    assert (flat[ok] - flat[tg[ok]] >= 0).all()                  # no negative height above the outlet
    raw = dem.reshape(-1)
    assert (raw[ok] - raw[tg[ok]]).min() < 0                     # which the raw DEM has: the case's reason
    if max_cut is None:
        assert (carved < dem).sum() > 1000 and (filled > dem).sum() > 1000


def test_carved_refuses_a_nan_height(rough):
    from descriptools_amd import flowdir
    bad = rough[0].copy()
    bad[100, 100] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        flowdir.d8_carved(bad, 10.0)


def test_carved_example():
    """a 512 x 512 window of the bundled Example: carved <= dem, and the reference"""
    from descriptools_amd import flowdir
    dem = np.ascontiguousarray(load_example()[0][:512, :512], np.float32)
    fdr, carved = flowdir.d8_carved(dem, 30.0)
    valid = dem > -100
    assert valid.sum() > 1000
    assert (carved[valid] <= dem[valid]).all()
    fdr_r, carved_r, _ = R.carved(dem, 30.0)
    np.testing.assert_array_equal(fdr, fdr_r)
    np.testing.assert_array_equal(carved, carved_r)


def test_identities():
    from descriptools_amd import flowacc, flowdir, flowpath as fp, watershed as ws
    H, W = 200, 260
    fdr, dem = _field(H, W, 31, cycles=8, nodata=True)
    valid = dem > -100
    one = fp.upslope_extreme(fdr, np.ones((H, W), np.float32), "max", dem).value
    assert (one[valid] == 1).all() and np.isnan(one[~valid]).all()
    # an acyclic field: the position itself as the value
    rng = np.random.default_rng(8)
    acyclic = _background(rng, H, W)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    d = fp.downstream_extreme(acyclic, idx, "max", where=True)
    np.testing.assert_array_equal(d.where, d.value.astype(np.int64))
    np.testing.assert_array_equal(d.where, ws.drainage(acyclic).target)  # every move goes to a larger index
    pour = (rng.random((H, W)) < 0.01).astype(np.int64)
    s = fp.downstream_extreme(acyclic, idx, "max", stop=pour > 0)
    assert (s.value[pour > 0] == idx[pour > 0]).all()
    tg = ws.drainage(acyclic, pour_points=pour).target
    np.testing.assert_array_equal(np.where(tg >= 0, tg, -1), np.where(np.isnan(s.value), -1, s.value).astype(np.int64))
    # accumulation grows along every path of a conditioned DEM: its downstream maximum is the outlet's
    sdem = oracle.synth_dem(13, 300, 280)
    cfdr = flowdir.d8_conditioned(sdem, 10.0)
    acc = flowacc.accumulate(cfdr)
    assert acc.max() < 2 ** 24
    m = fp.downstream_extreme(cfdr, acc, "max").value
    t = ws.drainage(cfdr).target
    assert (t >= 0).all()
    np.testing.assert_array_equal(m, acc.reshape(-1)[t].astype(np.float32))


def test_device_tier_contract():
    """on a Chain's own fdr the device tier equals the host tier; NULL outputs are left alone; a bad kind and a
    non-finite max_cut are refused with a message; two runs give the same bits; a dt_dev_upslope_length between two
    calls of ours (it takes the context's scratch) does not disturb them; dt_dev_carve_blend in place"""
    from descriptools_amd import _lib, chain, device, flowdir, flowpath as fp
    H, W = 320, 384
    dem = oracle.synth_dem(7, H, W)
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=10.0, overlap=False, tune_placement=False, river_threshold=200)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float32))
    v_d, w_d = ctx.empty((H, W), np.float32), ctx.empty((H, W), np.int64)
    keep_v = ctx.to_device(np.full((H, W), 12345.0, np.float32))
    keep_w = ctx.to_device(np.full((H, W), -777, np.int64))
    len_d = ctx.empty((H, W), np.float64)
    L = _lib.lib()
    held = [d, v_d, w_d, keep_v, keep_w, len_d]
    try:
        ch.run(d.ptr)
        f, hp = ch.p("fdr"), ctx.h
        fdr = ch.buf["fdr"].to_host()
        river = (ch.buf["river"].to_host() != 0).astype(np.uint8)
        r_d = ctx.to_device(river)
        held.append(r_d)
        runs = []
        for _ in range(2):
            _lib.check(L.dt_dev_flowpath_upslope(hp, f, None, d.ptr, H, W, 1, v_d.ptr, w_d.ptr))
            ctx.sync()
            up = (v_d.to_host(), w_d.to_host())
            _lib.check(L.dt_dev_upslope_length(hp, f, None, H, W, 10.0, len_d.ptr))
            _lib.check(L.dt_dev_flowpath_downstream(hp, f, None, d.ptr, r_d.ptr, H, W, 0, v_d.ptr, w_d.ptr))
            ctx.sync()
            runs.append(up + (v_d.to_host(), w_d.to_host()))
        # NULL outputs: only the other is written
        _lib.check(L.dt_dev_flowpath_upslope(hp, f, None, d.ptr, H, W, 1, None, w_d.ptr))
        _lib.check(L.dt_dev_flowpath_downstream(hp, f, None, d.ptr, None, H, W, 0, v_d.ptr, None))
        _lib.check(L.dt_dev_flowpath_upslope(hp, f, None, d.ptr, H, W, 0, None, None))
        ctx.sync()
        w_only, v_only = w_d.to_host(), v_d.to_host()
        assert (keep_v.to_host() == 12345.0).all() and (keep_w.to_host() == -777).all()
        # refusals
        for bad in (2, -1):
            assert L.dt_dev_flowpath_upslope(hp, f, None, d.ptr, H, W, bad, v_d.ptr, None) != 0
            assert b"kind" in L.dt_last_error()
            assert L.dt_dev_flowpath_downstream(hp, f, None, d.ptr, None, H, W, bad, v_d.ptr, None) != 0
            assert b"kind" in L.dt_last_error()
        for bad in (float("nan"), float("inf"), -1.0):
            assert L.dt_dev_carve_blend(hp, d.ptr, d.ptr, d.ptr, H, W, bad, v_d.ptr) != 0
            assert b"max_cut" in L.dt_last_error()
        assert L.dt_dev_flowpath_upslope(hp, None, None, None, 0, 0, 0, None, None) == 0
        # the blend in place: carved aliases lowest
        fdr_c, filled = flowdir.d8_conditioned(dem, 10.0, return_filled=True)
        fc_d, fl_d = ctx.to_device(fdr_c), ctx.to_device(filled)
        held += [fc_d, fl_d]
        _lib.check(L.dt_dev_flowpath_upslope(hp, fc_d.ptr, d.ptr, d.ptr, H, W, 1, v_d.ptr, None))
        _lib.check(L.dt_dev_carve_blend(hp, d.ptr, fl_d.ptr, v_d.ptr, H, W, 0.5, v_d.ptr))
        ctx.sync()
        blended = v_d.to_host()
    finally:
        for b in held:
            b.free()
        ch.free()
        ctx.close()
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)
    demf = np.ascontiguousarray(dem, np.float32)
    host_up = fp.upslope_extreme(fdr, demf, "min", where=True)
    host_dn = fp.downstream_extreme(fdr, demf, "max", stop=river, where=True)
    _same("device up", runs[0][:2], host_up)
    _same("device down", runs[0][2:], host_dn)
    _same("reference up", runs[0][:2], R.upslope(fdr, demf, "min"))
    _same("reference down", runs[0][2:], R.downstream(fdr, demf, "max", None, river))
    np.testing.assert_array_equal(w_only, host_up.where)
    np.testing.assert_array_equal(v_only, fp.downstream_extreme(fdr, demf, "max").value)
    np.testing.assert_array_equal(blended, flowdir.d8_carved(dem, 10.0, 0.5)[1])
