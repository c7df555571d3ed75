"""GPU (-m gpu): weighted flow accumulation (flowacc.accumulate_weighted, dt_flowacc_weighted, dt_dev_flowacc_weighted;
k_faw_* in dt_tiles.hip).  Weights of 1 reproduce the count bit for bit; float64, float32 and integer weights match a
numpy int64 fixed-point reference bit for bit; sums near 2^52 stay exact; runs and tiers agree; a bad weight on the
device tier raises DT_STATUS_BAD_WEIGHT and leaves the context usable.  Fields run on a width the count path's fused
last pass takes (1024) and on one it does not (1000)."""
import ctypes

import numpy as np
import pytest

import oracle

from _flowacc_weighted_ref import reference

pytestmark = pytest.mark.gpu

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
DT_STATUS_BAD_WEIGHT = 4
_DY = {E: 0, SE: 1, S: 1, SW: 1, W_: 0, NW: -1, N: -1, NE: -1}
_DX = {E: 1, SE: 1, S: 0, SW: -1, W_: -1, NW: -1, N: 0, NE: 1}


def expected(fdr, w, dem=None, s=None):
    from descriptools_amd import flowacc
    w64 = np.asarray(w, np.float64)
    if s is None:
        s = flowacc.weight_frac_bits(w64)
    q = np.rint(np.ldexp(w64, s))
    sums, dead = reference(fdr, q, dem)
    return np.where(dead, -100.0, np.ldexp(sums.astype(np.float64), -s))


def _south(rng, H, W):
    fdr = np.full((H, W), S, np.uint8)
    fdr[rng.random((H, W)) < 0.2] = SE
    fdr[rng.random((H, W)) < 0.2] = SW
    return fdr


def _cycles(W):
    H = 192
    fdr = _south(np.random.default_rng(W), H, W)
    fdr[63, 63], fdr[63, 64], fdr[64, 64], fdr[64, 63] = E, S, W_, N      # four tiles
    fdr[20, 40:90] = E                                                   # two tiles
    fdr[20:30, 90] = S
    fdr[30, 41:91] = W_
    fdr[21:31, 40] = N
    return fdr, None


def _feeders(W):
    H = 192
    fdr = np.full((H, W), S, np.uint8)
    fdr[63, 64:128] = S
    fdr[63, 63], fdr[63, 128] = SE, SW
    fdr[64:128, 63] = E
    fdr[64:128, 128] = W_
    fdr[128, 64:128] = N
    fdr[128, 63], fdr[128, 128] = NE, NW
    fdr[63, 65], fdr[65, 63] = SW, NE
    fdr[64:127, 64:128] = S
    fdr[127, 64:96] = E
    fdr[127, 97:128] = W_
    fdr[127, 96] = S
    fdr[128, 96] = S
    return fdr, None


def _random(W):
    rng = np.random.default_rng(7 + W)
    codes = np.array([E, SE, S, SW, W_, NW, N, NE, 0, 3], np.uint8)   # 0 and 3: no successor
    fdr = codes[rng.integers(0, 10, size=(256, W))]
    dem = np.zeros(fdr.shape, np.float32)
    dem[100:120, 30:70] = -100.0
    dem[rng.random(fdr.shape) < 0.01] = -150.0
    return fdr, dem


def _terrain(W):
    dem = oracle.synth_dem(5, 320, W, 0, 0, 320, W, 3)
    _, fdr = oracle.slope_d8(dem, 10.0)
    return fdr, dem


FIELDS = {"cycles": _cycles, "feeders": _feeders, "random": _random, "terrain": _terrain}


def test_reference_counts_like_the_oracle():
    """the test's own reference, with unit weights, is the oracle's count"""
    for make in FIELDS.values():
        fdr, dem = make(200)
        sums, dead = reference(fdr, np.ones(fdr.shape), dem)
        got = np.where(dead, -100, sums)
        assert np.array_equal(got, oracle.flowacc(fdr, dem))


@pytest.mark.parametrize("W", [1024, 1000])
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_ones_equal_the_count(field, W):
    from descriptools_amd import flowacc
    fdr, dem = FIELDS[field](W)
    count = flowacc.accumulate(fdr, dem).astype(np.float64)
    got = flowacc.accumulate_weighted(fdr, np.ones(fdr.shape), dem)
    assert got.dtype == np.float64
    assert np.array_equal(got.view(np.int64), count.view(np.int64)), int((got != count).sum())
    assert np.array_equal(count, oracle.flowacc(fdr, dem).astype(np.float64))


@pytest.mark.parametrize("shape", [(1, 1000), (1, 1024), (1000, 1), (1, 1), (67, 131), (129, 65), (2, 3)])
def test_ones_equal_the_count_thin_and_odd(shape):
    from descriptools_amd import flowacc
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    codes = np.array([E, SE, S, SW, W_, NW, N, NE], np.uint8)
    for fdr in (codes[rng.integers(0, 8, size=shape)], np.full(shape, E if shape[1] > 1 else S, np.uint8)):
        count = flowacc.accumulate(fdr).astype(np.float64)
        got = flowacc.accumulate_weighted(fdr, np.ones(shape, np.int32))
        assert np.array_equal(got, count)


def _check_exact(fdr, w, dem=None, frac_bits=None):
    from descriptools_amd import flowacc
    got = flowacc.accumulate_weighted(fdr, w, dem, frac_bits=frac_bits)
    want = expected(fdr, w, dem, frac_bits)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), int((got != want).sum())
    return got


@pytest.mark.parametrize("W", [1024, 1000])
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_exact_against_the_fixed_point_reference(field, W):
    from descriptools_amd import flowacc
    fdr, dem = FIELDS[field](W)
    rng = np.random.default_rng(W + len(field))
    w64 = rng.random(fdr.shape) * 3.7
    w64[rng.random(fdr.shape) < 0.1] = 0.0
    got = _check_exact(fdr, w64, dem)
    # within n_upstream * 2^-(s+1) of a plain float64 sum (which has rounding of its own: a relative 1e-12)
    s = flowacc.weight_frac_bits(w64)
    count = flowacc.accumulate(fdr, dem)
    f64 = _float_sums(fdr, w64, dem)
    ok = count >= 0
    assert np.array_equal(got < 0, ~ok)
    tol = count[ok] * 2.0 ** -(s + 1) + 1e-12 * np.abs(f64[ok])
    assert (np.abs(got[ok] - f64[ok]) <= tol).all()
    _check_exact(fdr, w64.astype(np.float32), dem)
    wi = rng.integers(0, 1000, size=fdr.shape).astype(np.int32)
    got_i = _check_exact(fdr, wi, dem, frac_bits=0)
    sums, dead = reference(fdr, wi, dem)
    assert np.array_equal(got_i, np.where(dead, -100.0, sums.astype(np.float64)))


def _float_sums(fdr, w, dem):
    """plain float64 accumulation (peeling order), for the error bound"""
    H, Wd = fdr.shape
    acc = np.zeros(H * Wd)
    f = fdr.reshape(-1)
    y, x = np.divmod(np.arange(H * Wd), Wd)
    succ = np.full(H * Wd, -1, np.int64)
    for code in _DY:
        m = f == code
        ty, tx = y[m] + _DY[code], x[m] + _DX[code]
        ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < Wd)
        idx = np.flatnonzero(m)
        succ[idx[ok]] = ty[ok] * Wd + tx[ok]
    has = succ >= 0
    indeg = np.bincount(succ[has], minlength=H * Wd)
    wv = np.asarray(w, np.float64).reshape(-1)
    front = np.flatnonzero(indeg == 0)
    while front.size:
        src = front[has[front]]
        t = succ[src]
        np.add.at(acc, t, acc[src] + wv[src])
        np.subtract.at(indeg, t, 1)
        t = np.unique(t)
        front = t[indeg[t] == 0]
    return acc.reshape(H, Wd)


@pytest.mark.parametrize("W", [1024, 1000])
def test_sums_at_the_bound_are_exact(W):
    """a serpentine main stem through every tile of the raster, so that the outlet's sum is every cell's weight: at
    frac_bits=0 with the largest integer weight the bound admits, and at the default scale with weights just below a
    power of two, the sums reach about 2^52 and stay exact"""
    from descriptools_amd import flowacc
    H = 256
    fdr = np.empty((H, W), np.uint8)
    fdr[0::2, :] = E
    fdr[1::2, :] = W_
    fdr[0::2, W - 1] = S
    fdr[1::2, 0] = S
    fdr[H - 1, 0] = 0                                # H even: the last row runs west onto the outlet
    n = H * W
    order = np.arange(n).reshape(H, W)              # position of every cell along the stem
    order[1::2] = order[1::2, ::-1]
    outlet = (H - 1, 0)

    def stem(q):
        """sums along the stem: everything before the cell"""
        flat = np.zeros(n, np.int64)
        flat[order.reshape(-1)] = q.reshape(-1)
        up = np.concatenate([[0], np.cumsum(flat)[:-1]])
        return up[order]

    qmax = 2 ** 52 // n
    rng = np.random.default_rng(W)
    wi = rng.integers(qmax - 1000, qmax + 1, size=(H, W)).astype(np.int64)
    got = flowacc.accumulate_weighted(fdr, wi, frac_bits=0)
    want = stem(wi).astype(np.float64)
    assert np.array_equal(got, want), int((got != want).sum())
    assert got[outlet] == float(int(wi.sum()) - int(wi[outlet])) > 2.0 ** 51
    wf = np.nextafter(2.0, 0.0) - rng.random((H, W)) * 1e-9
    s = flowacc.weight_frac_bits(wf)
    got = flowacc.accumulate_weighted(fdr, wf)
    sums = stem(np.rint(np.ldexp(wf, s)).astype(np.int64))
    assert int(sums.max()) <= 2 ** 52 and int(sums.max()) > 2 ** 51
    assert np.array_equal(got.view(np.int64), np.ldexp(sums.astype(np.float64), -s).view(np.int64))


def test_determinism_and_tiers():
    """two runs, and the host and the device tier, are bit-identical"""
    from descriptools_amd import _lib, flowacc
    from descriptools_amd.device import Context
    fdr, dem = _terrain(1000)
    w = np.random.default_rng(1).random(fdr.shape) * 10
    a = flowacc.accumulate_weighted(fdr, w, dem)
    b = flowacc.accumulate_weighted(fdr, w, dem)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    s = flowacc.weight_frac_bits(w)
    d = np.where(dem <= -100, np.float32(-100), np.float32(0)).astype(np.float32)
    ctx = Context()
    try:
        L = _lib.lib()
        H, W = fdr.shape
        f_d, z_d, w_d = ctx.to_device(fdr), ctx.to_device(d), ctx.to_device(w)
        out = ctx.empty((H, W), np.float64)
        for _ in range(2):
            _lib.check(L.dt_dev_flowacc_weighted(ctx.h, f_d.ptr, z_d.ptr, w_d.ptr, H, W, s, out.ptr))
            assert ctx.status() == 0
            assert np.array_equal(out.to_host().view(np.int64), a.view(np.int64))
        for x in (f_d, z_d, w_d, out):
            x.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), 1e6])
def test_bad_weight_raises_the_status(bad):
    """the device entry given a weight outside the contract raises DT_STATUS_BAD_WEIGHT (1e6 is over the bound of the
    frac_bits passed); the context then runs a good call with a clean status, and the host tier fails the call"""
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    fdr, _ = _cycles(200)
    H, W = fdr.shape
    w = np.ones((H, W))
    s = 30  # 38400 * 2^30 < 2^52 < 38400 * 1e6 * 2^30
    w_bad = w.copy()
    w_bad[70, 70] = bad
    L = _lib.lib()
    ctx = Context()
    try:
        f_d, wb_d, wg_d = ctx.to_device(fdr), ctx.to_device(w_bad), ctx.to_device(w)
        out = ctx.empty((H, W), np.float64)
        _lib.check(L.dt_dev_flowacc_weighted(ctx.h, f_d.ptr, None, wb_d.ptr, H, W, s, out.ptr))
        if bad < 0:
            with pytest.raises(ValueError, match="BAD_WEIGHT"):
                ctx.raise_on_status()
        else:
            assert ctx.status() & DT_STATUS_BAD_WEIGHT
        _lib.check(L.dt_dev_flowacc_weighted(ctx.h, f_d.ptr, None, wg_d.ptr, H, W, s, out.ptr))
        assert ctx.status() == 0
        assert np.array_equal(out.to_host(), expected(fdr, w, None, s))
        for x in (f_d, wb_d, wg_d, out):
            x.free()
    finally:
        ctx.close()
    acc = np.empty((H, W))
    c = ctypes
    rc = L.dt_flowacc_weighted(np.ascontiguousarray(fdr).ctypes.data_as(c.POINTER(c.c_uint8)), None,
                               w_bad.ctypes.data_as(c.POINTER(c.c_double)), H, W, s,
                               acc.ctypes.data_as(c.POINTER(c.c_double)))
    assert rc != 0 and b"weight" in L.dt_last_error()
