"""CPU: conditioning on float64 heights (flowdir.d8_conditioned(heights=...), run_host(heights="float64",
condition=True), dt_*condition*_f64) -- the expectation the GPU tests compare against, what is refused before any
device work, and the C ABI of the three entry points.

The expectation needs no float64 oracle.  Fill and flat routing are invariant under any strictly increasing map of the
valid heights; only D8's choice among lower neighbours uses the values themselves.  So the pinned float32 oracle runs
on the dense ranks of the heights (exact below 2^24 distinct heights), its filled surface is mapped back to heights,
and D8 on that float64 surface (test_gpu_chain_f64.d8_f64_np) gives the codes wherever it finds a lower neighbour;
the remaining cells are flats, whose routing the rank surface gives."""
import heapq

import numpy as np
import pytest

import oracle


def expected_f64(dem, px):
    """(fdr, filled) of conditioned D8 on float64 heights, from the float32 oracle on the dense ranks of the heights.
    Every valid height must lie above -100: D8 treats heights <= -100 as nodata, and the rank map would not."""
    from test_gpu_chain_f64 import d8_f64_np
    dem = np.asarray(dem, np.float64)
    valid = dem != -100.0
    assert (dem[valid] > -100.0).all()
    uniq, inv = np.unique(dem[valid], return_inverse=True)
    assert len(uniq) < 2 ** 24, "ranks must be float32-exact"
    r = np.full(dem.shape, -100.0, np.float32)
    r[valid] = (inv.reshape(-1) + 1).astype(np.float32)
    fdr_r, filled_r = oracle.condition_d8(r, px)
    filled = np.full(dem.shape, -100.0)
    filled[valid] = uniq[filled_r[valid].astype(np.int64) - 1]
    d8 = d8_f64_np(filled, px)
    return np.where(d8 != 0, d8, fdr_r).astype(np.uint8), filled


def priority_flood_f64(dem):
    """an independent sequential priority flood in float64: outlets are valid cells on the raster edge or next to
    nodata; W(n) = max(z(n), W(c)) in order of increasing W"""
    dem = np.asarray(dem, np.float64)
    H, W = dem.shape
    valid = dem != -100.0
    out = np.where(valid, np.inf, -100.0)
    heap = []
    for y in range(H):
        for x in range(W):
            if not valid[y, x]:
                continue
            edge = y in (0, H - 1) or x in (0, W - 1)
            if edge or not valid[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].all():
                out[y, x] = dem[y, x]
                heapq.heappush(heap, (dem[y, x], y, x))
    done = np.zeros((H, W), bool)
    while heap:
        w, y, x = heapq.heappop(heap)
        if done[y, x]:
            continue
        done[y, x] = True
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                v, u = y + dy, x + dx
                if (dy or dx) and 0 <= v < H and 0 <= u < W and valid[v, u] and not done[v, u]:
                    nw = max(dem[v, u], w)
                    if nw < out[v, u]:
                        out[v, u] = nw
                        heapq.heappush(heap, (nw, v, u))
    return out


def rough_f64(H, W, seed):
    """genuinely float64 terrain: integer heights around 4000 with noise, pits, a plateau and nodata, plus k * 1e-5
    (k < 8), below float32's resolution there (2.4e-4): rounded to float32 it is the integer terrain again"""
    rng = np.random.default_rng(seed)
    base = oracle.synth_dem(seed, 2048, 2048, 11, 17, H, W, 3)
    nod = base == -100
    z = np.floor(base.astype(np.float64) + rng.normal(0, 6.0, base.shape)) + 4000.0
    z[rng.random(z.shape) < 0.02] -= 40.0
    z += rng.integers(0, 8, z.shape) * 1e-5
    if H > 40 and W > 40:
        z[10:30, 5:35] = z[10:30, 5:35].min()  # a lake-sized plateau
    z[nod] = -100.0
    return z


def test_expectation_equals_an_independent_float64_priority_flood():
    for H, W, seed, nodata in ((23, 31, 1, False), (40, 37, 2, True)):
        dem = rough_f64(H, W, seed)
        if nodata:
            dem[12:18, 10:20] = -100.0
            dem[0, :5] = -100.0
        else:
            dem[dem == -100.0] = 4000.0
        assert (dem == -100.0).any() == nodata
        fdr, filled = expected_f64(dem, 10.0)
        assert np.array_equal(filled, priority_flood_f64(dem))
        valid = dem != -100.0
        assert (filled[valid] > dem[valid]).any(), "pits were filled"
        assert (fdr[valid] != 0).all() and (fdr[~valid] == 0).all()


def test_default_tier_still_refuses_float64_heights():
    from descriptools_amd import flowdir
    dem64 = rough_f64(20, 30, 3)
    for call in (lambda: flowdir.d8_conditioned(dem64, 10.0), lambda: flowdir.d8_conditioned(dem64, 10.0, True),
                 lambda: flowdir.d8_conditioned(dem64, 10.0, heights="float32")):
        with pytest.raises(ValueError, match="not exactly representable in float32"):
            call()


def test_bogus_tier_raises():
    from descriptools_amd import flowdir
    with pytest.raises(ValueError, match="heights must be one of"):
        flowdir.d8_conditioned(np.zeros((8, 8), np.float32), 10.0, heights="bogus")


def test_float64_conditioning_entry_points_are_declared_and_bound():
    from test_cabi import header_symbols
    from descriptools_amd import _lib
    new = {"dt_d8_conditioned_f64", "dt_dev_condition_d8_f64", "dt_dev_condition_d8_f64_async"}
    assert new <= set(header_symbols()) and new <= set(_lib.exported_symbols())


def test_run_host_refuses_out_of_scope_arguments_before_device_work(monkeypatch):
    from descriptools_amd import chain

    def no_context(*a, **k):
        raise AssertionError("a Context was created before the arguments were checked")
    monkeypatch.setattr(chain, "Context", no_context)
    dem64 = rough_f64(20, 30, 4)
    for lw in (True, "auto"):
        with pytest.raises(ValueError, match="long_walks"):
            chain.run_host(dem64, 10.0, heights="float64", condition=True, long_walks=lw)
    with pytest.raises(ValueError, match="external_fdr"):
        chain.run_host(dem64, 10.0, heights="auto", condition=True, external_fdr=True)
