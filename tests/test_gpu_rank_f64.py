"""GPU (-m gpu): the rank-tiled step on float64 heights (tiling.RankTile(heights="float64")) against the untiled
float64 chain (chain.Chain(heights="float64")) on the whole raster, every raster bit for bit -- through simulate_dev,
run_ranks_local, run_rank and real processes -- and its downslope walks across rank borders."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle
from test_gpu_chain_f64 import chain_once, d8_f64_np, wide_dems
from test_hydro_f64_host import rough_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fdr", "fac", "river", "fdist", "idx", "hand", "slope", "ti", "mti", "gfi", "lnhlh", "down"]


def make_tiles(layout, dem, heights="float64", fdr=None, px=10.0, **kw):
    """one RankTile per logical rank on device 0, its DEM (and codes, when given) cut from the global raster with the
    halo; outside the raster: nodata, code 0"""
    from descriptools_amd import tiling
    import torch
    h = tiling.HALO
    pad = np.pad(np.asarray(dem, np.float64), h, constant_values=-100.0)
    fpad = np.pad(fdr, h, constant_values=0) if fdr is not None else None
    thr = (layout.Hg * layout.Wg) // 512
    tiles = []
    for r in range(layout.size):
        tl = tiling.RankTile(layout, r, device=0, px=px, river_threshold=thr, tune_placement=False, heights=heights,
                             **kw)
        y0, x0 = layout.origin(r)
        tl.set_dem_ext(pad[y0:y0 + tl.He, x0:x0 + tl.We])
        if fpad is not None:
            with tl.on_stream():
                tl.t["fdr"].copy_(torch.as_tensor(np.ascontiguousarray(fpad[y0:y0 + tl.He, x0:x0 + tl.We])))
            tl.ctx.sync()
        tiles.append(tl)
    return tiles


def check(tiles, layout, ref, names=NAMES):
    for tl in tiles:
        y0, x0 = layout.origin(tl.rank)
        sl = (slice(y0, y0 + tl.H), slice(x0, x0 + tl.W))
        for n in names:
            got, want = tl.host(n), ref[n][sl]
            if n == "hand":
                assert got.dtype == want.dtype == np.float64
            assert np.array_equal(got, want.astype(got.dtype), equal_nan=True), \
                "rank %d %s: %d cells differ" % (tl.rank, n, int((got != want.astype(got.dtype)).sum()))


def free(tiles):
    import torch
    for tl in tiles:
        tl.free()
    torch.cuda.empty_cache()


def finish_walks(tiles, layout):
    """tiling.finish_downslope on every logical rank, one thread each (LocalComm)"""
    from descriptools_amd import tiling
    comms = tiling.LocalComm.create(layout.size)
    done, errors = [None] * layout.size, []

    def work(r):
        try:
            done[r] = tiling.finish_downslope(tiles[r], comms[r])
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append(e)
            comms[r].sh.barrier.abort()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(layout.size)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    return done


@pytest.mark.parametrize("dem_kind,heights,widths,driver,kw", [
    ("d64", [128, 128], [128, 128], "simulate_dev", {}),                           # 2 x 2
    ("mm", [192], [128, 128], "run_ranks_local", {}),                             # 1 x 2, nodata
    ("rough", [128, 70], [64, 90], "run_ranks_local", {"idx64": True, "acc64": True}),  # ragged last row / column
    ("rough", [64, 64, 64], [64, 64, 64], "simulate_dev", {"acc64": True}),        # 3 x 3
    ("d64", [100], [130], "simulate_dev", {"idx64": True}),                        # 1 x 1
])
def test_tiled_equals_untiled_float64_chain(dem_kind, heights, widths, driver, kw):
    from descriptools_amd import tiling
    layout = tiling.Layout(heights, widths)
    Hg, Wg = layout.Hg, layout.Wg
    if dem_kind == "rough":
        dem = rough_f64(Hg, Wg, 7)
    else:
        d64, mm = wide_dems(Hg, Wg)
        dem = d64 if dem_kind == "d64" else mm.astype(np.float64)
    assert (dem.astype(np.float32).astype(np.float64) != dem).any(), "the DEM is meant to be genuinely float64"
    ref = chain_once(dem, 10.0, "float64", river_threshold=(Hg * Wg) // 512)
    tiles = make_tiles(layout, dem, **kw)
    try:
        if driver == "simulate_dev":
            tiling.simulate_dev(tiles, layout)
        else:
            tiling.run_ranks_local(tiles, layout)
        for tl in tiles:
            tl.check_status()
            assert tl.unresolved_downslope() == 0
        check(tiles, layout, ref)
    finally:
        free(tiles)


@pytest.mark.parametrize("overlap", [False, True])
def test_run_rank_one_rank(overlap):
    """run_rank on a single rank (overlap on and off): the step with the side stream and the Exchange object"""
    from descriptools_amd import tiling
    layout = tiling.Layout([96], [160])
    dem = rough_f64(96, 160, 3)
    ref = chain_once(dem, 10.0, "float64", river_threshold=(96 * 160) // 512)
    tiles = make_tiles(layout, dem)
    try:
        ex = tiling.Exchange(tiles[0], layout, 1)
        for _ in range(2):
            tiling.run_rank(tiles[0], layout, ex, overlap=overlap)
        check(tiles, layout, ref)
    finally:
        free(tiles)


def _flat_rough(Hg, Wg, seed):
    """rough_f64 terrain with a wide flat across the rank borders: conditioned, its walks run along the flat for more
    than a halo's width"""
    dem = rough_f64(Hg, Wg, seed)
    valid = dem != -100.0
    lo = dem[valid].min()
    dem[40:90, 20:Wg - 20] = lo + 3.25e-5
    return dem


def test_conditioned_codes_walks_across_rank_borders():
    """d8=False on the float64-conditioned codes: walks leave their rank (-50 marks), finish_downslope walks them on
    as float64 walkers; then every raster equals the untiled float64 chain's on the same codes"""
    from descriptools_amd import flowdir, tiling
    layout = tiling.Layout([128, 128], [128, 128])
    dem = _flat_rough(layout.Hg, layout.Wg, 11)
    codes = flowdir.d8_conditioned(dem, 10.0, heights="float64")
    ref = chain_once(dem, 10.0, "float64", fdr=codes, river_threshold=(layout.Hg * layout.Wg) // 512)
    tiles = make_tiles(layout, dem, fdr=codes)
    try:
        tiling.simulate_dev(tiles, layout, d8=False)
        marked = sum(tl.unresolved_downslope() for tl in tiles)
        assert marked > 0, "the flat is meant to send walks across the rank borders"
        assert all(d == marked for d in finish_walks(tiles, layout))
        assert all(tl.unresolved_downslope() == 0 for tl in tiles)
        check(tiles, layout, ref)
    finally:
        free(tiles)


def test_plane_walks_with_sub_float32_detail():
    """a 1 per mille plane with a flat and nodata (test_gpu_tiling.test_downslope_walks_across_rank_borders) plus
    sub-float32 detail, and a dz float32 cannot hold: every walk is long and crosses ranks; the result equals the
    float64 oracle's walk on the whole raster"""
    from descriptools_amd import tiling
    layout = tiling.Layout([192, 192], [256, 256])
    Hg, Wg = layout.Hg, layout.Wg
    yy, xx = np.mgrid[0:Hg, 0:Wg]
    rng = np.random.default_rng(4)
    dem = 200.0 - 0.001 * xx - 0.0002 * yy + rng.integers(0, 8, (Hg, Wg)) * 1e-5
    dem[150:180, 100:500] = 150.0
    dem[rng.random((Hg, Wg)) < 0.0005] = -100.0
    dz = 5.0 + 3e-6
    assert float(np.float32(dz)) != dz
    fdr = d8_f64_np(dem, 1.0)
    want = oracle.downslope_f64(dem, fdr, 1.0, dz)
    tiles = make_tiles(layout, dem, px=1.0, dz=dz)
    try:
        tiling.simulate_dev(tiles, layout)
        marked = sum(tl.unresolved_downslope() for tl in tiles)
        assert marked > 1000
        assert all(d == marked for d in finish_walks(tiles, layout))
        check(tiles, layout, {"fdr": fdr, "down": want}, names=["fdr", "down"])
    finally:
        free(tiles)


def test_float32_exact_heights_equal_the_float32_tier():
    """on heights that are float32 values a float64 tile gives the float32 tile's rasters; hand agrees after the cast"""
    from descriptools_amd import tiling
    layout = tiling.Layout([128, 128], [128, 128])
    got = {}
    for heights in ("float32", "float64"):
        tiles = make_tiles(layout, np.zeros((layout.Hg, layout.Wg)), heights=heights)
        try:
            for tl in tiles:
                tl.synth_dem(3, 2)
            tiling.simulate_dev(tiles, layout)
            got[heights] = [{n: tl.host(n) for n in NAMES} for tl in tiles]
        finally:
            free(tiles)
    for a, b in zip(got["float32"], got["float64"]):
        assert b["hand"].dtype == np.float64
        for n in NAMES:
            assert np.array_equal(a[n], b[n].astype(a[n].dtype), equal_nan=True), n


def test_two_processes_over_gloo(tmp_path):
    """run_rank (d8=False, overlap off and on) + finish_downslope on float64 tiles in two real processes (gloo between
    them, the one GPU shared): every raster equals the untiled float64 chain's on the same codes"""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    H, W = 192, 192
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "_rank_child_f64.py"), "--out",
           str(tmp_path), "--h", str(H), "--w", str(W)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _rank_child_f64 import global_dem
    from descriptools_amd import flowdir, tiling
    layout = tiling.Layout.uniform(2, H, W)
    dem = global_dem(layout.Hg, layout.Wg)
    codes = flowdir.d8(dem, 10.0, heights="float64")
    ref = chain_once(dem, 10.0, "float64", fdr=codes, river_threshold=(layout.Hg * layout.Wg) // 512)
    sent = 0
    for r in range(2):
        p = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        y0, x0 = (int(v) for v in p["origin"])
        sent += int(p["sent"])
        sl = (slice(y0, y0 + p["fdr"].shape[0]), slice(x0, x0 + p["fdr"].shape[1]))
        assert np.array_equal(p["dem"], dem[sl])
        for n in NAMES:
            got, want = p[n], ref[n][sl]
            assert np.array_equal(got, want.astype(got.dtype), equal_nan=True), (r, n, int((got != want).sum()))
    assert sent > 0, "walks are meant to cross the process border"
