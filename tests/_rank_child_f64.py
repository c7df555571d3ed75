"""One rank of tests/test_gpu_rank_f64.py::test_two_processes_over_gloo (launched by torch.distributed.run): a
RankTile(heights="float64") on its window of a float64 DEM with given D8 codes, two steps of tiling.run_rank
(d8=False, overlap on the second), tiling.finish_downslope over gloo, and its core rasters written for the parent."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def global_dem(Hg, Wg):
    """a 1 per mille plane with sub-float32 detail, a flat and nodata: its downslope walks are hundreds of moves long
    and cross the process border (the same array in the parent)"""
    yy, xx = np.mgrid[0:Hg, 0:Wg]
    rng = np.random.default_rng(13)
    dem = 200.0 - 0.001 * xx - 0.0002 * yy + rng.integers(0, 8, (Hg, Wg)) * 1e-5
    dem[60:90, 40:Wg - 40] = 150.0
    dem[rng.random((Hg, Wg)) < 0.001] = -100.0
    return dem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--h", type=int, required=True)
    ap.add_argument("--w", type=int, required=True)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    from descriptools_amd import flowdir, tiling
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    layout = tiling.Layout.uniform(world, a.h, a.w)
    dem = global_dem(layout.Hg, layout.Wg)
    codes = flowdir.d8(dem, 10.0, heights="float64")
    tile = tiling.RankTile(layout, rank, device=0, px=10.0, river_threshold=(layout.Hg * layout.Wg) // 512,
                           heights="float64")
    h = tiling.HALO
    y0, x0 = layout.origin(rank)
    tile.set_dem_ext(np.pad(dem, h, constant_values=-100.0)[y0:y0 + tile.He, x0:x0 + tile.We])
    with tile.on_stream():
        fp = np.pad(codes, h, constant_values=0)[y0:y0 + tile.He, x0:x0 + tile.We]
        tile.t["fdr"].copy_(torch.as_tensor(np.ascontiguousarray(fp)))
    tile.ctx.sync()
    exchange = tiling.Exchange(tile, layout, world)
    for overlap in (False, True):  # twice: the step reuses its buffers
        tiling.run_rank(tile, layout, exchange, overlap=overlap, d8=False)
    tile.check_status()
    sent = tiling.finish_downslope(tile, tiling.DistComm())
    assert tile.unresolved_downslope() == 0
    names = ["dem", "fdr", "fac", "river", "fdist", "idx", "hand", "slope", "ti", "mti", "gfi", "lnhlh", "down"]
    np.savez(os.path.join(a.out, "rank%d.npz" % rank), origin=np.array(layout.origin(rank)), sent=np.array(sent),
             **{n: tile.host(n) for n in names})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
