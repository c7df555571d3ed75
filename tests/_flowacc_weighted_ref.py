"""Pure numpy reference of weighted flow accumulation on a D8 raster, on the quantised weights in integers.  Shared by
tests/test_gpu_flowacc_weighted.py and the rows of tests/_poison_cases.py."""
import numpy as np

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
_DY = {E: 0, SE: 1, S: 1, SW: 1, W_: 0, NW: -1, N: -1, NE: -1}
_DX = {E: 1, SE: 1, S: 0, SW: -1, W_: -1, NW: -1, N: 0, NE: 1}


def reference(fdr, q, dem=None):
    """int64 sums of q over the cells strictly upstream (in-degree peeling on the D8 tree; cells never peeled sit on a
    cycle), -100 on cycles and nodata -> (sums, mask of -100)"""
    H, W = fdr.shape
    n = H * W
    f = fdr.reshape(-1)
    succ = np.full(n, -1, np.int64)
    y, x = np.divmod(np.arange(n), W)
    for code in _DY:
        m = f == code
        ty, tx = y[m] + _DY[code], x[m] + _DX[code]
        ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        idx = np.flatnonzero(m)
        succ[idx[ok]] = ty[ok] * W + tx[ok]
    has = succ >= 0
    indeg = np.bincount(succ[has], minlength=n)
    acc = np.zeros(n, np.int64)
    q = q.reshape(-1).astype(np.int64)
    done = np.zeros(n, bool)
    front = np.flatnonzero(indeg == 0)
    while front.size:
        done[front] = True
        src = front[has[front]]
        t = succ[src]
        np.add.at(acc, t, acc[src] + q[src])
        np.subtract.at(indeg, t, 1)
        t = np.unique(t)
        front = t[indeg[t] == 0]
    dead = ~done
    if dem is not None:
        dead |= np.asarray(dem).reshape(-1) <= -100
    return acc.reshape(H, W), dead.reshape(H, W)
