"""numpy reference of descriptools_amd.regions (the definition in that module's docstring), in two independent forms,
and the masks the tests label.

flood(mask, connectivity): a scan in ascending flat index with an explicit stack; the first cell of a region found is
its smallest cell, hence its label.
relax(mask, connectivity): every foreground cell starts with its own flat index; repeated np.minimum over the shifted
label planes, then every cell takes the label of the cell its label names, until nothing changes.

Both return the int64 label raster, -100 on background.  pairing_model(mask, connectivity, tile) applies, one after the
other on the host, exactly the unions the kernels make (which pairs, inside tiles and across seams): it shows that those
pairs suffice, for any tile edge.  sizes, connected, sieve and inundate_connected are written out
from the definitions; inundate_connected takes the depth from tests/_reaches_ref.py."""
import numpy as np

BIG = np.iinfo(np.int64).max
OFFS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
        8: ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def foreground(mask):
    return np.asarray(mask) != 0


def flood(mask, connectivity=8):
    fg = foreground(mask)
    H, W = fg.shape
    offs = OFFS[connectivity]
    f = fg.reshape(-1).tolist()
    out = [-100] * (H * W)
    for s in np.flatnonzero(fg.reshape(-1)).tolist():  # ascending
        if out[s] != -100:
            continue
        out[s] = s
        stack = [s]
        while stack:
            y, x = divmod(stack.pop(), W)
            for dy, dx in offs:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W:
                    n = yy * W + xx
                    if f[n] and out[n] == -100:
                        out[n] = s
                        stack.append(n)
    return np.array(out, np.int64).reshape(H, W)


def relax(mask, connectivity=8):
    fg = foreground(mask)
    H, W = fg.shape
    lab = np.where(fg, np.arange(H * W, dtype=np.int64).reshape(H, W), BIG)
    if not fg.any():
        return np.full((H, W), -100, np.int64)
    while True:
        pad = np.full((H + 2, W + 2), BIG, np.int64)
        pad[1:-1, 1:-1] = lab
        new = lab
        for dy, dx in OFFS[connectivity]:
            new = np.minimum(new, pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        new = np.where(fg, new, BIG)
        flat = new.reshape(-1)
        new = np.where(fg, flat[np.where(fg, new, 0)], BIG)  # the label of the cell the label names
        if (new == lab).all():
            break
        lab = new
    return np.where(fg, lab, -100).astype(np.int64)


def pairing_model(mask, connectivity=8, tile=64):
    """the pairs csrc/dt_regions.hip unites, applied one after the other on the host: inside every tile (cells outside
    it count as background), then from the cells of every tile's first row and first column across the seams.  (c, W)
    always; (c, N) unless W and NW are foreground too; a diagonal pair only when both cells that touch the two are
    background.  Returns the label raster these unions give."""
    fg = foreground(mask)
    H, W = fg.shape
    T = tile
    par = list(range(H * W))

    def find(a):
        while par[a] != a:
            a = par[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            par[max(a, b)] = min(a, b)

    def rules(c, w, e, n, nw, ne):
        if n and not (w and nw):
            unite(c, c - W)
        if connectivity == 8:
            if nw and not n and not w:
                unite(c, c - W - 1)
            if ne and not n and not e:
                unite(c, c - W + 1)

    def at(y, x):
        return 0 <= y < H and 0 <= x < W and bool(fg[y, x])

    for y, x in np.argwhere(fg).tolist():
        def local(dy, dx):
            return 0 <= y % T + dy < T and 0 <= x % T + dx < T and at(y + dy, x + dx)
        c = y * W + x
        if local(0, -1):
            unite(c, c - 1)  # the row run
        if y % T:
            rules(c, local(0, -1), local(0, 1), local(-1, 0), local(-1, -1), local(-1, 1))
    for y in range(T, H, T):      # first rows: N, NW, NE
        for x in range(W):
            if fg[y, x]:
                rules(y * W + x, at(y, x - 1), at(y, x + 1), at(y - 1, x), at(y - 1, x - 1), at(y - 1, x + 1))
    for x in range(T, W, T):      # first columns: W, NW, SW
        for y in range(H):
            if not fg[y, x]:
                continue
            c = y * W + x
            if at(y, x - 1):
                unite(c, c - 1)
            elif connectivity == 8:
                if at(y - 1, x - 1) and not at(y - 1, x):
                    unite(c, c - W - 1)
                if at(y + 1, x - 1) and not at(y + 1, x):
                    unite(c, c + W - 1)
    out = np.full(H * W, -100, np.int64)
    for i in np.flatnonzero(fg.reshape(-1)).tolist():
        out[i] = find(i)
    return out.reshape(H, W)


def sizes(label):
    """int64: the number of cells that carry the cell's label, 0 on background"""
    lab = np.asarray(label, np.int64)
    fg = lab >= 0
    count = np.bincount(lab[fg], minlength=lab.size).astype(np.int64)
    return np.where(fg, count[np.where(fg, lab, 0)], 0).astype(np.int64)


def connected(mask, seeds, connectivity=8, min_cells=1, form=flood):
    """uint8 keep; seeds None: every region counts as seeded"""
    lab = form(mask, connectivity)
    fg = lab >= 0
    keep = fg & (sizes(lab) >= min_cells)
    if seeds is not None:
        sd = foreground(seeds) & fg  # a seed on background seeds nothing
        seeded = np.zeros(lab.size, bool)
        seeded[lab[sd]] = True
        keep &= seeded[np.where(fg, lab, 0)]
    return keep.astype(np.uint8)


def sieve(mask, min_cells, connectivity=8, form=flood):
    return connected(mask, None, connectivity, min_cells, form)


def wet_mask(catch, hand, stage):
    """the third clause of inundation: catch in range, stage finite, 0 <= hand <= stage"""
    c = np.asarray(catch).astype(np.int64)
    h = np.asarray(hand)
    h = (h if h.dtype in (np.float32, np.float64) else h.astype(np.float64)).astype(np.float64)
    sg = np.asarray(stage, np.float64)
    inr = (c >= 0) & (c < sg.size)
    st = np.where(inr, sg[np.where(inr, c, 0)] if sg.size else np.nan, np.nan)
    with np.errstate(invalid="ignore"):
        return inr & np.isfinite(st) & (h >= 0) & (h <= st)


def inundate_connected(catch, hand, stage, river, connectivity=8, form=flood):
    """(depth float32, kept bool): _reaches_ref.inundate, 0 on the wet cells whose wet region holds no wet river cell"""
    import _reaches_ref as RR
    wet = wet_mask(catch, hand, stage)
    seeds = wet & (np.asarray(river).astype(np.int8) == 1)
    kept = connected(wet, seeds, connectivity, 1, form) == 1
    depth = RR.inundate(catch, hand, stage).copy()
    depth[wet & ~kept] = np.float32(0)
    return depth, kept


# ---- masks -------------------------------------------------------------------------------------------------------------
def serpentine(H, W):
    """a one-cell-wide corridor: every other row full, joined at alternating ends -> one region under both
    connectivities, of serpentine_cells(H, W) cells"""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def serpentine_cells(H, W):
    full = (H + 1) // 2
    return full * W + (full - 1)


def rings(H, W):
    """concentric square rings two cells apart: nested regions that never touch"""
    y, x = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    return (d % 3 == 0).astype(np.uint8)


def patterns(H, W, seed=0):
    """name -> uint8 mask"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    p = {"none": np.zeros((H, W), np.uint8), "all": np.ones((H, W), np.uint8)}
    c = np.zeros((H, W), np.uint8)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = 1
    p["corners"] = c
    for pct in (5, 41, 50, 59, 95):
        p["random%d" % pct] = (rng.random((H, W)) < pct / 100.0).astype(np.uint8)
    p["checkerboard"] = ((y + x) % 2 == 0).astype(np.uint8)
    p["comb_h"] = ((y % 2 == 0) | (x == 0)).astype(np.uint8)
    p["comb_v"] = ((x % 2 == 0) | (y == H - 1)).astype(np.uint8)
    p["serpentine"] = serpentine(H, W)
    p["rings"] = rings(H, W)
    return p


def terrain_mask(oracle, H, W, seed=3, nodata_pct=0, px=10.0, threshold=30, level=3):
    """(mask uint8 = hand <= level, river int8, hand) of the oracle's chain on its synthetic terrain"""
    dem = oracle.synth_dem(seed, H, W, nodata_pct=nodata_pct)
    _, fdr = oracle.slope_d8(dem, px)
    fac = oracle.flowacc(fdr, dem)
    river = (fac > threshold).astype(np.int8)
    _, _, hand = oracle.flowhand(dem, fdr, river, px)
    return (hand <= level).astype(np.uint8), river, hand
