"""Pure numpy / Python reference of descriptools_amd.flowpath's weighted sums, independent of the kernels' schedule and
of the identity they rest on: downstream_sum by sequential walks (each cell walks down until it meets a cell whose sum
is known, then the walk is unwound), upslope_longest by brute force over every source's path (every cell without a
feeder walks its whole path and offers its running sum to each cell it passes) -- never as M - T, so that U = M - T is
itself under test.  All arithmetic is on the quantised weights q = rint(w * 2^s) in integers.  Built on
_watershed_ref.graph.

Shared by tests/test_pathsum_host.py (which checks it on hand-built cases with literal expected arrays and checks the
identities) and tests/test_gpu_pathsum.py (which holds the GPU to it cell for cell)."""
import numpy as np

from _watershed_ref import E, N, S, SE, SW, W_, graph

UNKNOWN, FAIL = -2, -1


def quantise(weights, frac_bits):
    """q = rint(w * 2^s) as int64, round half to even"""
    return np.rint(np.ldexp(np.asarray(weights, np.float64), frac_bits)).astype(np.int64)


def default_frac_bits(weights):
    """accumulate_weighted's rule: s = 51 - ceil(log2 N) - floor(log2 max(w)); 0 when every weight is 0"""
    w = np.asarray(weights, np.float64)
    if w.size == 0 or w.max() == 0:
        return 0
    lg_n = 0
    while (1 << lg_n) < w.size:
        lg_n += 1
    e = 0
    top = float(w.max())
    while 2.0 ** (e + 1) <= top:
        e += 1
    while 2.0 ** e > top:
        e -= 1
    return 51 - lg_n - e


def sums(fdr, q, dem=None, stop=None):
    """T as a flat int64 array (FAIL where the path does not stop), by sequential walks"""
    fdr = np.asarray(fdr, np.uint8)
    n = fdr.size
    valid, succ, _ = graph(fdr, dem)
    st = None if stop is None else (np.asarray(stop).reshape(-1) != 0)
    halt = (valid & (succ < 0)) if st is None else (valid & st)
    succ_l, halt_l, valid_l, q_l = succ.tolist(), halt.tolist(), valid.tolist(), np.asarray(q).reshape(-1).tolist()
    T = [UNKNOWN] * n
    for c in range(n):
        if T[c] != UNKNOWN:
            continue
        path, on_path, cur = [], set(), c
        while True:
            if not valid_l[cur]:
                base = FAIL
                break
            if T[cur] != UNKNOWN:
                base = T[cur]
                break
            if halt_l[cur]:
                T[cur] = base = 0
                break
            if succ_l[cur] < 0 or cur in on_path:    # a terminal that is no stop cell, or round a cycle
                base = FAIL
                if succ_l[cur] < 0:
                    T[cur] = FAIL
                break
            on_path.add(cur)
            path.append(cur)
            cur = succ_l[cur]
        for p in reversed(path):
            if base != FAIL:
                base += q_l[p]
            T[p] = base
        if not valid_l[c]:
            T[c] = FAIL
    return np.array(T, np.int64)


def _scaled(v, ok, frac_bits, shape):
    return np.where(ok, np.ldexp(np.where(ok, v, 0).astype(np.float64), -frac_bits), -100.0).reshape(shape)


def downstream_sum(fdr, weights, dem=None, stop=None, frac_bits=None):
    """float64 by the definition in descriptools_amd/flowpath.py"""
    s = default_frac_bits(weights) if frac_bits is None else frac_bits
    T = sums(fdr, quantise(weights, s), dem, stop)
    return _scaled(T, T >= 0, s, np.asarray(fdr).shape)


def walk_paths(fdr, q, dem, stop, starts):
    """the cells `starts` (flat indices, whose paths must stop) walk their paths in lockstep.  Yields, per step,
    (cells, src, run, moving): where each walker stands, where it started, the sum of q from src up to but excluding
    the cell, and whether it moves on (False at its target)."""
    fdr = np.asarray(fdr, np.uint8)
    valid, succ, _ = graph(fdr, dem)
    st = None if stop is None else (np.asarray(stop).reshape(-1) != 0)
    halt = (succ < 0) if st is None else ((succ < 0) | (valid & st))
    q = np.asarray(q, np.int64).reshape(-1)
    cur = np.asarray(starts, np.int64)
    src = cur.copy()
    run = np.zeros(cur.size, np.int64)
    while cur.size:
        go = ~halt[cur]
        yield cur, src, run, go
        run = run[go] + q[cur[go]]
        src = src[go]
        cur = succ[cur[go]]


def sources(fdr, dem, ok):
    """the cells of `ok` (a flat mask) that no cell of `ok` drains into"""
    _, succ, _ = graph(fdr, dem)
    fed = np.zeros(ok.size, bool)
    fed[succ[(succ >= 0) & ok]] = True
    return np.flatnonzero(ok & ~fed)


def longest(fdr, q, dem=None):
    """U as a flat int64 array (FAIL where the stop-less T is undefined), by brute force over every source's path:
    the weights are >= 0, so the longest path that ends at a cell starts at a cell nothing drains into"""
    T = sums(fdr, q, dem, None)
    ok = T >= 0
    U = np.where(ok, 0, FAIL).astype(np.int64)
    for cells, _, run, _ in walk_paths(fdr, q, dem, None, sources(fdr, dem, ok)):
        np.maximum.at(U, cells, run)
    return U


def upslope_longest(fdr, weights, dem=None, frac_bits=None):
    """float64 by the definition in descriptools_amd/flowpath.py"""
    s = default_frac_bits(weights) if frac_bits is None else frac_bits
    U = longest(fdr, quantise(weights, s), dem)
    return _scaled(U, U >= 0, s, np.asarray(fdr).shape)


def step_length(fdr, px, dem=None):
    valid, succ, diag = graph(fdr, dem)
    out = np.where(succ >= 0, np.where(diag, px * np.sqrt(2.0), px), 0.0)
    return out.reshape(np.asarray(fdr).shape)


def field(H, W, seed, cycles, nodata=False, ring=(150, 90)):
    """test_gpu_flowpath.py's generator: random codes that move east or down, terminals and non-D8 codes, 5 % noise
    codes, planted 2 x 2 cycles, one long cycle of ring[0] x ring[1] moves, and (nodata) discs and specks of nodata"""
    rng = np.random.default_rng(seed)
    fdr = rng.choice(np.array([SW, S, SE, E], np.uint8), size=(H, W))
    fdr[rng.random((H, W)) < 0.002] = rng.choice(np.array([0, 3, 255], np.uint8))
    noisy = rng.random((H, W)) < 0.05
    fdr[noisy] = rng.choice(np.array([1, 2, 4, 8, 16, 32, 64, 128], np.uint8), size=int(noisy.sum()))
    for _ in range(cycles):
        y, x = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
        fdr[y, x], fdr[y, x + 1], fdr[y + 1, x + 1], fdr[y + 1, x] = E, S, W_, N
    y0, x0 = H // 3, W // 4
    rw, rh = ring
    fdr[y0, x0:x0 + rw] = E
    fdr[y0:y0 + rh, x0 + rw] = S
    fdr[y0 + rh, x0 + 1:x0 + rw + 1] = W_
    fdr[y0 + 1:y0 + rh + 1, x0] = N
    dem = None
    if nodata:
        dem = rng.random((H, W)).astype(np.float32) * 50
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(6):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(5, 40)
            dem[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = -100
        dem[rng.random((H, W)) < 0.01] = -150
    return fdr, dem


def hand_cases():
    """name -> dict(fdr, dem, weights, stop, frac_bits, dn, up): literal expected float64 arrays; dn is taken with the
    case's stop (None: to the terminal), up never has one"""
    f64 = lambda a: np.array(a, np.float64)
    c = {}
    # one row draining east to an outlet at the east edge: the outlet's own weight is never counted
    c["row_to_edge"] = dict(
        fdr=np.array([[E, E, E, E]], np.uint8), dem=None, stop=None, frac_bits=0, weights=f64([[1, 2, 4, 8]]),
        dn=f64([[7, 6, 4, 0]]), up=f64([[0, 1, 3, 7]]))
    # halves at one fractional bit
    c["halves"] = dict(
        fdr=np.array([[E, E, 0]], np.uint8), dem=None, stop=None, frac_bits=1, weights=f64([[0.5, 1.5, 9]]),
        dn=f64([[2.0, 1.5, 0]]), up=f64([[0, 0.5, 2.0]]))
    # round half to even: 0.25 * 2 = 0.5 -> 0, 0.75 * 2 = 1.5 -> 2
    c["half_to_even"] = dict(
        fdr=np.array([[E, E, 0]], np.uint8), dem=None, stop=None, frac_bits=1, weights=f64([[0.25, 0.75, 0]]),
        dn=f64([[1.0, 1.0, 0]]), up=f64([[0, 0, 1.0]]))
    # a negative scale: weights in units of 4
    c["negative_frac_bits"] = dict(
        fdr=np.array([[E, E, 0]], np.uint8), dem=None, stop=None, frac_bits=-2, weights=f64([[8, 9, 100]]),
        dn=f64([[16, 8, 0]]), up=f64([[0, 8, 16]]))
    # five branches into (1,1): its longest path is the costliest single move
    c["branches"] = dict(
        fdr=np.array([[SE, S, SW], [E, 0, W_]], np.uint8), dem=None, stop=None, frac_bits=0,
        weights=f64([[5, 2, 7], [1, 100, 3]]), dn=f64([[5, 2, 7], [1, 0, 3]]), up=f64([[0, 0, 0], [0, 7, 0]]))
    # two branches into (2,3): three moves of 1 beat two moves of 1
    c["branch_choice"] = dict(
        fdr=np.array([[0, SE, E, S], [0, 0, SE, S], [0, 0, 0, 0]], np.uint8), dem=None, stop=None, frac_bits=0,
        weights=np.ones((3, 4), np.int32), dn=f64([[0, 2, 3, 2], [0, 0, 1, 1], [0, 0, 0, 0]]),
        up=f64([[0, 0, 0, 1], [0, 0, 1, 2], [0, 0, 0, 3]]))
    # (0,0) -> SE (1,1) -> E (1,2), which points into nodata (1,3): a terminal
    c["diagonal_into_nodata"] = dict(
        fdr=np.array([[SE, 0, 0, 0], [0, E, E, E]], np.uint8), dem=np.array([[1, 1, 1, 1], [1, 1, 1, -100]], np.float32),
        stop=None, frac_bits=0, weights=f64([[3, 1, 1, 1], [1, 4, 9, 9]]),
        dn=f64([[7, 0, 0, 0], [0, 4, 0, -100]]), up=f64([[0, 0, 0, 0], [0, 3, 7, -100]]))
    # a 2 x 2 cycle with the tributary (1,2): no value on the cycle and on what drains into it, in both outputs
    c["cycle_with_tributary"] = dict(
        fdr=np.array([[E, S, 0], [N, W_, W_]], np.uint8), dem=None, stop=None, frac_bits=0,
        weights=np.ones((2, 3), np.uint8), dn=f64([[-100, -100, 0], [-100, -100, -100]]),
        up=f64([[-100, -100, 0], [-100, -100, -100]]))
    # a stop cell on a cycle stops it; (1,2) is a terminal that meets no stop cell
    c["stop_cell_on_cycle"] = dict(
        fdr=np.array([[E, S, 0], [N, W_, 0]], np.uint8), dem=None, stop=np.array([[0, 1, 1], [0, 0, 0]], np.int32),
        frac_bits=0, weights=f64([[1, 2, 3], [4, 5, 6]]), dn=f64([[1, 0, 0], [5, 10, -100]]),
        up=f64([[-100, -100, 0], [-100, -100, 0]]))
    # a stop cell on nodata is ignored: the cell above it is a terminal without a stop cell
    c["stop_on_nodata"] = dict(
        fdr=np.array([[S], [S], [0]], np.uint8), dem=np.array([[1], [-200], [1]], np.float32),
        stop=np.array([[0], [1], [1]], np.uint8), frac_bits=0, weights=f64([[2], [2], [2]]),
        dn=f64([[-100], [-100], [0]]), up=f64([[0], [-100], [0]]))
    # the path below the stop cell ends at a terminal without meeting another
    c["terminal_without_stop"] = dict(
        fdr=np.array([[E, E, E, E, 0]], np.uint8), dem=None, stop=np.array([[0, 1, 0, 0, 0]], bool), frac_bits=0,
        weights=f64([[1, 2, 3, 4, 5]]), dn=f64([[1, 0, -100, -100, -100]]), up=f64([[0, 1, 3, 6, 10]]))
    return c
