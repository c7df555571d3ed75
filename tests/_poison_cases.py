"""The table behind tests/test_gpu_poison.py: one row per public function of the op modules that launches a kernel.

A row builds its inputs from a seed, calls the op, and names the reference with the bar the op's own GPU test holds it to
(the tests/_*_ref.py function that test uses, or `oracle` for the chain ops; `EQUAL` is dtype, shape and bytes).  Builders
and references are numpy / Python only: they run without the library and without a GPU.  EXEMPT names every public
function that has no row, with the reason; test_gpu_poison.py fails for a public function that is in neither.

The inputs are the smallest at which the tile scaffolds still run all their parts: 130 x 67 cells are 3 x 2 tiles of
64 x 64, ragged both ways, with one interior tile row; a block of nodata covers the corner four tiles share and cuts
the tile edges that meet there; direction fields come from the generators the ops' tests use (planted 2-cycles, a long
ring, a serpentine), so that more than one global round runs.  Ops with a second code path by size get a second row at
the smallest input that takes it."""
import functools
import importlib
import math

import numpy as np

MODULES = ("cost", "dinf", "downslope", "evaluation", "filters", "flowacc", "flowdir", "flowhand", "flowpath", "focal",
           "gfi", "harmonic", "horizon", "inundation", "mfd", "morphology", "mrvbf", "proximity", "reaches", "regions",
           "resample", "routing", "slope", "streams", "terrain", "topoindexes", "vector", "watershed", "wetness", "zonal")
H, W, PX = 130, 67, 10.0
HOLE = (slice(56, 72), slice(58, 67))  # covers the tile corner (64, 64), cuts the tile edges y = 64 and x = 64
EQUAL = "equal"


def close(rtol, atol=0.0):
    """conftest.assert_float_close's bar: nodata (-100) exact, NaN with NaN, |got - ref| <= rtol |ref| + atol"""
    return ("close", rtol, atol)


class Row:
    def __init__(self, name, covers, build, call, ref, bars=EQUAL, unordered=None):
        self.name, self.covers, self.call = name, tuple(covers), call
        self.build, self.ref = (f if hasattr(f, "cache_info") else cached(f) for f in (build, ref))  # computed once
        self.bars = bars            # EQUAL, close(...), a dict output -> one of these, or a function (got, want, inputs)
        self.unordered = unordered  # None, or "file:line: why the bytes may depend on the order of work"

    def __repr__(self):
        return self.name


ROWS = []


def row(name, covers, build, ref, bars=EQUAL, unordered=None):
    """decorator of the row's call: call(m, inputs) -> {output: array}, m.<module> the op modules"""
    def add(call):
        ROWS.append(Row(name, covers, build, call, ref, bars, unordered))
        return call
    return add


class _Modules:
    def __getattr__(self, name):
        return importlib.import_module("descriptools_amd." + name)


M = _Modules()


# ---- comparison -----------------------------------------------------------------------------------------------------
def leaves(x, path=""):
    """every array and every number of a result (an info word is a 0-d array), in a fixed order: (path, ndarray)"""
    if x is None:
        return
    if isinstance(x, np.ndarray):
        yield path, np.asarray(x)
    elif isinstance(x, (bool, int, float, np.number, np.bool_)):
        yield path, np.asarray(x)
    elif isinstance(x, dict):
        for k in x:
            yield from leaves(x[k], "%s.%s" % (path, k))
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            yield from leaves(v, "%s[%d]" % (path, i))
    elif hasattr(x, "__dict__") and not callable(x):
        for k in sorted(vars(x)):
            yield from leaves(vars(x)[k], "%s.%s" % (path, k))


def same_bytes(what, got, want):
    g, w = list(leaves(got)), list(leaves(want))
    assert [p for p, _ in g] == [p for p, _ in w], "%s: outputs %s, expected %s" % (what, [p for p, _ in g],
                                                                                  [p for p, _ in w])
    for (p, a), (_, b) in zip(g, w):
        assert a.dtype == b.dtype and a.shape == b.shape, "%s%s: %s%s, expected %s%s" % (what, p, a.dtype, a.shape,
                                                                                        b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            va, vb = (np.ascontiguousarray(v).reshape(-1).view(np.uint8) for v in (a, b))
            bad = np.flatnonzero(va != vb)
            i = np.unravel_index(bad[0] // a.dtype.itemsize, a.shape) if a.ndim else ()
            raise AssertionError("%s%s: %d bytes differ, first at %s: %r, expected %r" % (what, p, bad.size, i, a[i], b[i]))


def _close(what, got, ref, rtol, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    nod = ref == -100
    assert np.array_equal(got == -100, nod), what + ": nodata mask differs"
    ok = (np.isnan(got) & np.isnan(ref)) | nod | (got == ref) | (np.abs(got - ref) <= rtol * np.abs(ref) + atol)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError("%s: %d cells differ, first at %s got %r ref %r" % (what, len(bad), i, got[i], ref[i]))


def meets(r, got, want, inputs):
    """the outputs the reference names, each at the row's bar"""
    if getattr(r.bars, "whole", False):  # a bar over the whole result: (got, want, inputs)
        r.bars(got, want, inputs)
        return
    for k, w in want.items():
        bar = r.bars.get(k, EQUAL) if isinstance(r.bars, dict) else r.bars  # one bar for every output, or one each
        what = "%s: %s" % (r.name, k)
        assert k in got, what + " is missing"
        if callable(bar):
            bar(what, got[k], w)
        elif bar == EQUAL:
            same_bytes(what, got[k], w)
        else:
            _close(what, got[k], w, bar[1], bar[2])


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _frozen(d):
    for _, a in leaves(d):
        a.setflags(write=False)
    return d


def cached(f):
    """a builder or a reference: computed once per argument, its arrays read-only"""
    g = functools.lru_cache(maxsize=None)(lambda *a: _frozen(f(*a)))
    return functools.wraps(f)(g)


class Inputs(dict):
    """a dict that hashes by identity, so that a reference can be cached on the inputs it was built for"""
    __hash__ = object.__hash__
    __eq__ = object.__eq__


def relief(seed, shape=(H, W), hole=True, below=False):
    """float32 heights: a few smooth waves, a tilt and 0.5 m steps (flats and exact ties), pits, the nodata block"""
    rng = np.random.default_rng(seed)
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 120 + 0.35 * y + 0.2 * x + 18 * np.sin(y / 9.0 + rng.uniform(0, 6)) * np.cos(x / 7.0 + rng.uniform(0, 6))
    z += rng.uniform(0, 4, shape)
    z = (np.round(z * 2) / 2).astype(np.float32)
    for _ in range(max(1, h * w // 800)):
        py, px_ = int(rng.integers(2, max(3, h - 2))), int(rng.integers(2, max(3, w - 2)))
        z[py - 1:py + 2, px_ - 1:px_ + 2] -= 12
    if hole and h > 72 and w > 58:
        z[HOLE] = -100
        if below:
            z[HOLE[0].start:HOLE[0].start + 3, HOLE[1].start] = -9999
    return z


@cached
def world(seed):
    """the chain's rasters on relief(seed), by the oracle: raw and conditioned D8, accumulation, river, HAND"""
    import oracle
    dem = relief(seed)
    slope, fdr_raw = oracle.slope_d8(dem, PX)
    fdr, filled = oracle.condition_d8(dem, PX)
    acc = oracle.flowacc(fdr, dem)
    river = (acc > 40).astype(np.int8)
    fdist, idx, hand = oracle.flowhand(dem, fdr, river, PX)
    slope_rad = np.where(dem <= -100, -100, np.arctan(slope / 100)).astype(np.float32)
    return Inputs(dem=dem, slope=slope, fdr_raw=fdr_raw, fdr=fdr, filled=filled, acc=acc, river=river, fdist=fdist,
                  idx=idx, hand=hand, slope_rad=slope_rad)


def serpentine_d8(shape=(H, W)):
    """one path through every cell: east along the even rows, west along the odd ones, south at the ends"""
    h, w = shape
    fdr = np.empty(shape, np.uint8)
    fdr[0::2], fdr[1::2] = 1, 16
    fdr[0::2, w - 1], fdr[1::2, 0] = 4, 4
    fdr[h - 1, w - 1 if (h - 1) % 2 == 0 else 0] = 0
    return fdr


@cached
def d8_field(seed):
    """_pathsum_ref.field: random codes, noise, non-D8 codes, planted 2 x 2 cycles, a ring through four tiles; the
    nodata block of relief(); `snake`: the serpentine with the same block cut out of it"""
    import _pathsum_ref as PS
    fdr, _ = PS.field(H, W, seed, cycles=3, ring=(30, 40))
    dem = relief(seed, below=True)
    rng = np.random.default_rng(seed + 100)
    values = rng.uniform(-50, 50, (H, W)).astype(np.float32)
    weights = rng.random((H, W)) * 3.7
    weights[rng.random((H, W)) < 0.1] = 0.0
    stop = (rng.random((H, W)) < 0.01).astype(np.uint8)
    return Inputs(fdr=fdr, dem=dem, snake=serpentine_d8(), values=values, weights=weights, stop=stop)


# ---- the chain ops: oracle, at the bars of tests/test_gpu_parity.py and tests/test_gpu_hydro.py -------------------------
def _ref_d8(i):
    return {"fdr": i["fdr_raw"], "slope": i["slope"]}


@row("flowdir.d8", ["flowdir.d8"], world, _ref_d8)
def _(m, i):
    fdr, sl = m.flowdir.d8(i["dem"], PX, return_slope=True)
    return {"fdr": fdr, "slope": sl, "fdr_alone": m.flowdir.d8(i["dem"], PX)}


@row("flowdir.d8[float64]", ["flowdir.d8"], world, _ref_d8)
def _(m, i):
    fdr, sl = m.flowdir.d8(i["dem"].astype(np.float64), PX, return_slope=True, heights="float64")
    return {"fdr": fdr, "slope": sl}


class _debug:
    """a debug key of the library for the block, 0 at its end"""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        from descriptools_amd import _lib
        _lib.check(_lib.lib().dt_debug_set(self.key, self.value))

    def __exit__(self, *exc):
        from descriptools_amd import _lib
        _lib.check(_lib.lib().dt_debug_set(self.key, 0))


HY_COLOUR_MIN = 8  # DT_DBG_HY_COLOUR_MIN = 1: the coloured conditioning rounds (activity flags in place) at this size


def _conditioned(m, dem, heights):
    out = {}
    for name, colour in (("", 0), (" coloured", 1)):
        with _debug(HY_COLOUR_MIN, colour):
            out["fdr" + name], out["filled" + name] = m.flowdir.d8_conditioned(dem, PX, return_filled=True, heights=heights)
            out["alone" + name] = m.flowdir.d8_conditioned(dem, PX, heights=heights)
    return out


def _ref_conditioned(i, dtype):
    filled = i["filled"].astype(dtype)
    return {"fdr": i["fdr"], "filled": filled, "alone": i["fdr"], "fdr coloured": i["fdr"], "filled coloured": filled,
            "alone coloured": i["fdr"]}


@row("flowdir.d8_conditioned", ["flowdir.d8_conditioned"], world, lambda i: _ref_conditioned(i, np.float32))
def _(m, i):
    return _conditioned(m, i["dem"], "float32")


@row("flowdir.d8_conditioned[float64]", ["flowdir.d8_conditioned"], world, lambda i: _ref_conditioned(i, np.float64))
def _(m, i):
    return _conditioned(m, i["dem"].astype(np.float64), "float64")


@cached
def _ref_carved(i):
    import _flowpath_ref as FP
    out = {}
    for cut in (None, 3.0):
        fdr, carved, filled = FP.carved(i["dem"], PX, cut)
        out["fdr %s" % cut], out["carved %s" % cut], out["filled %s" % cut] = fdr, carved, filled
    return out


@row("flowdir.d8_carved", ["flowdir.d8_carved"], world, _ref_carved)
def _(m, i):
    out = {}
    for cut in (None, 3.0):
        fdr, carved, filled = m.flowdir.d8_carved(i["dem"], PX, cut, return_filled=True)
        out["fdr %s" % cut], out["carved %s" % cut], out["filled %s" % cut] = fdr, carved, filled
    return out


@row("slope.sloper", ["slope.sloper"], world, lambda i: {"slope": i["slope"]})
def _(m, i):
    return {"slope": m.slope.sloper(i["dem"], PX).astype(np.float32), "f64": m.slope.sloper(i["dem"].astype(np.float64), PX)}


@cached
def _ref_flowacc(i):
    import oracle
    return {"acc": oracle.flowacc(i["fdr"], i["dem"]), "snake": oracle.flowacc(i["snake"], i["dem"]),
            "bare": oracle.flowacc(i["fdr"])}


@row("flowacc.accumulate", ["flowacc.accumulate"], d8_field, _ref_flowacc)
def _(m, i):
    return {"acc": m.flowacc.accumulate(i["fdr"], i["dem"]), "snake": m.flowacc.accumulate(i["snake"], i["dem"]),
            "bare": m.flowacc.accumulate(i["fdr"])}


def _frac_bits(weights):
    import _pathsum_ref as PS
    return PS.default_frac_bits(weights)


@cached
def _ref_flowacc_weighted(i):
    from _flowacc_weighted_ref import reference
    s = _frac_bits(i["weights"])
    out = {}
    for name in ("fdr", "snake"):
        sums, dead = reference(i[name], np.rint(np.ldexp(i["weights"], s)), i["dem"])
        out[name] = np.where(dead, -100.0, np.ldexp(sums.astype(np.float64), -s))
    return out


@row("flowacc.accumulate_weighted", ["flowacc.accumulate_weighted"], d8_field, _ref_flowacc_weighted)
def _(m, i):
    s = _frac_bits(i["weights"])
    return {name: m.flowacc.accumulate_weighted(i[name], i["weights"], i["dem"], frac_bits=s) for name in ("fdr", "snake")}


@row("flowhand.flow_hand_index", ["flowhand.flow_hand_index"], world,
     lambda i: {"fdist": i["fdist"], "idx": i["idx"], "hand": i["hand"]}, {"fdist": close(1e-6)})
def _(m, i):
    fd, idx, hand = m.flowhand.flow_hand_index(i["dem"], i["fdr"], i["river"], PX)
    return {"fdist": fd, "idx": idx, "hand": hand}


@row("flowhand.hand_calculator", ["flowhand.hand_calculator"], world, lambda i: {"hand": i["hand"]})
def _(m, i):
    return {"hand": m.flowhand.hand_calculator(i["dem"], i["idx"])}


def _dem64(i):
    """heights float32 cannot hold: the float64 entries (dt_hand_f64) take them"""
    d = np.where(i["dem"] > -100, i["dem"].astype(np.float64) + 0.1, -100.0)
    assert (d.astype(np.float32).astype(np.float64) != d).any()
    return d


def _ref_hand64(i):
    import oracle
    hand = oracle.hand_f64(_dem64(i), i["idx"])
    return {"fdist": i["fdist"], "idx": i["idx"], "hand": hand, "hand alone": hand}


@row("flowhand.flow_hand_index[float64]", ["flowhand.flow_hand_index", "flowhand.hand_calculator"], world, _ref_hand64,
     {"fdist": close(1e-6)})
def _(m, i):
    fd, idx, hand = m.flowhand.flow_hand_index(_dem64(i), i["fdr"], i["river"], PX)
    return {"fdist": fd, "idx": idx, "hand": hand, "hand alone": m.flowhand.hand_calculator(_dem64(i), i["idx"])}


@cached
def _ref_fdist_tile(i):
    import oracle
    fd, idx, _ = oracle.flowhand(i["dem"], i["fdr"], i["river"], PX)
    return {"fdist": fd, "idx": idx}


@row("flowhand.flow_distance_indexes_sequential", ["flowhand.flow_distance_index_cpu"], world, _ref_fdist_tile,
     {"fdist": close(1e-6)})
def _(m, i):
    fd, idx = m.flowhand.flow_distance_indexes_sequential(i["fdr"], i["river"], PX)
    return {"fdist": fd, "idx": idx}


@cached
def _ref_downslope(i):
    import oracle
    return {"down": oracle.downslope(i["dem"], i["fdr"], PX, 5.0)}


@row("downslope.downsloper", ["downslope.downsloper", "downslope.downslope_cpu"], world, _ref_downslope)
def _(m, i):
    return {"down": m.downslope.downsloper(i["dem"], i["fdr"], PX, 5), "raw": m.downslope.downslope_cpu(i["dem"], i["fdr"], PX, 5)}


@cached
def _ref_twi(i):
    import oracle
    ti, mti = oracle.twi(i["acc"], i["slope_rad"], PX, 0.1)
    return {"ti": ti, "mti": mti}


@row("topoindexes.topographic_index_cpu", ["topoindexes.topographic_index_cpu"], world, _ref_twi,
     {"ti": close(1e-5), "mti": close(1e-5, 1e-6)})
def _(m, i):
    ti, mti = m.topoindexes.topographic_index_cpu(i["acc"], i["slope_rad"], PX, 0.1)
    return {"ti": ti, "mti": mti}


@cached
def _ref_gfi(i):
    import oracle
    fac = i["acc"].reshape(-1)
    return {"gfi": oracle.gfi(i["hand"], i["acc"], i["idx"], 0.4, 0.1, PX),
            "lnhlh": oracle.lnhlh(i["hand"], i["acc"], 0.4, 0.1, PX),
            "river_acc": np.where(i["idx"] != -100, fac[i["idx"]], fac[0])}


@row("gfi", ["gfi.gfi_calculator", "gfi.ln_hl_H_calculator", "gfi.river_accumulation"], world, _ref_gfi,
     {"gfi": close(1e-5, 1e-6), "lnhlh": close(1e-5, 1e-6), "river_acc": lambda what, g, w: np.testing.assert_array_equal(g, w, what)})
def _(m, i):
    return {"gfi": m.gfi.gfi_calculator(i["hand"], i["acc"], i["idx"], 0.4, 0.1, PX),
            "lnhlh": m.gfi.ln_hl_H_calculator(i["hand"], i["acc"], 0.4, 0.1, PX),
            "river_acc": m.gfi.river_accumulation(i["acc"], i["idx"])}


# ---- D8 path ops on the direction fields: tests/_flowpath_ref.py, _pathsum_ref.py, _watershed_ref.py, _streams_ref.py ----
FIELDS = ("fdr", "snake")


@cached
def _ref_extremes(i):
    import _flowpath_ref as FP
    out = {}
    for f in FIELDS:
        for kind in ("max", "min"):
            out["up %s %s" % (f, kind)] = FP.upslope(i[f], i["values"], kind, i["dem"])
            for st in (None, "stop"):
                out["down %s %s %s" % (f, kind, st)] = FP.downstream(i[f], i["values"], kind, i["dem"], st and i[st])
    return out


@row("flowpath.extremes", ["flowpath.upslope_extreme", "flowpath.downstream_extreme"], d8_field, _ref_extremes)
def _(m, i):
    out = {}
    for f in FIELDS:
        for kind in ("max", "min"):
            out["up %s %s" % (f, kind)] = tuple(m.flowpath.upslope_extreme(i[f], i["values"], kind, i["dem"], where=True))
            out["alone %s %s" % (f, kind)] = m.flowpath.upslope_extreme(i[f], i["values"], kind, i["dem"]).value
            for st in (None, "stop"):
                out["down %s %s %s" % (f, kind, st)] = tuple(
                    m.flowpath.downstream_extreme(i[f], i["values"], kind, i["dem"], st and i[st], where=True))
    return out


@cached
def _ref_pathsums(i):
    import _pathsum_ref as PS
    s = PS.default_frac_bits(i["weights"])
    out = {}
    for f in FIELDS:
        out["longest " + f] = PS.upslope_longest(i[f], i["weights"], i["dem"], s)
        for st in (None, "stop"):
            out["sum %s %s" % (f, st)] = PS.downstream_sum(i[f], i["weights"], i["dem"], st and i[st], s)
    return out


@row("flowpath.sums", ["flowpath.downstream_sum", "flowpath.upslope_longest"], d8_field, _ref_pathsums)
def _(m, i):
    s = _frac_bits(i["weights"])
    out = {}
    for f in FIELDS:
        out["longest " + f] = m.flowpath.upslope_longest(i[f], i["weights"], i["dem"], s)
        for st in (None, "stop"):
            out["sum %s %s" % (f, st)] = m.flowpath.downstream_sum(i[f], i["weights"], i["dem"], st and i[st], s)
    return out


@cached
def _ref_watershed(i):
    import _watershed_ref as WS
    pour = (i["stop"] != 0) * (np.arange(H * W).reshape(H, W) % 7 + 1)
    out = {}
    for f in FIELDS:
        t, l, _ = WS.drainage(i[f], PX, i["dem"])
        tp, lp, lb = WS.drainage(i[f], PX, i["dem"], pour)
        out["target " + f], out["length " + f], out["basins " + f] = t, l, t
        out["target pour " + f], out["length pour " + f], out["watersheds " + f] = tp, lp, lb
        out["upslope " + f] = WS.upslope_length(i[f], PX, i["dem"])
    return out


@row("watershed", ["watershed.drainage", "watershed.basins", "watershed.watersheds", "watershed.upslope_length"], d8_field,
     _ref_watershed)
def _(m, i):
    pour = (i["stop"] != 0) * (np.arange(H * W).reshape(H, W) % 7 + 1)
    out = {}
    for f in FIELDS:
        out["target " + f], out["length " + f] = m.watershed.drainage(i[f], PX, i["dem"])
        out["target pour " + f], out["length pour " + f] = m.watershed.drainage(i[f], PX, i["dem"], pour)
        out["basins " + f] = m.watershed.basins(i[f], i["dem"])
        out["watersheds " + f] = m.watershed.watersheds(i[f], pour, i["dem"])
        out["upslope " + f] = m.watershed.upslope_length(i[f], PX, i["dem"])
    return out


def _network(i, f):
    """a river raster for field f: the cells many cells drain through, cycles and a block of non-river included"""
    import oracle
    acc = oracle.flowacc(i[f])
    river = ((acc > 6) | (acc < 0)).astype(np.int8)
    river[HOLE] = 0
    return river


@cached
def _ref_streams(i):
    import _streams_ref as ST
    out = {}
    for f in FIELDS:
        so, sh, lk = ST.reference(i[f], _network(i, f))
        out["strahler " + f], out["shreve " + f], out["link " + f], out["strahler alone " + f] = so, sh, lk, so
    return out


@row("streams", ["streams.stream_network", "streams.strahler"], d8_field, _ref_streams)
def _(m, i):
    out = {}
    for f in FIELDS:
        river = _network(i, f)
        out["strahler " + f], out["shreve " + f], out["link " + f] = m.streams.stream_network(i[f], river)
        out["strahler alone " + f] = m.streams.strahler(i[f], river)
    return out


# ---- tile-round ops: tests/_cost_ref.py, _morphology_ref.py, _proximity_ref.py ---------------------------------------
@cached
def cost_inputs(seed):
    import _cost_ref as CR
    f, s = CR.random_case((H, W), "uniform", seed)
    f[HOLE] = -100
    fs, ss = CR.serpentine((H, W))
    return Inputs(friction=f, sources=s, snake=fs, snake_sources=ss)


@cached
def _ref_cost(i):
    import _cost_ref as CR
    out = {}
    for name, f, s, conn in (("random", "friction", "sources", 8), ("four", "friction", "sources", 4),
                             ("snake", "snake", "snake_sources", 8)):
        c, idx, link, linkless, _ = CR.reference(i[f], i[s], PX, conn)
        assert linkless == 0
        out[name] = (c, idx, link)
        out[name + " plain"] = (c, idx)
    return out


@row("cost.cost_distance", ["cost.cost_distance"], cost_inputs, _ref_cost)
def _(m, i):
    out = {}
    for name, f, s, conn in (("random", "friction", "sources", 8), ("four", "friction", "sources", 4),
                             ("snake", "snake", "snake_sources", 8)):
        out[name] = tuple(m.cost.cost_distance(i[f], i[s], PX, connectivity=conn, backlink=True))
        out[name + " plain"] = tuple(m.cost.cost_distance(i[f], i[s], PX, connectivity=conn))[:2]
    return out


@cached
def morphology_inputs(seed):
    import _morphology_ref as MR
    marker, mask = MR.random_case((H, W), "nodata", seed)
    mask[HOLE] = -100
    smarker, smask = MR.serpentine(130)
    dem = MR.dem_with_voids((H, W), seed)
    dem[HOLE] = -100
    dem[60:68, 30:40] = 1.0  # a plateau split by a tile seam: a regional minimum
    return Inputs(marker=marker, mask=mask, snake_marker=smarker, snake_mask=smask, dem=dem)


@cached
def _ref_reconstruct(i):
    import _morphology_ref as MR
    out = {"%s/%d" % (kind, cn): MR.reconstruct(i["marker"], i["mask"], kind, cn)
           for kind in MR_KINDS for cn in (8, 4)}
    out["snake"] = MR.reconstruct(i["snake_marker"], i["snake_mask"])
    return out


MR_KINDS = ("dilation", "erosion")


@row("morphology.reconstruct", ["morphology.reconstruct"], morphology_inputs, _ref_reconstruct)
def _(m, i):
    out = {"%s/%d" % (kind, cn): np.asarray(m.morphology.reconstruct(i["marker"], i["mask"], kind=kind, connectivity=cn))
           for kind in MR_KINDS for cn in (8, 4)}
    out["snake"] = np.asarray(m.morphology.reconstruct(i["snake_marker"], i["snake_mask"]))
    return out


@cached
def _ref_morphology_derived(i):
    import _filters_ref as FR
    import _morphology_ref as MR
    dem = i["dem"]
    neg = np.where(MR.valid(dem), -dem, np.float32(np.nan))
    ex = FR.extremes(dem, 2)
    return {"fill": MR.priority_flood(dem, cn=8), "fill/4": MR.priority_flood(dem, cn=4),
            "hminima": MR.h_extrema(dem, 2.5, False, 8), "hmaxima": MR.h_extrema(dem, 2.5, True, 8),
            "regional_minima": MR.regional(dem, False, 8), "regional_maxima": MR.regional(neg, True, 8),
            "opening": MR.reconstruct(ex["min"], dem), "closing": MR.reconstruct(ex["max"], dem, "erosion")}


@row("morphology.derived", ["morphology.fill", "morphology.hminima", "morphology.hmaxima", "morphology.regional_minima",
                            "morphology.regional_maxima", "morphology.opening_by_reconstruction",
                            "morphology.closing_by_reconstruction"], morphology_inputs, _ref_morphology_derived)
def _(m, i):
    import _morphology_ref as MR
    mo, dem = m.morphology, i["dem"]
    neg = np.where(MR.valid(dem), -dem, np.float32(np.nan))
    out = {"fill": mo.fill(dem), "fill/4": mo.fill(dem, connectivity=4), "hminima": mo.hminima(dem, 2.5),
           "hmaxima": mo.hmaxima(dem, 2.5), "regional_minima": mo.regional_minima(dem),
           "regional_maxima": mo.regional_maxima(neg), "opening": mo.opening_by_reconstruction(dem, 2),
           "closing": mo.closing_by_reconstruction(dem, 2)}
    return {k: np.asarray(v) for k, v in out.items()}


@cached
def proximity_inputs(seed):
    rng = np.random.default_rng(seed)
    river = (rng.random((H, W)) < 0.01).astype(np.int8)
    river[HOLE] = 1  # sources on nodata are none
    return Inputs(river=river, dem=relief(seed, below=True), none=np.zeros((H, W), np.int8))


@cached
def _ref_proximity(i):
    import _proximity_ref as PR
    nod = i["dem"] <= -100
    out = {}
    for name, river, nodata in (("bare", i["river"], None), ("dem", i["river"], nod), ("none", i["none"], nod)):
        idx, dist, _ = PR.brute(river, nodata, PX)
        out[name] = (dist, idx)
    return out


@row("proximity.nearest_river", ["proximity.nearest_river"], proximity_inputs, _ref_proximity)
def _(m, i):
    return {"bare": tuple(m.proximity.nearest_river(i["river"], PX)),
            "dem": tuple(m.proximity.nearest_river(i["river"], PX, dem=i["dem"])),
            "none": tuple(m.proximity.nearest_river(i["none"], PX, dem=i["dem"]))}


# ---- the countdown ops: tests/_dinf_ref.py, _dinf_dist_ref.py, _mfd_ref.py, _routing_ref.py ----------------------------
@cached
def flow_inputs(seed):
    """relief with its pits, conditioned: the D-infinity angles and the MFD shares of the references, weights, a river"""
    import _dinf_ref as DR
    import _mfd_ref as MF
    w = world(seed)
    angle, _ = DR.flow_direction(w["filled"], PX, w["fdr"])
    shares = MF.flow_shares(w["filled"], 2, False, w["fdr"])
    rng = np.random.default_rng(seed + 7)
    weights = rng.random((H, W)) * 3.7
    weights[rng.random((H, W)) < 0.1] = 0.0
    pick = rng.random((H, W))
    decay = rng.uniform(0.5, 1.0, (H, W))
    decay[pick < 0.1], decay[pick > 0.9] = 0.0, 1.0
    cap = 40.0 * rng.uniform(0.0, 1.0, (H, W)) ** 2
    cap[pick < 0.1], cap[pick > 0.9] = 0.0, np.inf
    return Inputs(dem=w["dem"], filled=w["filled"], fdr=w["fdr"], river=w["river"], angle=angle, shares=shares,
                  weights=weights, decay=decay, capacity=cap)


@cached
def _ref_dinf_direction(i):
    import _dinf_ref as DR
    out = {}
    for name, dem, fdr in (("raw", i["dem"], None), ("cond", i["filled"], i["fdr"])):
        out[name] = DR.flow_direction(dem, PX, fdr)
    return out


def _bar_dinf_direction(got, want, inputs):
    """check_direction of tests/test_gpu_dinf.py: slope bit for bit, the angle's -1 and -100 masks equal, angles within
    one float32 spacing on at most 10 cells per million"""
    for name, (ra, rs) in want.items():
        ga, gs = got[name]
        same_bytes("dinf.flow_direction %s: slope" % name, gs, rs)
        assert ga.dtype == np.float32 and ga.shape == ra.shape
        for v in (-1.0, -100.0):
            assert np.array_equal(ga == np.float32(v), ra == np.float32(v)), "mask of angle == %g differs" % v
        diff = ga != ra
        assert (np.abs(ga[diff].astype(np.float64) - ra[diff].astype(np.float64)) <= np.spacing(ra[diff])).all()
        assert int(diff.sum()) * 1_000_000 <= 10 * ra.size, "%d of %d angles differ" % (int(diff.sum()), ra.size)


_bar_dinf_direction.whole = True


@row("dinf.flow_direction", ["dinf.flow_direction"], flow_inputs, _ref_dinf_direction, _bar_dinf_direction)
def _(m, i):
    return {"raw": tuple(m.dinf.flow_direction(i["dem"], PX)), "cond": tuple(m.dinf.flow_direction(i["filled"], PX, i["fdr"]))}


@cached
def _ref_dinf_accumulate(i):
    import _dinf_ref as DR
    return {"ones": DR.accumulate(i["angle"]), "weighted": DR.accumulate(i["angle"], i["weights"])}


@row("dinf.accumulate", ["dinf.accumulate"], flow_inputs, _ref_dinf_accumulate)
def _(m, i):
    return {"ones": m.dinf.accumulate(i["angle"]), "weighted": m.dinf.accumulate(i["angle"], i["weights"])}


DD_CASES = (("ave", True), ("min", False), ("max", True))


@cached
def _ref_dinf_distance(i):
    import _dinf_dist_ref as DD
    out = {"%s %s" % c: DD.distance_down(i["angle"], i["river"], PX, i["filled"], *c) for c in DD_CASES}
    out["flat"] = DD.distance_down(i["angle"], i["river"], PX, None, "ave", True)[:1]
    out["hand"] = out["ave True"][1]
    return out


@row("dinf.distance_down", ["dinf.distance_down", "dinf.hand"], flow_inputs, _ref_dinf_distance)
def _(m, i):
    out = {"%s %s" % c: tuple(m.dinf.distance_down(i["angle"], i["river"], PX, i["filled"], *c)) for c in DD_CASES}
    out["flat"] = tuple(m.dinf.distance_down(i["angle"], i["river"], PX))[:1]
    out["hand"] = m.dinf.hand(i["angle"], i["river"], i["filled"], PX)
    return out


@cached
def _ref_mfd_shares(i):
    import _mfd_ref as MF
    return {"plain": MF.flow_shares(i["dem"], 2), "contour": MF.flow_shares(i["filled"], 1, True, i["fdr"]),
            "d8": MF.d8_shares(i["fdr"])}


@row("mfd.flow_shares", ["mfd.flow_shares", "mfd.d8_shares"], flow_inputs, _ref_mfd_shares)
def _(m, i):
    return {"plain": m.mfd.flow_shares(i["dem"], 2), "contour": m.mfd.flow_shares(i["filled"], 1, True, i["fdr"]),
            "d8": m.mfd.d8_shares(i["fdr"])}


@cached
def _ref_mfd_accumulate(i):
    import _mfd_ref as MF
    return {"ones": MF.accumulate(i["shares"]), "weighted": MF.accumulate(i["shares"], i["weights"])}


@row("mfd.accumulate", ["mfd.accumulate"], flow_inputs, _ref_mfd_accumulate)
def _(m, i):
    return {"ones": m.mfd.accumulate(i["shares"]), "weighted": m.mfd.accumulate(i["shares"], i["weights"])}


ROUTES = (("shares", "decay", "decay"), ("shares", "capacity", "retain"), ("shares", "capacity", "limit"),
          ("angle", "decay", "decay"), ("angle", "capacity", "retain"), ("angle", "capacity", "limit"),
          ("fdr", "capacity", "retain"))


@cached
def _ref_route(i):
    import _mfd_ref as MF
    import _routing_ref as RR
    out = {}
    for flow, param, transfer in ROUTES:
        f = MF.d8_shares(i[flow]) if flow == "fdr" else i[flow]
        r = RR.route(f, i[param], transfer, i["weights"])
        out["%s %s" % (flow, transfer)] = {k: r[k] for k in RR.OUTPUTS}
    return out


@row("routing.route", ["routing.route"], flow_inputs, _ref_route)
def _(m, i):
    import _routing_ref as RR
    return {"%s %s" % (flow, transfer): dict(m.routing.route(i[flow], i[param], transfer, i["weights"], outputs=RR.OUTPUTS))
            for flow, param, transfer in ROUTES}


# ---- wetness: tests/_wetness_ref.py --------------------------------------------------------------------------------
@cached
def wetness_inputs(seed):
    import _wetness_ref as WR
    a, s = WR.random_case((H, W), "plateau", seed)
    a[HOLE] = -100.0
    sa, ss = WR.serpentine((H, W))
    rng = np.random.default_rng(seed + 3)
    sl = (rng.random((H, W)) ** 3 * 1.2).astype(np.float32)
    sl.reshape(-1)[:7] = [0.0, 1e-4, 0.1, 1.0, 1.5, np.pi / 2, -100.0]
    bad = rng.random((H, W)) < 0.03
    bad.reshape(-1)[:7] = False
    sl[bad] = rng.choice(np.array([np.nan, -100.0, 1.6, -1e-6, np.inf], np.float32), int(bad.sum()))
    return Inputs(area=a, suction=s, snake_area=sa, snake_suction=ss, slope=sl)


@cached
def _ref_wetness_modified(i):
    import _wetness_ref as WR
    return {"random": WR.reference(i["area"], i["suction"]), "snake": WR.reference(i["snake_area"], i["snake_suction"])}


@row("wetness.modified_catchment_area", ["wetness.modified_catchment_area"], wetness_inputs, _ref_wetness_modified)
def _(m, i):
    return {"random": np.asarray(m.wetness.modified_catchment_area(i["area"], i["suction"])),
            "snake": np.asarray(m.wetness.modified_catchment_area(i["snake_area"], i["snake_suction"]))}


@cached
def _ref_wetness_saga(i):
    import _wetness_ref as WR
    return {"suction": WR.suction(i["slope"])}


def _spacing_ok(name, g, r):
    """tests/test_gpu_wetness.py: -100 on exactly the reference's cells, elsewhere at most one float32 spacing apart"""
    assert g.dtype == np.float32 and r.dtype == np.float32 and g.shape == r.shape
    assert np.array_equal(g == -100, r == -100), name
    assert not np.isnan(g).any(), name
    tol = np.spacing(np.maximum(np.abs(g), np.abs(r)))
    diff = np.abs(g.astype(np.float64) - r.astype(np.float64))
    assert (diff <= tol).all(), "%s: %d cells beyond one float32 spacing" % (name, int((diff > tol).sum()))


def _bar_wetness_saga(got, want, i):
    """test_saga_wetness_index: the suction against numpy; the modified area against the reference run on the suction
    plane the call itself produced; the index against numpy on that reference"""
    import _wetness_ref as WR
    _spacing_ok("suction", got["suction"], want["suction"])
    M = WR.reference(i["area"], got["suction"])
    same_bytes("modified", got["modified"], M)
    _spacing_ok("swi", got["swi"], WR.swi(M, i["slope"]))
    assert got["plain"].tobytes() == got["swi"].tobytes()


_bar_wetness_saga.whole = True


@row("wetness.saga_wetness_index", ["wetness.suction", "wetness.saga_wetness_index"], wetness_inputs, _ref_wetness_saga,
     _bar_wetness_saga)
def _(m, i):
    swi, M = m.wetness.saga_wetness_index(i["area"], i["slope"], modified=True)
    return {"suction": m.wetness.suction(i["slope"]), "swi": swi, "modified": np.asarray(M),
            "plain": m.wetness.saga_wetness_index(i["area"], i["slope"])}


# ---- window ops: tests/_filters_ref.py, _focal_ref.py, _terrain_ref.py, _horizon_ref.py, _mrvbf_ref.py ----------------
def nan_same(what, got, want):
    """the ops' _assert_same: dtype and shape, NaN on the same cells, every other cell bit for bit"""
    for (p, g), (_, w) in zip(leaves(got), leaves(want)):
        assert g.dtype == w.dtype and g.shape == w.shape, what + p
        if g.dtype.kind == "f":
            gn, wn = np.isnan(g), np.isnan(w)
            assert np.array_equal(gn, wn), "%s%s: NaN positions differ at %d cells" % (what, p, int((gn != wn).sum()))
            g, w = np.where(gn, 0, g).astype(g.dtype), np.where(wn, 0, w).astype(w.dtype)
        same_bytes(what + p, g, w)


@cached
def window_inputs(seed):
    """_focal_ref.terrain (holes of nodata) with the nodata block, between 100 and 130 m as the MRVBF tests take it"""
    import _focal_ref as FO
    dem = FO.terrain(H, W, seed, holes=True, lo=100.0, hi=130.0).copy()
    dem[HOLE] = -100
    return Inputs(dem=dem)


@cached
def _ref_filters_extremes(i):
    import _filters_ref as FR
    out = {}
    for r in (3, 70):
        out["extremes %d" % r] = FR.extremes(i["dem"], r)
        out["opening %d" % r], out["closing %d" % r] = FR.opening(i["dem"], r), FR.closing(i["dem"], r)
    return out


@row("filters.extremes", ["filters.extremes", "filters.opening", "filters.closing"], window_inputs, _ref_filters_extremes)
def _(m, i):
    out = {}
    for r in (3, 70):
        out["extremes %d" % r] = dict(m.filters.extremes(i["dem"], r, ("min", "max", "range")))
        out["opening %d" % r], out["closing %d" % r] = m.filters.opening(i["dem"], r), m.filters.closing(i["dem"], r)
    return out


QS = (0, 10, 50, 100)


@cached
def _ref_filters_percentile(i):
    import _filters_ref as FR
    return {"r%d" % r: list(FR.percentiles(i["dem"], r, QS)) for r in (1, 4)}


@row("filters.percentile", ["filters.percentile"], window_inputs, _ref_filters_percentile)
def _(m, i):
    return {"r%d" % r: [m.filters.percentile(i["dem"], r, q) for q in QS] for r in (1, 4)}


@cached
def _ref_filters_denoise(i):
    import _filters_ref as FR
    return {"default": FR.denoise(i["dem"], 2.0), "tight": FR.denoise(i["dem"], 2.0, 2, 15.0, 2, 0.05)}


@row("filters.denoise", ["filters.denoise"], window_inputs, _ref_filters_denoise)
def _(m, i):
    return {"default": m.filters.denoise(i["dem"], 2.0), "tight": m.filters.denoise(i["dem"], 2.0, 2, 15.0, 2, 0.05)}


FOCAL_BITS = 8
FOCAL_OUTPUTS = ("count", "mean", "std", "tpi", "dev")


@cached
def _ref_focal(i):
    import _focal_ref as FO
    o = FO.default_origin(i["dem"])
    out = {"r%d" % r: FO.statistics(i["dem"], r, o, FOCAL_BITS) for r in (2, 64)}
    out["dev_max"] = FO.dev_max(i["dem"], (1, 3, 10, 40), o, FOCAL_BITS)
    return out


@row("focal.statistics", ["focal.statistics", "focal.dev_max"], window_inputs, _ref_focal, nan_same)
def _(m, i):
    import _focal_ref as FO
    o = FO.default_origin(i["dem"])
    out = {"r%d" % r: dict(m.focal.statistics(i["dem"], r, FOCAL_OUTPUTS, FOCAL_BITS, o)) for r in (2, 64)}
    out["dev_max"] = tuple(m.focal.dev_max(i["dem"], (1, 3, 10, 40), FOCAL_BITS, o))
    return out


def _aspect_close(name, g, r):
    """tests/test_gpu_terrain.py: -100 and -1 on the same cells, elsewhere one float32 spacing round the circle, and at
    most 16 cells that differ at all"""
    assert g.dtype == r.dtype == np.float32 and g.shape == r.shape, name
    assert np.array_equal(g == -100, r == -100), name + ": cells without a value differ"
    assert np.array_equal(g == -1, r == -1), name + ": flat cells differ"
    live = r >= 0
    assert ((g[live] >= 0) & (g[live] < 360)).all(), name
    g64, r64 = g[live].astype(np.float64), r[live].astype(np.float64)
    d = np.abs(g64 - r64)
    d = np.minimum(d, 360.0 - d)
    tol = np.spacing(np.maximum(g[live], r[live])).astype(np.float64)
    assert (d <= tol).all(), "%s: an aspect is off by %r" % (name, float((d - tol).max()))
    assert int((g64 != r64).sum()) <= 16, name


TERRAIN_OUTPUTS = ("gradient", "aspect", "profile", "plan", "tangential", "mean", "laplacian", "hillshade")


@cached
def _ref_terrain(i):
    import _terrain_ref as TR
    return {"r%d %s" % (r, k): v for r in (1, 3) for k, v in TR.attributes(i["dem"], PX, TERRAIN_OUTPUTS, r).items()}


@row("terrain.attributes", ["terrain.attributes"], window_inputs, _ref_terrain,
     {"r%d aspect" % r: _aspect_close for r in (1, 3)})
def _(m, i):
    return {"r%d %s" % (r, k): v for r in (1, 3) for k, v in m.terrain.attributes(i["dem"], PX, TERRAIN_OUTPUTS, r).items()}


def _openness_close(name, g, r):
    """tests/test_gpu_horizon.py: -100 on the same cells, elsewhere within one float32 spacing, at most 16 cells differ"""
    assert g.dtype == r.dtype == np.float32 and g.shape == r.shape, name
    assert np.array_equal(g == -100, r == -100), name + ": cells without a value differ"
    live = r != -100
    g64, r64 = g[live].astype(np.float64), r[live].astype(np.float64)
    assert ((g64 > 0) & (g64 < np.pi)).all(), name
    tol = np.spacing(np.maximum(g[live], r[live])).astype(np.float64)
    d = np.abs(g64 - r64)
    assert (d <= tol).all(), "%s: a value is off by %r" % (name, float((d - tol).max()))
    assert int((g64 != r64).sum()) <= 16, name


HORIZON_OUTPUTS = ("landform", "pattern", "positive", "negative", "sky_view")


@cached
def _ref_horizon(i):
    import _horizon_ref as HR
    out = {}
    for r, skip in ((3, 0), (10, 2)):
        for k, v in HR.attributes(i["dem"], PX, HR.flat_tangent(1.0), HORIZON_OUTPUTS, r, skip).items():
            out["r%d %s" % (r, k)] = v
    return out


@row("horizon.attributes", ["horizon.attributes"], window_inputs, _ref_horizon,
     {"r%d %s" % (r, k): _openness_close for r in (3, 10) for k in ("positive", "negative")})
def _(m, i):
    out = {}
    for r, skip in ((3, 0), (10, 2)):
        for k, v in m.horizon.attributes(i["dem"], PX, HORIZON_OUTPUTS, radius=r, skip=skip).items():
            out["r%d %s" % (r, k)] = v
    return out


MRVBF_PX = 30.0


def _one_spacing(what, got, want):
    """tests/test_gpu_mrvbf.py, BOUND = 1: -100 on the same cells, no NaN, at most one float32 spacing apart"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and not np.isnan(got).any(), what
    assert np.array_equal(got == -100, want == -100), what
    d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert d.max() <= 1, "%s: %d cells beyond the bound, the worst by %d spacings" % (what, int((d > 1).sum()), int(d.max()))


@cached
def _ref_mrvbf(i):
    import _mrvbf_ref as MV
    out = {"levels %s %s" % (lv, k): v for lv in (None, 2)
           for k, v in MV.indices(i["dem"], MRVBF_PX, ("mrvbf", "mrrtf"), levels=lv).items()}
    return out


@row("mrvbf.indices", ["mrvbf.indices"], window_inputs, _ref_mrvbf,
     {"levels %s %s" % (lv, k): _one_spacing for lv in (None, 2) for k in ("mrvbf", "mrrtf")})
def _(m, i):
    return {"levels %s %s" % (lv, k): v for lv in (None, 2)
            for k, v in m.mrvbf.indices(i["dem"], MRVBF_PX, ("mrvbf", "mrrtf"), levels=lv).items()}


@cached
def _ref_mrvbf_parts(i):
    import _mrvbf_ref as MV
    out = {}
    for r in (3, 16):
        ok, lo, hi = MV.percentile64(i["dem"], r)
        out["lower %d" % r] = np.where(ok, lo.astype(np.float32), np.float32(-100))
        out["higher %d" % r] = np.where(ok, hi.astype(np.float32), np.float32(-100))
    out["coarsen"] = tuple(MV.coarsen(i["dem"], 7.3))
    return out


@row("mrvbf.parts", ["mrvbf.elevation_percentile", "mrvbf.coarsen"], window_inputs, _ref_mrvbf_parts)
def _(m, i):
    out = {}
    for r in (3, 16):
        out["lower %d" % r] = m.mrvbf.elevation_percentile(i["dem"], r, "lower")
        out["higher %d" % r] = m.mrvbf.elevation_percentile(i["dem"], r, "higher")
    out["coarsen"] = tuple(m.mrvbf.coarsen(i["dem"], 7.3))
    return out


# ---- harmonic and inundation: tests/_harmonic_ref.py, _inundation_ref.py ---------------------------------------------
HARMONIC_TOL = 1e-5


@cached
def harmonic_inputs(seed):
    """test_gpu_harmonic.py's larger case at 130 x 67: a domain with 10 % holes, a hole on the corner of four tiles, a
    wall, the nodata block; 0.5 % of the cells fixed"""
    rng = np.random.default_rng(seed)
    dom = rng.random((H, W)) >= 0.10
    dom[62:67, 30:35] = False
    dom[100:103, 10:60] = False
    dom[HOLE] = False
    fixed = dom & (rng.random((H, W)) < 0.005)
    v = np.where(fixed, rng.normal(0.0, 300.0, (H, W)), 0.0).astype(np.float32)
    return Inputs(values=v, fixed=fixed.astype(np.int8), domain=dom.astype(np.int8))


@cached
def _ref_harmonic(i):
    import _harmonic_ref as HR
    return {"reach": HR.reachable(i["fixed"] != 0, i["domain"] != 0)}


def _bar_harmonic(got, want, i):
    """_check of tests/test_gpu_harmonic.py: NaN exactly off the reachable set, fixed cells carry their value, the
    residual the reference measures on the field is within tol and is the one the call reports"""
    import _harmonic_ref as HR
    u, reach, fixed = got["field"], want["reach"], i["fixed"] != 0
    assert u.dtype == np.float64 and u.shape == (H, W)
    assert np.array_equal(np.isnan(u), ~reach), "NaN exactly outside the domain and on the cells without a value"
    same_bytes("fixed cells", u[fixed], i["values"][fixed].astype(np.float64))
    r = HR.residual(np.where(reach, u, 0.0), fixed, reach)
    assert r.max() <= HARMONIC_TOL
    info = got["info"]
    assert info["residual"] == r.max() and info["converged"]
    assert info["unreached"] == int(((i["domain"] != 0) & ~reach).sum()) and info["levels"] >= 2


_bar_harmonic.whole = True


@row("harmonic.interpolate", ["harmonic.interpolate"], harmonic_inputs, _ref_harmonic, _bar_harmonic)
def _(m, i):
    got = m.harmonic.interpolate(i["values"], i["fixed"], i["domain"], tol=HARMONIC_TOL)
    return {"field": got.field, "info": got.info}


@cached
def inundation_inputs(seed):
    """_inundation_ref.rough_terrain's recipe at 130 x 67 with the nodata block, rain and one inflow hydrograph"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    dem = (0.02 * x + 0.01 * y + 0.3 * rng.random((H, W))).astype(np.float32)
    dem[HOLE] = -100.0
    cell = 35 * W + 3
    return Inputs(dem=dem, valid=dem > -100, cell=np.array([cell]), times=np.array([0.0]), q=np.array([[20.0]]))


INUNDATION_T, INUNDATION_RAIN = 240.0, 50e-3 / 3600.0
INUNDATION_STATE = ("depth", "qx", "qy", "max_depth", "arrival")
INUNDATION_INFO = ("steps", "t", "finished", "hmax", "dt_last", "dt_min", "limited_steps")  # test_gpu_inundation._same


@cached
def _ref_inundation(i):
    import _inundation_ref as IR
    out = {}
    for boundary in ("closed", "open"):
        ref = IR.simulate(i["dem"].astype(np.float64), i["valid"], PX, INUNDATION_T, rain=INUNDATION_RAIN,
                          inflow=(i["cell"], i["times"], i["q"]), boundary=boundary)
        assert ref["finished"] and ref["steps"] >= 20
        out[boundary] = {k: np.asarray(ref[k], np.float64) for k in INUNDATION_STATE}
        out[boundary + " masked"] = (np.where(i["valid"], ref["depth"], -100.0), np.where(i["valid"], ref["max_depth"], -100.0),
                                     np.asarray(ref["arrival"], np.float64))
        out[boundary + " info"] = {k: np.asarray(ref[k]) for k in INUNDATION_INFO}
        out[boundary + " info"]["volume"] = np.asarray(math.fsum((ref["depth"][i["valid"]] * (PX * PX)).tolist()))
    return out


def info_equal(what, got, want):
    """the info words by value, as the op's test compares them (==)"""
    assert list(got) == list(want), what
    for k in want:
        assert np.asarray(got[k]).item() == np.asarray(want[k]).item(), "%s: %s is %r, the reference has %r" % (what, k, got[k], want[k])


@row("inundation.simulate", ["inundation.simulate"], inundation_inputs, _ref_inundation,
     {b + " info": info_equal for b in ("closed", "open")})
def _(m, i):
    out = {}
    for boundary in ("closed", "open"):
        got = m.inundation.simulate(i["dem"], PX, INUNDATION_T, rain=INUNDATION_RAIN, inflow=(i["cell"], i["times"], i["q"]),
                                    boundary=boundary, outputs=("depth", "max_depth", "arrival"))
        out[boundary] = {k: np.asarray(got.state[k], np.float64) for k in INUNDATION_STATE}
        out[boundary + " masked"] = (got.depth, got.max_depth, got.arrival)
        out[boundary + " info"] = {k: np.asarray(got.info[k]) for k in INUNDATION_INFO + ("volume",)}
        assert got.state["steps"] == got.info["steps"] and got.state["t"] == got.info["t"]
    return out


# ---- regions and reaches: tests/_regions_ref.py, _reaches_ref.py -------------------------------------------------------
@cached
def regions_inputs(seed):
    """noise at the percolation threshold (regions that wind through every tile), the serpentine, the nodata block"""
    import _regions_ref as RG
    rng = np.random.default_rng(seed)
    noise = (rng.random((H, W)) < 0.45).astype(np.uint8)
    noise[HOLE] = 0
    seeds = (rng.random((H, W)) < 0.01).astype(np.uint8)
    return Inputs(noise=noise, snake=np.asarray(RG.serpentine(H, W)), seeds=seeds)


@cached
def _ref_regions(i):
    import _regions_ref as RG
    out = {}
    for name in ("noise", "snake"):
        for cn in (8, 4):
            lab = RG.flood(i[name], cn)
            out["label %s/%d" % (name, cn)], out["sizes %s/%d" % (name, cn)] = lab, (lab, RG.sizes(lab))
            out["connected %s/%d" % (name, cn)] = RG.connected(i[name], i["seeds"], cn, 3)
            out["sieve %s/%d" % (name, cn)] = RG.sieve(i[name], 5, cn)
    return out


@row("regions", ["regions.label", "regions.connected", "regions.sieve"], regions_inputs, _ref_regions)
def _(m, i):
    out = {}
    for name in ("noise", "snake"):
        for cn in (8, 4):
            out["label %s/%d" % (name, cn)] = m.regions.label(i[name], cn)
            out["sizes %s/%d" % (name, cn)] = tuple(m.regions.label(i[name], connectivity=cn, sizes=True))
            out["connected %s/%d" % (name, cn)] = m.regions.connected(i[name], i["seeds"], cn, 3)
            out["sieve %s/%d" % (name, cn)] = m.regions.sieve(i[name], 5, cn)
    return out


FEET = 0.3048


@cached
def reach_inputs(seed):
    """the conditioned world with its network: links, river index, HAND, slope; 84 stages a foot apart and 4 coarse"""
    import _reaches_ref as RC
    w = world(seed)
    link, idx, hand = RC.network(w["dem"], w["fdr"], w["river"])
    reach, cat, heads = RC.catchments(link, idx)
    assert heads.size >= 4
    rng = np.random.default_rng(seed)
    stage = rng.uniform(0.0, 6.0, heads.size)
    stage[::5] = 0.0
    return Inputs(fdr=w["fdr"], river=w["river"], slope=w["slope"], link=link, idx=idx, hand=hand, reach=reach, cat=cat,
                  heads=heads, stages=np.arange(84) * FEET, coarse=np.arange(1, 5) * 2.0, stage=stage)


def _tables(RC, i, stages, slope):
    nr = i["heads"].size
    s = RC.default_frac_bits(i["cat"].size, stages, slope)
    cells, hq, bq, _ = RC.tables(i["cat"], i["hand"], stages, nr, s, slope)
    return (cells,) + tuple(RC.derive(stages, cells, hq, bq, PX, s))


@cached
def _ref_reaches(i):
    import _reaches_ref as RC
    import _regions_ref as RG
    nr = i["heads"].size
    out = {"catchments": tuple(RC.catchments(i["link"], i["idx"])),
           "channels": tuple(RC.channels(i["fdr"], i["reach"], PX, nr)),
           "inundate": RC.inundate(i["cat"], i["hand"], i["stage"]),
           "inundate64": RC.inundate(i["cat"], i["hand"].astype(np.float64), i["stage"]),
           "connected": RG.inundate_connected(i["cat"], i["hand"], i["stage"], i["river"], 8)[0],
           "connected/4": RG.inundate_connected(i["cat"], i["hand"], i["stage"], i["river"], 4)[0]}
    for slots in (0, 1, -1):
        out["tables slope, slots %d" % slots] = _tables(RC, i, i["stages"], i["slope"])
        out["tables coarse, slots %d" % slots] = _tables(RC, i, i["coarse"], None)
    return out


@row("reaches", ["reaches.catchments", "reaches.channels", "reaches.hydraulic_tables", "reaches.inundate",
                 "reaches.inundate_connected"], reach_inputs, _ref_reaches)
def _(m, i):
    from descriptools_amd import _lib
    rc, nr = m.reaches, i["heads"].size
    out = {"catchments": tuple(rc.catchments(i["link"], i["idx"])),
           "channels": tuple(rc.channels(i["fdr"], i["reach"], PX, nr)),
           "inundate": rc.inundate(i["cat"], i["hand"], i["stage"]),
           "inundate64": rc.inundate(i["cat"], i["hand"].astype(np.float64), i["stage"]),
           "connected": rc.inundate_connected(i["cat"], i["hand"], i["stage"], i["river"]),
           "connected/4": rc.inundate_connected(i["cat"], i["hand"], i["stage"], i["river"], connectivity=4)}
    for slots in (0, 1, -1):  # DT_DBG_RC_SLOTS: the LDS table, capped at one slot, and absent (one global atomic per cell)
        _lib.check(_lib.lib().dt_debug_set(10, slots))
        try:
            for name, stages, slope in (("slope", i["stages"], i["slope"]), ("coarse", i["coarse"], None)):
                t = rc.hydraulic_tables(i["cat"], i["hand"], PX, stages, nr, slope=slope)
                out["tables %s, slots %d" % (name, slots)] = (t.cells, t.area, t.volume, t.bed_area)
        finally:
            _lib.check(_lib.lib().dt_debug_set(10, 0))
    return out


# ---- zonal: tests/_zonal_ref.py (the generators are test_gpu_zonal.py's) ----------------------------------------------
SLOTS = (0, 3, -1)  # DT_DBG_RC_SLOTS: the LDS table, capped at three slots (it overflows), absent


class _slots:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from descriptools_amd import _lib
        _lib.check(_lib.lib().dt_debug_set(10, self.n))

    def __exit__(self, *exc):
        from descriptools_amd import _lib
        _lib.check(_lib.lib().dt_debug_set(10, 0))


@cached
def zonal_inputs(seed):
    """values from -60 to 940 with NaN, +-inf, -100 and -0.0; zonings of a few blocks (the direct LDS table), stripes,
    one zone per cell (the table in global memory), and 256 / 257 zones on one tile: the two sides of the threshold
    between the direct and the claimed LDS table"""
    rng = np.random.default_rng(seed)
    v = (rng.random((H, W)) * 1000 - 60).astype(np.float32)
    r = rng.random((H, W))
    v[r < 0.04] = np.nan
    v[(r >= 0.04) & (r < 0.06)] = np.inf
    v[(r >= 0.06) & (r < 0.08)] = -np.inf
    v[(r >= 0.08) & (r < 0.12)] = -100.0
    v[0, 0], v[0, 1] = -0.0, 0.0
    yy, xx = np.mgrid[0:H, 0:W]
    nbx = (W + 17) // 64 + 1
    z = {"blocks": (((yy + 31) // 64) * nbx + (xx + 17) // 64, ((H + 31) // 64 + 1) * nbx),
         "stripes3": (xx // 3, (W + 2) // 3), "cells": (rng.permutation(H * W).reshape(H, W), H * W)}
    out = Inputs(values=v, names=("blocks", "stripes3", "cells", "z256", "z257"))
    for k, (zones, n) in z.items():
        zones = np.ascontiguousarray(zones, np.int32)
        zones[HOLE] = -100
        out[k], out["n " + k] = zones, np.int64(n)
    one = (np.arange(64 * 64, dtype=np.int32) % 256).reshape(64, 64)
    out["z256"], out["n z256"], out["z257"], out["n z257"] = one, np.int64(256), one + 1, np.int64(257)
    out["v64"] = np.ascontiguousarray(v[:64, :64])
    out["labels"] = rng.choice(np.array([0, 31, 32, 63, 64, 4095, 4096, 70000, -1, -100]), (H, W)).astype(np.int64)
    out["classes"] = rng.integers(-1, 10, (H, W)).astype(np.int32)
    out["edges"] = np.sort(rng.random(17) * 900 - 50)
    out["table"] = (rng.random(50) * 1e6 - 5e5).astype(np.float32)
    out["table"][:3] = [np.inf, -0.0, np.nan]
    out["paint"] = rng.integers(-3, 53, (H, W)).astype(np.int32)
    return out


def _zv(i, name):
    return i[name], (i["v64"] if name.startswith("z2") else i["values"]), int(i["n " + name])


@cached
def _ref_zonal_tables(i):
    import _zonal_ref as ZR
    out = {}
    for k, name in enumerate(i["names"]):
        zones, v, nz = _zv(i, name)
        nodata, origin = (None, 300.5) if k % 2 else (-100.0, None)
        o, s = ZR.default_scale(zones, v, nz, nodata, None, origin)
        r = ZR.tables(zones, v, nz, o, s, nodata)
        assert r["out"] == 0
        st = ZR.statistics(r, o, s)
        for n in SLOTS:
            out["%s, slots %d" % (name, n)] = tuple(r[f] for f in ("count", "s1", "s2_lo", "s2_hi", "vmin", "vmax"))
            out["statistics %s, slots %d" % (name, n)] = {f: st[f] for f in ZONAL_OUTPUTS}
    return out


ZONAL_OUTPUTS = ("count", "sum", "mean", "std", "min", "max", "range")


@row("zonal.tables", ["zonal.tables", "zonal.statistics"], zonal_inputs, _ref_zonal_tables)
def _(m, i):
    out = {}
    for k, name in enumerate(i["names"]):
        zones, v, nz = _zv(i, name)
        nodata, origin = (None, 300.5) if k % 2 else (-100.0, None)
        for n in SLOTS:
            with _slots(n):
                out["%s, slots %d" % (name, n)] = tuple(m.zonal.tables(zones, v, nz, origin=origin, nodata=nodata))[:6]
                out["statistics %s, slots %d" % (name, n)] = dict(
                    m.zonal.statistics(zones, v, nz, ZONAL_OUTPUTS, origin=origin, nodata=nodata))
    return out


@cached
def _ref_zonal_counts(i):
    import _zonal_ref as ZR
    out = {"compact": tuple(ZR.compact(i["labels"], 70000)), "compact all": tuple(ZR.compact(i["labels"])),
           "paint nan": ZR.paint(i["table"], i["paint"], np.nan), "paint -100": ZR.paint(i["table"], i["paint"], -100.0)}
    b = (i["values"] > 300).astype(np.int32)
    for n in SLOTS:
        for name in ("blocks", "cells"):
            zones, v, nz = _zv(i, name)
            out["histogram %s, slots %d" % (name, n)] = ZR.histogram(zones, v, nz, i["edges"])
        out["crosstab, slots %d" % n] = ZR.crosstab(i["classes"], b, 10, 2)
        out["crosstab wide, slots %d" % n] = ZR.crosstab(i["stripes3"], i["classes"], int(i["n stripes3"]), 10)
    return out


@row("zonal.counts", ["zonal.compact", "zonal.histogram", "zonal.crosstab", "zonal.paint"], zonal_inputs, _ref_zonal_counts)
def _(m, i):
    z = m.zonal
    out = {"compact": tuple(z.compact(i["labels"], 70000)), "compact all": tuple(z.compact(i["labels"])),
           "paint nan": z.paint(i["table"], i["paint"], np.nan), "paint -100": z.paint(i["table"], i["paint"], -100.0)}
    b = (i["values"] > 300).astype(np.int32)
    for n in SLOTS:
        with _slots(n):
            for name in ("blocks", "cells"):
                zones, v, nz = _zv(i, name)
                out["histogram %s, slots %d" % (name, n)] = z.histogram(zones, v, nz, i["edges"])
            out["crosstab, slots %d" % n] = z.crosstab(i["classes"], b, 10, 2)
            out["crosstab wide, slots %d" % n] = z.crosstab(i["stripes3"], i["classes"], int(i["n stripes3"]), 10)
    return out


# ---- resample and vector: tests/_resample_ref.py, _vector_ref.py, _polygonize_ref.py and their case files -------------
WARPS = (((-0.3, 67 / 40, 0.0, 0.2, 0.0, 130 / 33), (33, 40)),   # down, ragged
         ((-3.5, 0.37, 0.0, 2.25, 0.0, 0.41), (259, 200)),       # up, past two edges
         ((5.0, 0.6, 0.8, -20.0, -0.8, 0.6), (150, 120)))        # rotated: the point methods only
FLOAT_METHODS = ("nearest", "bilinear", "cubic", "average", "sum", "min", "max")
POINT_METHODS = FLOAT_METHODS[:3]


def _warp_methods(matrix):
    return FLOAT_METHODS if matrix[2] == 0.0 and matrix[4] == 0.0 else POINT_METHODS


@cached
def resample_inputs(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = (300.0 + 40.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.uniform(-3.0, 3.0, (H, W))).astype(np.float32)
    z[HOLE] = -100.0
    z[20:24, 20:24] = (1e6 * rng.uniform(-1.0, 1.0, (4, 4))).astype(np.float32)  # a spike: cubic overshoots, sums cancel
    z[100, :] = -100.0
    z[7, 7], z[8, 40] = np.nan, -1e30
    classes = rng.integers(0, 12, (H, W)).astype(np.uint8)
    return Inputs(z=z, z64=z.astype(np.float64), classes=classes)


@cached
def _ref_resample(i):
    import _resample_ref as RS
    out = {}
    for k, (matrix, shape) in enumerate(WARPS):
        for method in _warp_methods(matrix):
            out["%s %d" % (method, k)] = RS.warp(i["z"], matrix, shape, method)
        if len(_warp_methods(matrix)) > 3:
            out["mode %d" % k] = RS.warp(i["classes"], matrix, shape, "mode", nodata=3, fill=77)
    out["cubic f64"] = RS.warp(i["z64"], *WARPS[0], "cubic")
    for how in ("average", "sum", "min", "max"):
        out["aggregate " + how] = RS.aggregate(i["z"], (2, 3), how)
    out["aggregate mode"] = RS.aggregate(i["classes"], 8, "mode")
    out["resize"] = RS.resize(i["z"], (131, 126), "bilinear")
    return out


@row("resample.warp", ["resample.warp"], resample_inputs, _ref_resample)
def _(m, i):
    rs = m.resample
    out = {}
    for k, (matrix, shape) in enumerate(WARPS):
        for method in _warp_methods(matrix):
            out["%s %d" % (method, k)] = rs.warp(i["z"], matrix, shape, method)
        if len(_warp_methods(matrix)) > 3:
            out["mode %d" % k] = rs.warp(i["classes"], matrix, shape, "mode", nodata=3, fill=77)
    out["cubic f64"] = rs.warp(i["z64"], *WARPS[0], "cubic")
    for how in ("average", "sum", "min", "max"):
        out["aggregate " + how] = rs.aggregate(i["z"], (2, 3), how)
    out["aggregate mode"] = rs.aggregate(i["classes"], 8, "mode")
    out["resize"] = rs.resize(i["z"], (131, 126), "bilinear")
    return out


RASTERIZE = (("polygon", "two holes", 8, False), ("polygon", "five overlapping", 8, False), ("polygon", "tessellation", 8, False),
             ("polygon", "partly outside", 8, False), ("polygon", "concave", 4, True), ("polygon", "far vertices", 8, True),
             ("line", "random walk", 8, False), ("line", "random walk", 4, False), ("line", "octants", 8, False),
             ("point", "points", 8, False))


def _vector_case(group, name):
    import _vector_cases as VC
    return {"polygon": VC.polygon_cases, "line": VC.line_cases, "point": VC.point_cases}[group]()[name]


@cached
def vector_inputs(seed):
    return Inputs({"%s %s" % (g, n): tuple(_vector_case(g, n)[1:4]) for g, n, _, _ in RASTERIZE})


def _ref_rasterize(cases):
    import _vector_ref as VR
    return {"%s %s /%d %s" % c: VR.rasterize(*_vector_case(*c[:2]), connectivity=c[2], all_touched=c[3]) for c in cases}


def _call_rasterize(m, cases):
    out = {}
    for c in cases:
        case = _vector_case(*c[:2])
        out["%s %s /%d %s" % c] = m.vector.rasterize(m.vector.Geometry(*case[:4]), case[4], c[2], c[3])
    return out


@row("vector.rasterize", ["vector.rasterize"], vector_inputs, lambda i: _ref_rasterize(RASTERIZE))
def _(m, i):
    return _call_rasterize(m, RASTERIZE)


@cached
def comb_inputs(seed):
    """_vector_cases.comb_case: 20,000 crossings on each of 40 rows, more than the LDS kernels sort: the slow rows in
    global memory; and 3,000 teeth, the large LDS kernel"""
    import _vector_cases as VC
    return Inputs(comb=tuple(VC.comb_case()[1:4]), comb3000=tuple(VC.comb_case(3000)[1:4]))


@cached
def _ref_comb(i):
    import _vector_cases as VC
    import _vector_ref as VR
    return {"slow rows": VR.rasterize(*VC.comb_case()), "large": VR.rasterize(*VC.comb_case(3000))}


@row("vector.rasterize[slow rows]", ["vector.rasterize"], comb_inputs, _ref_comb)
def _(m, i):
    import _vector_cases as VC
    out = {}
    for name, case in (("slow rows", VC.comb_case()), ("large", VC.comb_case(3000))):
        got, info = m.vector.rasterize(m.vector.Geometry(*case[:4]), case[4], return_info=True)
        out[name], out[name + " info"] = got, np.array([info[k] for k in ("crossings", "largest_row", "slow_rows", "overflow")])
    assert out["slow rows info"][2] == 40 and out["large info"][2] == 0
    return out


POLYGONIZE = ("nested", "holes in a row", "long walks", "spiral 65x67", "noise of 8 labels", "noise with background",
              "extreme labels")
PG_INFO = ("edges", "vertices", "rings", "holes", "rounds")


@cached
def polygonize_inputs(seed):
    import _polygonize_cases as PK
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 6, (H, W)).astype(np.int32)
    noise[HOLE] = -1
    out = Inputs({n: PK.cases()[n] for n in POLYGONIZE})
    out["noise 130x67"] = noise
    return out


@cached
def _ref_polygonize(i):
    import _polygonize_ref as PG
    out = {}
    for n in i:
        w = PG.polygonize(PG.normalise(i[n], None))
        out[n] = tuple(w[:4]) + (np.array([w[4][k] for k in PG_INFO]),)
    w = PG.polygonize(PG.normalise(i["noise 130x67"], 2))
    out["background 2"] = tuple(w[:4])
    return out


@row("vector.polygonize", ["vector.polygonize"], polygonize_inputs, _ref_polygonize)
def _(m, i):
    out = {}
    for n in i:
        pg, info = m.vector.polygonize(i[n], return_info=True)
        out[n] = (pg.geometry.coords, pg.geometry.parts, pg.geometry.ids, pg.shell, np.array([info[k] for k in PG_INFO]))
    pg = m.vector.polygonize(i["noise 130x67"], background=2)
    out["background 2"] = (pg.geometry.coords, pg.geometry.parts, pg.geometry.ids, pg.shell)
    return out


# ---- evaluation: tests/_evaluation_ref.py, _curve_ref.py -------------------------------------------------------------
def values_same(what, got, want):
    """_evaluation_ref.same on every array: dtype, shape, equal values, NaN in the same places"""
    g, w = list(leaves(got)), list(leaves(want))
    assert len(g) == len(w), what
    for (p, a), (_, b) in zip(g, w):
        assert a.dtype == b.dtype and a.shape == b.shape, "%s%s: %s%s, expected %s%s" % (what, p, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what + p


def curve_same(what, got, want):
    """test_gpu_curve.py's same_curve: every field, shape and values, NaN in the same places"""
    g, w = list(leaves(got)), list(leaves(want))
    assert len(g) == len(w), what
    for (p, a), (_, b) in zip(g, w):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what + p


@cached
def evaluation_inputs(seed):
    """test_gpu_curve.py's raster at 130 x 67: a HAND-like raw raster of heights 0..128 (a fifth 0, nodata -100, NaN), the
    reference's scaling of it with cells planted exactly on thresholds, and a benchmark map {-100, 0, 1}"""
    import _evaluation_ref as EV
    rng = np.random.default_rng(seed)
    n = H * W
    u, w = rng.random(n), rng.random(n)
    raw = np.where(w < 0.2, 0, np.where(w < 0.25, -100, np.floor(u * 1024) / 8)).astype(np.float32)
    raw[(w >= 0.25) & (w < 0.27)] = np.nan
    raw[0:4] = (np.nan, 0, 1, 128)
    desc = EV.scale(raw, 0, 128, -100)
    plant = np.flatnonzero((rng.random(n) < 0.3) & (np.arange(n) > 3))
    desc[plant] = (rng.integers(0, 10001, plant.size) / 10000).astype(desc.dtype)
    with np.errstate(invalid="ignore"):
        flood = ((desc <= 0.37) ^ (rng.random(n) < 0.1)).astype(np.int8)
    flood[rng.random(n) < 0.05] = -100
    return Inputs(raw=raw.reshape(H, W), desc=desc.reshape(H, W), flood=flood.reshape(H, W), th=np.arange(201) / 200)


def _scalar(x):
    return np.asarray(x, np.float64).reshape(1)


@cached
def _ref_evaluation(i):
    import _curve_ref as CV
    import _evaluation_ref as EV
    out = {"scale": EV.scale(i["raw"], 0, 128, -100), "remapped": EV.remap(i["flood"])}
    for under in ("under", "over"):
        th = EV.calibrate(i["desc"], i["flood"], under)
        binary = EV.binary_map(i["desc"], th, under)
        klass, counts = EV.class_map(binary, i["flood"])
        out["calibration " + under], out["binary " + under] = _scalar(th), binary
        out["avaliacao " + under] = (np.asarray(EV.indexes(counts), np.float64), klass)
        out["curve " + under] = tuple(np.asarray(f) for f in CV.curve(i["desc"], i["flood"], under, 200))
        out["counts " + under] = out["curve " + under][1]
        out["exhaustive " + under] = _scalar(CV.exhaustive(i["desc"], i["flood"], under, 10000, "fit"))
        out["exhaustive tss " + under] = _scalar(CV.exhaustive(i["desc"], i["flood"], under, 37, "tss"))
    return out


@row("evaluation", ["evaluation.minMaxScale", "evaluation.binary_map", "evaluation.avaliacao", "evaluation.calibration",
                    "evaluation.threshold_counts", "evaluation.curve", "evaluation.calibration_exhaustive"],
     evaluation_inputs, _ref_evaluation,
     dict({"scale": values_same, "remapped": values_same},
          **{"%s %s" % (k, u): (curve_same if k in ("curve", "counts") else values_same) for u in ("under", "over")
             for k in ("calibration", "binary", "avaliacao", "curve", "counts", "exhaustive", "exhaustive tss")}))
def _(m, i):
    ev = m.evaluation
    out = {"scale": ev.minMaxScale(i["raw"].copy(), 0, 128, -100)}
    for under in ("under", "over"):
        flood = i["flood"].copy()
        th = ev.calibration(i["desc"].copy(), flood, under)
        out["remapped"] = flood
        binary = ev.binary_map(i["desc"].copy(), th, under)
        c, f, cm = ev.avaliacao(binary.copy(), i["flood"].copy())
        out["calibration " + under], out["binary " + under] = _scalar(th), binary
        out["avaliacao " + under] = (np.asarray((c, f), np.float64), cm)
        out["curve " + under] = tuple(np.asarray(x) for x in ev.curve(i["desc"], i["flood"], under, steps=200))
        out["counts " + under] = ev.threshold_counts(i["desc"], i["flood"], i["th"], under)
        out["exhaustive " + under] = _scalar(ev.calibration_exhaustive(i["desc"], i["flood"], under))
        out["exhaustive tss " + under] = _scalar(ev.calibration_exhaustive(i["desc"], i["flood"], under, steps=37, objective="tss"))
    return out



RESIDENT = (("real", "under"), ("real", "over"), ("int", "under"))
RESIDENT_TH = np.arange(201) / 200


@cached
def resident_inputs(seed):
    """test_gpu_evaluation.py's hand_and_flood at 130 x 67 cells, flat: a HAND-like raster (a fifth 0, nodata -100, NaN,
    fractions in the 'real' kind, integers in the 'int' kind), a valid first cell, a benchmark map {-100, 0, 1}"""
    rng = np.random.default_rng(seed)
    n = H * W
    u, w = rng.random(n), rng.random(n)
    out = Inputs()
    for kind in ("real", "int"):
        raw = np.floor(u * 1024) / 8 if kind == "real" else np.floor(u * 129)
        raw = np.where(w < 0.2, 0, np.where(w < 0.25, -100, raw)).astype(np.float32)
        if kind == "real":
            raw[(w >= 0.25) & (w < 0.27)] = np.nan
            raw = np.where((raw > 0) & (np.arange(n) > 3), raw + np.float32(0.3), raw).astype(np.float32)
        raw[0:4] = (0, 0, 1, 128)
        out[kind] = raw
    with np.errstate(invalid="ignore"):
        wet = (out["real"] >= 0) & (out["real"] <= 40)
    flood = (wet ^ (rng.random(n) < 0.1)).astype(np.int8)
    flood[rng.random(n) < 0.05] = -100
    out["flood"] = flood
    return out


@cached
def _ref_resident(i):
    """test_gpu_evaluation.py's reference_pipeline, and test_gpu_curve.py's reference of the resident curve on the
    scaled raster as the device holds it (float64)"""
    import _curve_ref as CV
    import _evaluation_ref as EV
    out = {}
    for kind, under in RESIDENT:
        raw = i[kind].astype(np.int16) if kind == "int" else i[kind]
        with np.errstate(invalid="ignore"):
            e = EV.extremes(raw)
        mn, mx = e[1], e[2]
        desc = EV.scale(raw, mn, mx, -100)
        th = EV.calibrate(desc, i["flood"], under)
        binary = EV.binary_map(desc, th, under)
        klass, counts = EV.class_map(binary, i["flood"])
        assert counts.min() > 0 and desc[0] == 0
        c, f = EV.indexes(counts)
        d64 = desc.astype(np.float64)
        curve = CV.curve_of(RESIDENT_TH, CV.hist(d64, i["flood"], RESIDENT_TH, under, nodata=float(d64[0])), under)
        out["%s %s" % (kind, under)] = {
            "scalars": np.array([float(mn), float(mx), th, c, f]), "counts": np.asarray(counts, np.int64), "desc": d64,
            "binary": binary.astype(np.uint8), "klass": klass.astype(np.int32), "flood": EV.remap(i["flood"]),
            "curve": tuple(np.asarray(x) for x in curve)}
    return out


def _resident_same(what, got, want):
    """equal values, NaN in the same places (the tests' np.array_equal / same_curve), shapes included"""
    g, w = list(leaves(got)), list(leaves(want))
    assert [p for p, _ in g] == [p for p, _ in w], what
    for (p, a), (_, b) in zip(g, w):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what + p


@row("evaluation.resident", ["evaluation.evaluate_resident", "evaluation.curve_resident"], resident_inputs, _ref_resident,
     _resident_same)
def _(m, i):
    """the device tier: a context of its own, every buffer a dt_dev_malloc block made while the key is set"""
    from descriptools_amd import device
    n = H * W
    out = {}
    for kind, under in RESIDENT:
        ctx = device.Context()
        bufs = [ctx.to_device(i[kind]), ctx.to_device(i["flood"]), ctx.empty(n, np.float64), ctx.empty(n, np.uint8),
                ctx.empty(n, np.int32)]
        d_x, d_f, d_d, d_b, d_k = bufs
        try:
            plain = m.evaluation.evaluate_resident(ctx, d_x.ptr, d_f.ptr, n, under, integer_valued=kind == "int")
            res = m.evaluation.evaluate_resident(ctx, d_x.ptr, d_f.ptr, n, under, desc_ptr=d_d.ptr, integer_valued=kind == "int",
                                                 binary_ptr=d_b.ptr, class_ptr=d_k.ptr, remap_flood=True)
            assert plain["threshold"] == res["threshold"] and np.array_equal(plain["counts"], res["counts"])
            desc = d_d.to_host()
            flood = d_f.to_host()
            d_f.copy_from(i["flood"])
            curve = m.evaluation.curve_resident(ctx, d_d.ptr, d_f.ptr, n, RESIDENT_TH, under, float(desc[0]))
            out["%s %s" % (kind, under)] = {
                "scalars": np.array([res["mn"], res["mx"], res["threshold"], res["correctness"], res["fit"]]),
                "counts": np.asarray(res["counts"], np.int64), "desc": desc, "binary": d_b.to_host(), "klass": d_k.to_host(),
                "flood": flood, "curve": tuple(np.asarray(x) for x in curve)}
        finally:
            for b in bufs:
                b.free()
            ctx.close()
    return out


SEED = 5

# ---- public functions without a row ----------------------------------------------------------------------------------
EXEMPT = {
    "cost.cost_hand": "calls only cost.cost_distance and flowhand.hand_calculator",
    "dinf.specific_catchment_area": "calls only dinf.accumulate; the rest is numpy",
    "downslope.downslope_sequential_jit": "calls only downslope.downsloper's launch; the repair is numpy",
    "evaluation.correctness": "pure host helper",
    "evaluation.fit": "pure host helper",
    "evaluation.combine_extremes": "pure host helper",
    "filters.minimum": "calls only filters.extremes",
    "filters.maximum": "calls only filters.extremes",
    "filters.relief": "calls only filters.extremes",
    "filters.rank_table": "pure host helper",
    "filters.median": "calls only filters.percentile",
    "flowacc.weight_frac_bits": "pure host helper",
    "flowhand.index_calculator": "pure host helper",
    "flowhand.flow_distance_indexes_sequential": "calls only flowhand.flow_distance_index_cpu",
    "flowhand.fdist_indexes_sequential_jit": "calls only flowhand.flow_distance_index_cpu",
    "flowpath.path_frac_bits": "pure host helper",
    "flowpath.step_length": "pure host helper (numpy)",
    "flowpath.travel_time": "calls only flowpath.downstream_sum",
    "flowpath.time_of_concentration": "calls only flowpath.upslope_longest",
    "focal.qmax": "pure host helper",
    "focal.default_frac_bits": "pure host helper",
    "focal.mean": "calls only focal.statistics",
    "focal.std": "calls only focal.statistics",
    "focal.tpi": "calls only focal.statistics",
    "focal.dev": "calls only focal.statistics",
    "gfi.geomorphic_flood_index_cpu": "calls only the launch of gfi.ln_hl_H_calculator (dt_gfi_area), without the guard",
    "gfi.ln_hl_H_cpu": "calls only the launch of gfi.ln_hl_H_calculator",
    "gfi.geomorphic_flood_index_sequential_jit": "calls only gfi.geomorphic_flood_index_cpu",
    "gfi.ln_hl_H_sequential_jit": "calls only gfi.ln_hl_H_cpu",
    "harmonic.select_voids": "pure host helper (numpy)",
    "harmonic.fill_voids": "calls only regions.label and the dt_harmonic launch of harmonic.interpolate",
    "harmonic.base_level": "calls only the dt_harmonic launch of harmonic.interpolate",
    "harmonic.vdcn": "calls only harmonic.base_level's launch",
    "horizon.flat_tangent": "pure host helper",
    "horizon.geomorphons": "calls only horizon.attributes",
    "horizon.openness": "calls only horizon.attributes",
    "horizon.sky_view": "calls only horizon.attributes",
    "mfd.specific_catchment_area": "calls only mfd.accumulate; the rest is numpy",
    "mrvbf.slope_threshold": "pure host helper",
    "mrvbf.default_levels": "pure host helper",
    "mrvbf.mrvbf": "calls only mrvbf.indices",
    "mrvbf.mrrtf": "calls only mrvbf.indices",
    "proximity.euclidean_hand": "calls only proximity.nearest_river and flowhand.hand_calculator",
    "reaches.bed_weight_max": "pure host helper",
    "reaches.tables_from_sums": "pure host helper: the float64 tables from the integer sums of reaches.hydraulic_tables",
    "reaches.rating_curves": "pure host helper",
    "reaches.stage_for_discharge": "pure host helper",
    "resample.compose": "pure host helper",
    "resample.align": "calls only resample.warp",
    "resample.resize": "calls only resample.warp (the row calls it)",
    "resample.aggregate": "calls only resample.warp (the row calls it)",
    "routing.decayed_accumulation": "calls only routing.route",
    "routing.retention_limited": "calls only routing.route",
    "routing.transport_limited": "calls only routing.route",
    "routing.sink_capacity": "calls only watershed.drainage; the rest is numpy",
    "slope.slope_cpu": "calls only slope.sloper's launch on a padded tile",
    "slope.slope_sequential_jit": "calls only slope.sloper's launch",
    "streams.shreve": "calls only streams.stream_network",
    "terrain.sun_vector": "pure host helper",
    "terrain.gradient": "calls only terrain.attributes",
    "terrain.aspect": "calls only terrain.attributes",
    "terrain.curvature": "calls only terrain.attributes",
    "terrain.hillshade": "calls only terrain.attributes",
    "topoindexes.topographic_index": "calls only topoindexes.topographic_index_cpu",
    "topoindexes.topographic_index_sequential_jit": "calls only topoindexes.topographic_index_cpu",
    "topoindexes.modified_topographic_index_sequential_jit": "calls only topoindexes.topographic_index_cpu",
    "vector.to_pixel": "pure host helper",
    "vector.from_pixel": "pure host helper",
    "vector.from_geojson": "pure host helper",
    "vector.to_geojson": "pure host helper",
    "vector.count_crossings": "host arithmetic in the library: no device, no workspace",
    "vector.mask": "calls only vector.rasterize",
    "vector.burn": "calls only vector.rasterize and zonal.paint",
    "zonal.statistics_from_tables": "pure host helper",
    "zonal.quantiles": "pure host helper",
}
