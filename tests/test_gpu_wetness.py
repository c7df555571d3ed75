"""GPU (-m gpu): wetness.suction / modified_catchment_area / saga_wetness_index (dt_wetness_*, dt_dev_wetness_*, k_wet_*
in dt_wetness.hip) against tests/_wetness_ref.py: the modified area as int64 bit patterns against the max-heap Dijkstra,
dtype and shape included.  Trivial shapes; ragged tiles (65 x 63: 2 x 1 tiles of 64 x 64; 130 x 257: 3 x 5 tiles, every
colour and an interior tile) with uniform, plateau (exact ties, long fronts) and steep (many s = 0) suction, nodata of
every kind in both rasters, and a visit limit of 1 that forces a global round per sweep; the lone s = 0 cell among
nodata (0 * -inf); a certificate on the GPU result alone; a serpentine whose path winds through 135 tiles, which shows
that the multi-round path ran; the suction and the index against numpy to one float32 spacing; the device tier and its
budget; the C entry with NULL outputs between guard bands."""
import functools
import math

import numpy as np
import pytest

import _wetness_ref as R

pytestmark = pytest.mark.gpu

TILE = 64  # WT_T of csrc/dt_wetness.hip
SEED = 7


def _same(name, g, r):
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    gb = g.view(np.int64) if g.dtype == np.float64 else g
    rb = r.view(np.int64) if r.dtype == np.float64 else r
    if not np.array_equal(gb, rb):
        bad = np.argwhere(gb != rb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r" % (name, len(bad), i, g[i], r[i]))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _random_ref(shape, kind):
    """(area, suction, reference M, Jacobi sweeps, raised cells) of a random case: computed once, shared, never written
    to"""
    a, s = R.random_case(shape, kind, SEED)
    M = R.reference(a, s)
    sweeps = R.jacobi(a, s)[1]
    _frozen(a, s, M)
    return a, s, M, sweeps, R.raised(a, s, M)


@functools.lru_cache(maxsize=None)
def _serpentine_ref(sv):
    a, s = R.serpentine(s=np.float32(sv))
    M = R.reference(a, s)
    _frozen(a, s, M)
    return a, s, M


def check(a, s, limit=0, ref=None):
    from descriptools_amd import wetness
    got = wetness.modified_catchment_area(a, s, _visit_limit=limit)
    M = ref if ref is not None else R.reference(a, s)
    _same("modified", got, M)
    assert got.info["raised"] == R.raised(a, s, M)
    return got


# ---- trivial shapes -------------------------------------------------------------------------------------------------
def test_one_cell():
    got = check(np.full((1, 1), 3.5), np.full((1, 1), 0.5, np.float32))
    assert got[0, 0] == 3.5 and got.info == {"rounds": 0, "raised": 0, "tile_visits": 1}
    for a, s in ((-100.0, 0.5), (3.5, np.nan), (0.0, 0.5), (np.inf, 1.0), (3.5, 1.5)):
        got = check(np.full((1, 1), a), np.full((1, 1), s, np.float32))
        assert got[0, 0] == -100 and got.info["raised"] == 0


@pytest.mark.parametrize("shape", [(1, 200), (200, 1)], ids=lambda s: "%dx%d" % s)
def test_one_row_and_one_column(shape):
    a = np.ones(shape, np.float64)
    a.reshape(-1)[[20, 170]] = 5000.0, 80.0
    a.reshape(-1)[150] = np.nan  # cuts the line: nothing passes
    s = np.full(shape, 0.95, np.float32)
    got = check(a, s).reshape(-1)
    assert got[150] == -100 and got[149] > 1 and got[151] > 1
    # beyond the cut only the second peak is felt
    alone = R.reference(a.reshape(-1)[151:].reshape(1, -1), s.reshape(-1)[151:].reshape(1, -1))
    assert np.array_equal(got[151:], alone.reshape(-1))
    assert got[21] == float(np.float32(0.95)) * 5000.0


def test_all_nodata():
    shape = (70, 66)
    bad = np.array([0, -1, -100, np.nan, np.inf])[np.arange(70 * 66) % 5].reshape(shape)
    got = check(bad, np.full(shape, 0.9, np.float32))
    assert (got == -100).all() and got.info["raised"] == 0 and got.info["rounds"] == 0
    got = check(np.ones(shape), np.full(shape, -100, np.float32))
    assert (got == -100).all()


def test_empty_rasters():
    from descriptools_amd import wetness
    for shape in ((0, 5), (5, 0), (0, 0)):
        a, s = np.ones(shape), np.ones(shape, np.float32)
        got = wetness.modified_catchment_area(a, s)
        assert got.shape == shape and got.dtype == np.float64 and got.info["rounds"] == 0
        assert wetness.suction(s).shape == shape and wetness.suction(s).dtype == np.float32
        swi, M = wetness.saga_wetness_index(a, s, modified=True)
        assert swi.shape == shape and swi.dtype == np.float32 and M.shape == shape


# ---- ragged tiles, random cases -------------------------------------------------------------------------------------
CASES = [((65, 63), 0), ((65, 63), 1), ((130, 257), 0)]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape,limit", CASES, ids=["65x63", "65x63-limit1", "130x257"])
def test_random_cases(shape, limit, kind):
    a, s, M, sweeps, raised = _random_ref(shape, kind)
    ok = R.valid(a, s)
    assert ok.mean() >= 0.85 and raised >= 0.5 * ok.sum(), "the case tests too little: change the seed"
    got = check(a, s, limit=limit, ref=M)
    print("%s %s limit %d: jacobi sweeps %d, rounds %d, tile visits %d" % (shape, kind, limit, sweeps,
                                                                           got.info["rounds"], got.info["tile_visits"]))
    if limit == 1:
        # a stage (one colour's launch, one sweep per visit) moves information at most one cell, a round has four stages
        assert got.info["rounds"] >= (sweeps - 1) / 4
    assert got.info["tile_visits"] >= got.info["rounds"]
    assert got.info["raised"] == raised


def test_lone_zero_suction_cell_among_nodata_keeps_its_area():
    """0 * -inf = NaN must never win: the update is `cand > old`"""
    a = np.full((70, 70), -100.0)
    a[1, 1] = a[64, 64] = a[69, 0] = 5.0
    s = np.zeros(a.shape, np.float32)
    got = check(a, s)
    assert got[1, 1] == 5.0 and got[64, 64] == 5.0 and got[69, 0] == 5.0 and (got == -100).sum() == a.size - 3
    assert not np.isnan(got).any()


def test_certificate_on_the_gpu_result_alone():
    """M is a fixed point between A and max A, and every raised cell is held up by a neighbour: independent of the
    reference"""
    from descriptools_amd import wetness
    for kind in R.KINDS:
        a, s, _, _, _ = _random_ref((130, 257), kind)
        M = np.asarray(wetness.modified_catchment_area(a, s))
        ok = R.valid(a, s)
        H, W = a.shape
        assert (M[~ok] == -100).all()
        assert (M[ok] >= a[ok]).all() and (M[ok] <= a[ok].max()).all()
        P = np.full((H + 2, W + 2), -np.inf)
        P[1:-1, 1:-1] = np.where(ok, M, -np.inf)
        s64 = np.where(ok, s, 0).astype(np.float64)
        tight = np.zeros((H, W), bool)
        for dy, dx in R.MOVES:
            nb = P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            has = ok & (nb > -np.inf)
            cand = s64 * np.where(has, nb, 0.0)
            assert (M[has] >= cand[has]).all(), (kind, dy, dx)
            tight |= has & (M == cand)
        up = ok & (M > np.where(ok, a, np.inf))
        assert up.sum() > 0.5 * ok.sum() and tight[up].all(), kind


# ---- serpentine: many rounds ----------------------------------------------------------------------------------------
def test_serpentine_with_suction_one_floods_everything():
    a, s, M = _serpentine_ref(1.0)
    ok = R.valid(a, s)
    got = check(a, s, ref=M)
    assert int(ok.sum()) == 25154 and (np.asarray(got)[ok] == 1e6).all()


def test_serpentine_runs_many_rounds():
    a, s, M = _serpentine_ref(0.999)
    ok = R.valid(a, s)
    got = check(a, s, ref=M)
    g = np.asarray(got)
    assert len(np.unique(g[ok])) == 8386 and abs(g[ok].min() - 227.33468672097197) < 1e-9
    assert got.info["raised"] == 25154 - 1
    entries = R.serpentine_tile_entries(a.shape, TILE)
    print("serpentine: tile entries %d, rounds %d, tile visits %d" % (entries, got.info["rounds"],
                                                                      got.info["tile_visits"]))
    # the bars stand on the tile columns' last cells, so every path from (0, 0) to the last column enters that many
    # tiles; a round visits each tile once, so a front crosses at most four tiles (one per colour) per round
    assert entries == 135
    assert got.info["rounds"] >= entries / 4


# ---- order, run and scale -------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_run_or_scale():
    """the same call twice gives the same bytes; areas scaled by a power of two give M scaled exactly"""
    from descriptools_amd import wetness
    a, s, M, _, _ = _random_ref((65, 63), "uniform")
    x = wetness.modified_catchment_area(a, s)
    y = wetness.modified_catchment_area(a, s)
    assert x.tobytes() == y.tobytes()
    with np.errstate(invalid="ignore"):
        big = wetness.modified_catchment_area(a * 2.0 ** 20, s)
    ok = R.valid(a, s)
    assert np.array_equal(np.where(ok, np.asarray(x) * 2.0 ** 20, -100.0), np.asarray(big))


# ---- suction and index ----------------------------------------------------------------------------------------------
def _spacing_ok(name, g, r):
    """-100 on exactly the reference's cells; elsewhere at most one float32 spacing apart; prints the count"""
    assert g.dtype == np.float32 and r.dtype == np.float32 and g.shape == r.shape
    assert np.array_equal(g == -100, r == -100), name
    assert not np.isnan(g).any(), name
    tol = np.spacing(np.maximum(np.abs(g), np.abs(r)))
    diff = np.abs(g.astype(np.float64) - r.astype(np.float64))
    print("%s: %d of %d cells differ from numpy" % (name, int((diff > 0).sum()), g.size))
    assert (diff <= tol).all(), "%s: %d cells beyond one float32 spacing" % (name, int((diff > tol).sum()))


def _slopes(shape=(65, 63)):
    rng = np.random.default_rng(11)
    sl = (rng.random(shape) ** 3 * 1.2).astype(np.float32)
    sl.reshape(-1)[:7] = [0.0, 1e-4, 0.1, 1.0, 1.5, math.pi / 2, -100.0]
    bad = rng.random(shape) < 0.03
    bad.reshape(-1)[:7] = False
    sl[bad] = rng.choice(np.array([np.nan, -100.0, 1.6, -1e-6, np.inf], np.float32), int(bad.sum()))
    return sl


@pytest.mark.parametrize("t,weight,offset,minimum", [(10.0, 1.0, R.SLOPE_OFFSET, 0.0), (15.0, 1.0, R.SLOPE_OFFSET, 0.0),
                                                     (10.0, 2.5, 0.0, 0.02), (15.0, 0.3, 0.0, 0.0)])
def test_suction_against_numpy(t, weight, offset, minimum):
    from descriptools_amd import wetness
    sl = _slopes()
    g = wetness.suction(sl, t, weight, offset, minimum)
    r = R.suction(sl, t, weight, offset, minimum)
    _spacing_ok("suction t=%g weight=%g" % (t, weight), g, r)
    ok = g != -100
    assert (g[ok] >= 0).all() and (g[ok] <= 1).all()
    assert list(g.reshape(-1)[5:7]) == [-100, -100]
    if weight >= 1:
        assert g.reshape(-1)[4] == 0  # slope 1.5: t^e > 30, so s < t^(-1.5 exp(30)) underflows
    if offset == 0 and minimum == 0:
        assert g.reshape(-1)[0] == 1.0


@pytest.mark.parametrize("kind", ["uniform", "plateau"])
def test_saga_wetness_index(kind):
    from descriptools_amd import wetness
    a = _random_ref((65, 63), kind)[0]
    sl = _slopes(a.shape)
    s_gpu = wetness.suction(sl)
    swi, M = wetness.saga_wetness_index(a, sl, modified=True)
    # M is the reference run on the GPU's own suction plane
    ref = R.reference(a, s_gpu)
    _same("modified", M, ref)
    assert M.info["raised"] == R.raised(a, s_gpu, ref) and M.info["raised"] > 0.3 * a.size
    _spacing_ok("swi " + kind, swi, R.swi(ref, sl))
    assert ((swi == -100) == (np.asarray(M) == -100)).all()  # here no b reaches pi/2: nodata alone
    plain = wetness.saga_wetness_index(a, sl)
    assert plain.dtype == np.float32 and plain.tobytes() == swi.tobytes()
    _same("modified_catchment_area on the same plane", wetness.modified_catchment_area(a, s_gpu), ref)
    # other parameters reach the kernels; b >= pi/2 under a large offset is -100 though the cell is valid
    swi2, M2 = wetness.saga_wetness_index(a, sl, t=15.0, slope_weight=0.5, slope_offset=0.4, slope_min=0.45,
                                          modified=True)
    s2 = wetness.suction(sl, 15.0, 0.5, 0.4, 0.45)
    ref2 = R.reference(a, s2)
    _same("modified, other parameters", M2, ref2)
    want2 = R.swi(ref2, sl, 0.4, 0.45)
    assert ((want2 == -100) & (ref2 != -100)).any()
    _spacing_ok("swi, other parameters", swi2, want2)


# ---- the device tier ------------------------------------------------------------------------------------------------
def _dev_area(ctx, a, s, limit, rounds):
    """dt_dev_wetness_modified_area on resident rasters -> (modified, status bits)"""
    from descriptools_amd import _lib
    H, W = a.shape
    d_a, d_s = ctx.to_device(np.ascontiguousarray(a, np.float64)), ctx.to_device(np.ascontiguousarray(s, np.float32))
    d_m = ctx.empty((H, W), np.float64)
    try:
        _lib.check(_lib.lib().dt_dev_wetness_modified_area(ctx.h, d_a.ptr, d_s.ptr, H, W, limit, rounds, d_m.ptr))
        st = ctx.status()
        return d_m.to_host(), st
    finally:
        for d in (d_a, d_s, d_m):
            d.free()


def test_device_tier_equals_the_host_tier():
    from descriptools_amd import _lib, wetness
    from descriptools_amd.device import Context
    a = _random_ref((130, 257), "plateau")[0]
    sl = _slopes(a.shape)
    swi, M = wetness.saga_wetness_index(a, sl, modified=True)
    s_host = wetness.suction(sl)
    H, W = a.shape
    L = _lib.lib()
    ctx = Context()
    try:
        d_a, d_sl = ctx.to_device(np.ascontiguousarray(a)), ctx.to_device(sl)
        d_s, d_m, d_w = ctx.empty((H, W), np.float32), ctx.empty((H, W), np.float64), ctx.empty((H, W), np.float32)
        _lib.check(L.dt_dev_wetness_suction(ctx.h, d_sl.ptr, H, W, 10.0, 1.0, R.SLOPE_OFFSET, 0.0, d_s.ptr))
        _lib.check(L.dt_dev_wetness_modified_area(ctx.h, d_a.ptr, d_s.ptr, H, W, 0, 256, d_m.ptr))
        _lib.check(L.dt_dev_wetness_index(ctx.h, d_m.ptr, d_sl.ptr, H, W, R.SLOPE_OFFSET, 0.0, d_w.ptr))
        assert ctx.status() == 0
        assert d_s.to_host().tobytes() == s_host.tobytes()
        _same("modified", d_m.to_host(), np.asarray(M))
        assert d_w.to_host().tobytes() == swi.tobytes()
        for d in (d_a, d_sl, d_s, d_m, d_w):
            d.free()
        for kind in R.KINDS:
            a, s, ref, _, _ = _random_ref((130, 257), kind)
            m, st = _dev_area(ctx, a, s, 0, 256)
            assert st == 0
            _same("modified " + kind, m, ref)
    finally:
        ctx.close()


def test_device_tier_budget_and_refusals():
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    a, s, ref = _serpentine_ref(0.999)
    L = _lib.lib()
    ctx = Context()
    try:
        m, st = _dev_area(ctx, a, s, 0, 1)
        assert st == 2, "DT_STATUS_NOT_CONVERGED"
        m, st = _dev_area(ctx, a, s, 0, 4096)
        assert st == 0
        _same("modified", m, ref)
        for rounds in (0, -1, 4097):
            assert L.dt_dev_wetness_modified_area(ctx.h, None, None, 4, 4, 0, rounds, None) == -1
            assert b"rounds" in L.dt_last_error()
        assert L.dt_dev_wetness_modified_area(ctx.h, None, None, 0, 7, 0, 1, None) == 0
        assert L.dt_dev_wetness_modified_area(ctx.h, None, None, 4, 4, 0, 1, None) == -1
        assert L.dt_last_error() == b"invalid argument: NULL raster"
        assert L.dt_dev_wetness_modified_area(ctx.h, None, None, 1 << 16, 1 << 15, 0, 1, None) == -1
        assert b"2^31" in L.dt_last_error()
        for bad, word in (((1.0, 1.0, 0.1, 0.0), b"t must"), ((math.nan, 1.0, 0.1, 0.0), b"t must"),
                          ((10.0, 0.0, 0.1, 0.0), b"slope_weight"), ((10.0, math.inf, 0.1, 0.0), b"slope_weight"),
                          ((10.0, 1.0, -0.1, 0.0), b"slope_offset"), ((10.0, 1.0, 0.1, math.nan), b"slope_min")):
            assert L.dt_dev_wetness_suction(ctx.h, None, 0, 0, *bad, None) == -1
            assert word in L.dt_last_error(), bad
        assert L.dt_dev_wetness_suction(ctx.h, None, 0, 0, 10.0, 1.0, 0.0, 0.0, None) == 0
        assert L.dt_dev_wetness_index(ctx.h, None, None, 0, 0, 0.0, 0.0, None) == -1
        assert b"both be 0" in L.dt_last_error()
        assert L.dt_dev_wetness_index(ctx.h, None, None, 0, 0, 0.0, 0.1, None) == 0
        assert ctx.status() == 0
    finally:
        ctx.close()


# ---- the host-tier C entry itself -----------------------------------------------------------------------------------
def test_c_entry_with_null_outputs_between_guard_bands():
    from descriptools_amd import _lib, wetness
    a = np.ascontiguousarray(_random_ref((65, 63), "uniform")[0])
    sl = _slopes(a.shape)
    H, W = a.shape
    GUARD = 4096
    swi, M = wetness.saga_wetness_index(a, sl, modified=True)
    s_gpu = wetness.suction(sl)

    def guarded(dtype):
        raw = np.full(2 * GUARD + H * W * np.dtype(dtype).itemsize, 0xA5, np.uint8)
        return raw, raw[GUARD:raw.size - GUARD].view(dtype).reshape(H, W)

    L = _lib.lib()
    p = lambda x, t: _lib.ptr(x, t)
    par = (10.0, 1.0, R.SLOPE_OFFSET, 0.0)
    # the index alone: the suction and the modified area stay on the device
    raw_w, w = guarded(np.float32)
    info = np.full(4, -1, np.int64)
    _lib.check(L.dt_wetness_saga(p(a, _lib.c_f64p), p(sl, _lib.c_f32p), H, W, *par, 0, p(w, _lib.c_f32p), None, None,
                                 p(info, _lib.c_i64p)))
    assert w.tobytes() == swi.tobytes()
    assert info[0] >= 1 and info[1] == M.info["raised"] and info[2] >= 2 and info[3] == 0
    assert (raw_w[:GUARD] == 0xA5).all() and (raw_w[-GUARD:] == 0xA5).all()
    # every output, each between its guard bands; info4 may be NULL; one optional output at a time
    for want_m, want_s in ((True, True), (True, False), (False, True)):
        raw_w, w = guarded(np.float32)
        raw_m, m = guarded(np.float64)
        raw_s, s = guarded(np.float32)
        _lib.check(L.dt_wetness_saga(p(a, _lib.c_f64p), p(sl, _lib.c_f32p), H, W, *par, 0, p(w, _lib.c_f32p),
                                     p(m, _lib.c_f64p) if want_m else None, p(s, _lib.c_f32p) if want_s else None,
                                     None))
        assert w.tobytes() == swi.tobytes()
        if want_m:
            _same("modified", m, np.asarray(M))
        if want_s:
            assert s.tobytes() == s_gpu.tobytes()
        for raw, used in ((raw_w, True), (raw_m, want_m), (raw_s, want_s)):
            assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
            assert used or (raw == 0xA5).all()
    # dt_wetness_modified_area with and without info4
    raw_m, m = guarded(np.float64)
    _lib.check(L.dt_wetness_modified_area(p(a, _lib.c_f64p), p(s_gpu, _lib.c_f32p), H, W, 0, p(m, _lib.c_f64p), None))
    _same("modified", m, np.asarray(M))
    assert (raw_m[:GUARD] == 0xA5).all() and (raw_m[-GUARD:] == 0xA5).all()
    # refusals of the entries themselves
    for bad in ((1.0, 1.0, 0.1, 0.0), (10.0, -1.0, 0.1, 0.0), (10.0, 1.0, math.inf, 0.0), (10.0, 1.0, 0.0, 0.0)):
        assert L.dt_wetness_saga(p(a, _lib.c_f64p), p(sl, _lib.c_f32p), H, W, *bad, 0, p(w, _lib.c_f32p), None, None,
                                 None) == -1
    assert L.dt_wetness_saga(p(a, _lib.c_f64p), p(sl, _lib.c_f32p), H, W, *par, -1, p(w, _lib.c_f32p), None, None,
                             None) == -1
    assert L.dt_wetness_saga(p(a, _lib.c_f64p), None, H, W, *par, 0, p(w, _lib.c_f32p), None, None, None) == -1
    assert L.dt_wetness_saga(None, None, 0, 9, *par, 0, None, None, None, p(info, _lib.c_i64p)) == 0
    assert list(info) == [0, 0, 0, 0]
    assert L.dt_wetness_suction(None, 1 << 16, 1 << 15, *par, None) == -1
    assert b"2^31" in L.dt_last_error()
