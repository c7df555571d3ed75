"""Does any op depend on what its working memory held before?  Every row of tests/_poison_cases.py runs with debug key
12 (DT_DBG_POISON) off and then with the context scratch, the host tier's device blocks (scratch, inputs before their
upload, outputs), the side buffers and dt_dev_malloc's blocks filled with 0xFF, 0x80, 0x01 and 0xA5 before the op
starts.  Each run is held against the row's reference at the bar of the op's own GPU test, and each poisoned run against
the bytes of the clean one, dtype and shape included.

0xFF raises every flag, makes every count -1, every path-tile word PT_NONE / PT_FAILP / "resolved" and every float a NaN;
0x80 sets bit 31 (PT_RES) and the sign bits; 0x01 raises flags and leaves small counts; 0xA5 is the suite's own pattern.

The device tier (memory through dt_dev_malloc and the context scratch): one step of chain.Chain on float32 and on float64
heights and one tiling.RankTile step on Layout([128], [128]), against the bars of tests/test_gpu_parity.py and
tests/test_gpu_chain_f64.py; the resident evaluation (evaluate_resident, curve_resident) is a row of the table, on a
context and buffers of its own.

Not marked gpu: the completeness test -- every public function of the op modules is a row's or is in EXEMPT with its
reason -- and every row's builder and reference, which run without the library."""
import inspect

import numpy as np
import pytest

import _poison_cases as K

KEY = 12  # DT_DBG_POISON
BYTES = (0xFF, 0x80, 0x01, 0xA5)


# ---- without a GPU --------------------------------------------------------------------------------------------------
def _public(module):
    import importlib
    mod = importlib.import_module("descriptools_amd." + module)
    # a second name of a public function (slope_sequential = slope_sequential_jit) is that function
    return sorted("%s.%s" % (module, n) for n, f in vars(mod).items()
                  if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("_")
                  and (f.__name__ == n or f.__name__.startswith("_")))


def test_every_public_function_has_a_row_or_a_reason():
    covered = {c for r in K.ROWS for c in r.covers}
    public = {f for m in K.MODULES for f in _public(m)}
    assert not covered - public, "rows for functions that do not exist: %s" % sorted(covered - public)
    assert not set(K.EXEMPT) - public, "reasons for functions that do not exist: %s" % sorted(set(K.EXEMPT) - public)
    assert not covered & set(K.EXEMPT), "both a row and a reason: %s" % sorted(covered & set(K.EXEMPT))
    missing = sorted(public - covered - set(K.EXEMPT))
    assert not missing, "public functions with neither a row in tests/_poison_cases.py nor a reason in EXEMPT: %s" % missing
    for name, reason in K.EXEMPT.items():
        assert isinstance(reason, str) and reason.strip(), name
    names = [r.name for r in K.ROWS]
    assert len(set(names)) == len(names)
    for r in K.ROWS:
        assert r.unordered is None or ".hip:" in r.unordered or ".h:" in r.unordered, \
            "%s: an exemption from byte-identity cites the file and line that makes the op depend on the order" % r.name


@pytest.mark.parametrize("r", K.ROWS, ids=repr)
def test_builder_and_reference_run_without_the_library(r):
    inputs = r.build(K.SEED)
    want = r.ref(inputs)
    assert isinstance(want, dict) and want, "the reference names at least one output"
    assert list(K.leaves(want)), "the reference holds at least one array"
    assert r.build(K.SEED) is inputs and r.ref(inputs) is want, "computed once, shared"
    for _, a in K.leaves(want):
        assert not a.flags.writeable


# ---- on the GPU -----------------------------------------------------------------------------------------------------
@pytest.fixture
def poison():
    """poison(b) sets the key to 0x100 | b, poison(None) to 0; back to 0 whatever the test does"""
    from descriptools_amd import _lib
    L = _lib.lib()

    def set_(b):
        assert L.dt_debug_set(KEY, 0 if b is None else 0x100 | b) == 0
    try:
        yield set_
    finally:
        L.dt_debug_set(KEY, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("r", K.ROWS, ids=repr)
def test_row(r, poison):
    inputs = r.build(K.SEED)
    want = r.ref(inputs)
    poison(None)
    clean = r.call(K.M, inputs)
    K.meets(r, clean, want, inputs)
    for b in BYTES:
        poison(b)
        got = r.call(K.M, inputs)
        poison(None)
        K.meets(r, got, want, inputs)
        if r.unordered is None:
            K.same_bytes("%s, scratch filled with 0x%02X" % (r.name, b), got, clean)


# ---- the device tier: memory through dt_dev_malloc, the side buffers and the context scratch ---------------------------
THR = 40
SAME = ("fdr", "slope", "fac", "river", "idx", "down")


def _chain_reference(dem):
    """the chain on a float32-exact DEM by the oracle, as tests/test_gpu_parity.py takes it"""
    import oracle
    sl, fdr = oracle.slope_d8(dem, K.PX)
    fac = oracle.flowacc(fdr, dem)
    river = (fac > THR).astype(np.int8)
    fdist, idx, hand = oracle.flowhand(dem, fdr, river, K.PX)
    ref = {"slope": sl, "fdr": fdr, "fac": fac, "river": river, "fdist": fdist, "idx": idx, "hand": hand,
           "down": oracle.downslope(dem, fdr, K.PX, 5.0)}
    ref["gfi"], ref["lnhlh"] = oracle.gfi(hand, fac, idx, 0.4, 0.1, K.PX), oracle.lnhlh(hand, fac, 0.4, 0.1, K.PX)
    return ref


def _meets_chain(what, out, ref, keys=SAME):
    """test_gpu_parity.py's bars (test_gpu_chain_f64.py's for HAND as float64): codes, slope, accumulation, river, index,
    HAND and downslope exact; flow distance 1e-6; TI / MTI on the step's own slope and GFI / ln(hl/H) 1e-5"""
    import oracle
    from conftest import assert_float_close
    for k in keys:
        assert np.array_equal(out[k], ref[k].astype(out[k].dtype)), "%s: %s: %d cells differ" % (what, k, int((out[k] != ref[k]).sum()))
    assert np.array_equal(out["hand"], ref["hand"].astype(out["hand"].dtype)), what + ": hand"
    assert_float_close(out["fdist"], ref["fdist"], rtol=1e-6, what=what + ": flow distance")
    slr = out["slope_rad"] if "slope_rad" in out else np.where(ref["slope"] == -100, -100, np.arctan(ref["slope"] / 100))
    if "ti" in out:
        ti, mti = oracle.twi(ref["fac"], slr.astype(np.float32), K.PX, 0.1)
        assert_float_close(out["ti"], ti, rtol=1e-5, what=what + ": ti")
        assert_float_close(out["mti"], mti, rtol=1e-5, atol=1e-6, what=what + ": mti")
    assert_float_close(out["gfi"], ref["gfi"], rtol=1e-5, atol=1e-6, what=what + ": gfi")
    assert_float_close(out["lnhlh"], ref["lnhlh"], rtol=1e-5, atol=1e-6, what=what + ": lnhlh")


def _chain_step(dem, heights):
    """one step of a Chain on one stream; every buffer is the context's (dt_dev_malloc), made while the key is set"""
    from descriptools_amd import chain, device
    H, W = dem.shape
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=K.PX, overlap=False, tune_placement=False, heights=heights, river_threshold=THR,
                     n_top=0.1, n_gfi=0.4, b=0.1, dz=5.0)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float64 if heights == "float64" else np.float32))
    try:
        ch.run(d.ptr)
        ctx.sync()
        return {k: ch.buf[k].to_host() for k, _ in ch.outputs}
    finally:
        d.free()
        ch.free()
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("heights", ["float32", "float64"])
def test_chain_step(heights, poison):
    dem = K.relief(K.SEED)
    ref = _chain_reference(dem)
    assert ref["river"].any() and (ref["fdr"] == 0).any()
    poison(None)
    clean = _chain_step(dem, heights)
    assert clean["hand"].dtype == (np.float64 if heights == "float64" else np.float32)
    _meets_chain("clean", clean, ref)
    for b in BYTES:
        poison(b)
        got = _chain_step(dem, heights)
        poison(None)
        _meets_chain("0x%02X" % b, got, ref)
        K.same_bytes("chain step, memory filled with 0x%02X" % b, got, clean)


RANK_NAMES = ("fdr", "fac", "river", "fdist", "idx", "hand", "slope", "ti", "mti", "gfi", "lnhlh", "down")


def _rank_tile(shape):
    from descriptools_amd import tiling
    layout = tiling.Layout([shape[0]], [shape[1]])
    return layout, tiling.RankTile(layout, 0, device=0, px=K.PX, river_threshold=THR, tune_placement=False)


def _rank_step(t, layout, dem):
    """one step of a single RankTile through the windowed entries and the rank-level solves (scratch, scratch2 and aux
    are the knob's).  The tile's rasters and work planes are torch's (torch.zeros for the rasters, whose halos must read
    as zeros; torch.empty for the lift tables and temporaries): torch's memory is outside the knob, none of it is
    allocated by this test, and the test leaves all of it as RankTile made it.  A tile takes step after step, so one
    tile serves every pattern"""
    from descriptools_amd import tiling
    h = tiling.HALO
    pad = np.full((layout.Hg + 2 * h, layout.Wg + 2 * h), np.nan, np.float32)  # NaN = must never be read
    pad[h:h + layout.Hg, h:h + layout.Wg] = dem
    t.set_dem_ext(pad[:t.He, :t.We])
    tiling.simulate_dev([t], layout)
    assert t.unresolved_downslope() == 0
    return {n: t.host(n) for n in RANK_NAMES}


@pytest.mark.gpu
def test_rank_tile_step(poison):
    import torch
    dem = K.relief(K.SEED, (128, 128), hole=False)
    dem[56:72, 58:80] = -100
    ref = _chain_reference(dem)
    assert ref["river"].any()
    poison(None)
    layout, t = _rank_tile(dem.shape)
    try:
        clean = _rank_step(t, layout, dem)
        _meets_chain("clean", clean, ref)
        for b in BYTES:
            poison(b)
            got = _rank_step(t, layout, dem)
            poison(None)
            _meets_chain("0x%02X" % b, got, ref)
            K.same_bytes("rank tile step, memory filled with 0x%02X" % b, got, clean)
    finally:
        t.free()
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_the_key_fills_what_the_library_hands_out(poison):
    """the seam itself: a block of dt_dev_malloc reads back as the byte, and so do the 256 bytes dt_scratch_reset adds
    behind what an entry asks for, which no layout carves; with the key off, or at a value without bit 0x100, the same
    call leaves a pattern the test wrote there alone"""
    import ctypes as C
    from descriptools_amd import _lib, device
    L = _lib.lib()
    fdr = np.full((70, 70), 1, np.uint8)
    ctx = device.Context()
    try:
        d_fdr, d_out = ctx.to_device(fdr), ctx.empty((70, 70), np.float64)
        for b in BYTES:
            poison(b)
            a = ctx.empty((4099,), np.uint8)
            _lib.check(L.dt_dev_upslope_length(ctx.h, d_fdr.ptr, None, 70, 70, 10.0, d_out.ptr))
            poison(None)
            assert (a.to_host() == b).all(), "dt_dev_malloc, 0x%02X" % b
            a.free()
            n = int(L.dt_ctx_scratch_bytes(ctx.h))
            tail = np.empty(256, np.uint8)
            _lib.check(L.dt_dev_d2h(ctx.h, tail.ctypes.data_as(C.c_void_p),
                                    C.c_void_p(L.dt_ctx_scratch_ptr(ctx.h) + n - 256), 256))
            assert (tail == b).all(), "the context scratch, 0x%02X" % b
        np.testing.assert_array_equal(d_out.to_host()[0], np.arange(70) * 10.0)
        # off, and a value without bit 0x100: nothing is filled -- a pattern of the test's own in the pad survives the call,
        # and so does one in a block that dt_dev_malloc hands out again... which it need not, so only the pad is held to it
        where = C.c_void_p(L.dt_ctx_scratch_ptr(ctx.h) + n - 256)
        mine = np.full(256, 0x3C, np.uint8)
        for value in (0, 0xA5, 0xFF):
            _lib.check(L.dt_dev_h2d(ctx.h, where, mine.ctypes.data_as(C.c_void_p), 256))
            assert L.dt_debug_set(KEY, value) == 0
            _lib.check(L.dt_dev_upslope_length(ctx.h, d_fdr.ptr, None, 70, 70, 10.0, d_out.ptr))
            poison(None)
            _lib.check(L.dt_dev_d2h(ctx.h, tail.ctypes.data_as(C.c_void_p), where, 256))
            assert (tail == 0x3C).all(), "key %#x fills nothing" % value
        assert n == int(L.dt_ctx_scratch_bytes(ctx.h))
        d_fdr.free()
        d_out.free()
    finally:
        ctx.close()
