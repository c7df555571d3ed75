"""Device-resident descriptor chain (net-new, additive): slope -> D8 -> flow accumulation -> river
mask -> flow distance / river index / HAND -> TI / MTI -> GFI -> ln(hl/H) -> downslope, every raster
staying in HBM between steps (the reference round-trips each descriptor through the host,
Example/example.py:59-91).  Parameters default to the example's (n_top 0.1, n_gfi 0.4, b 0.1, dz 5)."""
import ctypes as C

import numpy as np

from . import _lib, placement
from ._lib import check
from .device import Context

F32, F64, U8, I8, I32 = np.float32, np.float64, np.uint8, np.int8, np.int32

OUTPUTS = (("slope", F32), ("fdr", U8), ("fac", I32), ("river", I8), ("fdist", F32), ("idx", I32),
           ("hand", F32), ("a_river", I32), ("slope_rad", F32), ("ti", F32), ("mti", F32), ("gfi", F32),
           ("lnhlh", F32), ("down", F32))

# Unfused algorithmic bytes per cell of the chain: slope 8, D8 5, flow-acc 5, river
# mask 5, HAND 18, TI+MTI 16, GFI 12, ln(hl/H) 12, downslope 9.
ALGO_BYTES_PER_CELL = 90

# rasters that one kernel writes together (placement.py: such a group must not sit in a single conflict class); the
# single-role "groups" just take what is left
WRITE_GROUPS = (("slope", "ti", "mti"), ("fdist", "idx", "hand", "gfi", "lnhlh"), ("fac",), ("a_river",),
                ("slope_rad",), ("down",))

# The ops of one step in launch order: (name, compulsory bytes per cell of the op AS FUSED HERE, kernels behind it
# as rocprofv3 names them).  Flow accumulation + river mask + HAND's first phase is one op: the last accumulation tile
# pass and HAND's first tile pass are one kernel (k_fa3fh1: fdr 1 read, acc 4 + river 1 written; then the perimeter
# node doubling, 2 B/cell by the unfused definition fdr 1 + river 1).  HAND's last pass with the fused GFI + ln(hl/H)
# epilogue reads dem 4 + fac 4 and writes fdist, idx, hand, gfi, lnhlh (20).  "d8" writes fdr only: slope comes out of
# the fused slope+TI+MTI stencil (dem 4 + fac 4 read, slope 4 + TI 4 + MTI 4 written = the north_star's 20 B/cell).
#
# That is the step as the profiles/r4 set measured it, and the step of every path that still launches the stencil
# (external_fdr, condition, want_slope_rad, rows that are not whole 64-cell tiles, the ranks of tiling.py); the tuple
# stays as it is because tests/test_profiles.py and tools/design_table.py tie it to those profiles.  The plain float32
# chain (Chain._from_d8) distributes the slope_twi bytes differently since round 6: "d8" runs k_d8_slope and writes the
# slope on its way (fdr 1 + slope 4 + the marks), "flowacc_flowhand_local" runs k_fa3fh1_twi, which reads that slope (4)
# and writes TI + MTI (8) beside the accumulation it has in registers, and "slope_twi" is only k_slope_twi_fix over
# the marked cells (microseconds on terrain): dem 4 + fac 4 are no longer read a second time, and a per-op rate
# computed from the 20 B/cell of "slope_twi" means nothing for that chain.  The kernel names are the r4
# profile's, not the live ones: the stencil pair is k_slope_twi<true, false, int> and k_slope_twi_fix<int> today.
# Since round 13 a single raster's "flowacc_flowhand_local" (this chain, external_fdr and float64 heights included; not
# the ranks) runs the walk form, k_fa3fh1w_twi / k_fa3fh1w<ND>: HAND's half walks the fed perimeter entries and writes
# no word cache, and k_fh_tile1 is not launched; "flowhand_gfi_finish" is then k_fh_tile3_solve, which reads the codes
# and the river mask (2 B/cell in place of the 4 B/cell cache) and solves the tile itself, followed by
# k_fh_tile1_marked and k_fh_tile3_marked for the tiles it gives up (none on terrain) -- DESIGN.md 4.3.
OPS = (
    ("d8", 5, ["k_d8<false>", "k_d8_fix"]),
    ("downslope", 9, ["k_downslope_win<24>"]),
    ("flowacc_flowhand_local", 5 + 1 + 2, ["k_fa_tile1", "k_fa_reduce", "k_fa_poison", "k_fa3fh1<2>", "k_fh_tile1",
                                           "k_fh_ghost_init", "k_fh_node_jump"]),
    ("slope_twi", 20, ["k_slope_twi<true, false, 1, int, 1>", "k_slope_twi_fix<int, 1>"]),
    ("flowhand_gfi_finish", 28, ["k_fh_tile3<false, 1, 5, int>"]),
)

# The step of a heights="float64" chain (same form as OPS).  The D8 kernel reads the DEM at 8 B/cell and writes the
# codes and the float32 nodata proxy (1 + 4) that the flow-accumulation / HAND-index kernels read in place of the DEM
# (they only test it for nodata: unchanged kernels).  Downslope reads dem 8 + fdr 1, writes 4.  The slope stencil
# reads dem 8 + fac 4 and writes slope + TI + MTI (12).  HAND's last pass writes fdist + idx only (reading fdr 1 +
# river 1: no heights); a last pass reads dem 8 + idx 4 + fac 4 and writes hand (float64, 8) + GFI + ln(hl/H) (8).
OPS_F64 = (
    ("d8", 13, ["k_d8_f64"]),
    ("downslope", 13, ["k_downslope_win_f64"]),
    ("flowacc_flowhand_local", 4 + 1 + 4 + 1 + 2, ["k_fa_tile1", "k_fa_reduce", "k_fa_poison", "k_fa3fh1<2>",
                                                 "k_fh_tile1", "k_fh_ghost_init", "k_fh_node_jump"]),
    ("slope_twi", 24, ["k_slope_twi_f64<false>"]),
    ("flowhand_finish", 10, ["k_fh_tile3<false, 1, 5, int>"]),
    ("hand_gfi", 32, ["k_hand_gfi_f64"]),
)

HEIGHTS = ("float32", "float64")


class Chain:
    """Owns the output rasters of one H x W tile on one device."""

    def __init__(self, H, W, ctx=None, px=10.0, n_top=0.1, n_gfi=0.4, b=0.1, dz=5.0,
                 river_threshold=None, alloc=None, want_slope_rad=True, side_ctx=None, overlap=True,
                 condition=False, condition_rounds=64, tune_placement=True, release=None, long_walks=False,
                 external_fdr=False, heights="float32"):
        # external_fdr: the D8 codes are GIVEN (a GIS tool's raster, as the reference's example reads one:
        # Example/example.py:36) -- the step has no D8 op; the caller writes the codes into buf["fdr"] (p("fdr")) first.
        # tune_placement: True (default) -- hand the blocks this chain allocates anyway to their roles by measured
        # write-conflict class (placement.py; ~100 probe launches, nothing else allocated); "search" -- also look for
        # blocks of other classes when those are all alike (bounded, transient allocations of tens of GiB: a set-up
        # option of a long-lived chain, what bench.py uses); False -- rasters in allocation order.
        """overlap (the default): downslope and the slope + TI + MTI stencil run as a second branch on their own stream
        (side_ctx, created on demand) beside the flow-accumulation / HAND kernels: ~3 % faster end to end at 16384^2.  overlap=False: one stream, kernels back to back (what per-kernel timings need:
        ops(serial=True) gives that order on a chain built either way).
        condition: the D8 codes come from the hydrologically conditioned surface (depressions filled, flats routed:
        dt_dev_condition_d8_async) instead of the plain steepest descent, for DEMs with pits and
        flats; the descriptors themselves keep using the DEM as given (as the reference's example does with a D8
        raster from a GIS tool, Example/example.py:36).  Nothing synchronises: `condition_rounds` fill / flat rounds
        are enqueued, and check_status() raises afterwards if that budget was too small for the raster."""
        # long_walks: for real, conditioned terrain, whose flats and valley floors make downslope walks thousands of
        # moves long (the bundled Example: 9.6 -> 1.0 ms).  True: the whole long-walk workspace up front
        # (dt_dev_downslope_lift, 56 B/cell), nothing synchronises.  "auto": the walks are queued (8 B/cell) and
        # finish_long_walks() -- a synchronisation point -- finishes them, with skip tables (25 B/cell more) only when
        # the raster has enough of them; run_host does this.  False: the plain kernel (the synthetic benchmark terrain
        # has no long walks).
        # heights: "float32" (the default) -- the DEM given to run / ops / capture is an H x W float32 raster;
        # "float64" -- an H x W float64 raster (a DEM float32 cannot hold: _lib.heights), every height difference taken
        # in float64 as the reference takes it in the DEM's own dtype.  buf["hand"] is then float64 (the reference's
        # HAND dtype on such a DEM); every other output keeps its dtype and meaning.  Out of scope on float64 heights:
        # condition=True (conditioned codes come in through external_fdr: dt_dev_condition_d8_f64_async), long_walks
        # (the skip tables are float32).  Several GPUs: tiling.RankTile(heights="float64").
        if heights not in HEIGHTS:
            raise ValueError("heights must be one of %s, not %r" % (HEIGHTS, heights))
        self.wide = heights == "float64"
        if self.wide and condition:
            raise ValueError("condition=True is float32-only in Chain: on float64 heights condition the codes with "
                             "dt_dev_condition_d8_f64_async into Chain(heights=\"float64\", external_fdr=True)'s "
                             "p(\"fdr\") (INTEGRATION.md), or use run_host(..., heights=\"float64\", condition=True)")
        if self.wide and long_walks is not False:
            raise ValueError("long_walks is float32-only: the float64 chain walks on its window kernel (long_walks=False)")
        assert long_walks in (False, True, "auto")
        assert not (external_fdr and condition), "conditioning computes the codes itself"
        self.outputs = tuple((k, F64 if (self.wide and k == "hand") else dt) for k, dt in OUTPUTS)
        self.external_fdr = bool(external_fdr)
        self.long_walks = long_walks
        self._lift = self._lift_q = self._lift_dem = self._lift_tables = None
        self.condition, self.condition_rounds = bool(condition), int(condition_rounds)
        self._alloc, self._release = alloc, release
        self.want_slope_rad = want_slope_rad
        self.H, self.W, self.N = int(H), int(W), int(H) * int(W)
        self.ctx = ctx or Context()
        self.side = None
        if overlap:
            self.side = side_ctx if side_ctx is not None else Context(device=self.ctx.device)
        self._own_side = overlap and side_ctx is None
        self.px, self.n_top, self.n_gfi, self.b, self.dz = px, n_top, n_gfi, b, dz
        self.river_threshold = self.N // 512 if river_threshold is None else int(river_threshold)
        self.buf = {}
        self._graphs = []
        for name, dt in self.outputs + ((("filled", F32),) if self.condition else ()):
            self.buf[name] = alloc((H, W), dt) if alloc else self.ctx.empty((H, W), dt)
        # the D8 kernel's nodata mask (one byte per four cells): what the accumulation pass needs of the DEM; on
        # float64 heights the float32 nodata proxy the first kernel writes (dt_dev_slope_d8_f64)
        self._nodata4 = self._proxy = self._marks = None
        if self.wide:
            self._proxy = self.ctx.empty((H, W), F32)
        elif not (self.external_fdr or self.condition):
            self._nodata4 = self.ctx.empty((int(_lib.lib().dt_nodata_mask_bytes(H, W)),), U8)
            # slope out of the D8 kernel, TI / MTI out of the last accumulation tile pass (ops()): the cells to redo
            # exactly are collected in marks of the chain's own, because three calls on two contexts share them
            if not want_slope_rad and _lib.lib().dt_slope_from_d8_ok(H, W):
                self._marks = self.ctx.empty((int(_lib.lib().dt_slope_marks_bytes(H, W)),), U8)
        assert tune_placement in (False, True, "search")
        self.placement = {"tuned": False, "why": "tune_placement=False"}
        if tune_placement:
            self._tune_placement(search=tune_placement == "search")

    def _tune_placement(self, search=False):
        """hand the 4-byte rasters to their roles so that no group of rasters written by one kernel lies in a single
        conflict class of the device's memory (placement.py; measured with ~100 timed launches of a write-only kernel
        at set-up, skipped for rasters below 64 MiB).  With the chain's own allocator, or an `alloc` that comes with
        a `release`, further candidate blocks are tried when the first twelve are all alike."""
        four = [name for name, dt in self.outputs if np.dtype(dt).itemsize == 4]
        objs = {}
        for name in four:
            b = self.buf[name]
            objs[int(b.ptr.value if hasattr(b, "ptr") else b)] = b

        def extra_alloc():
            b = self._alloc((self.H, self.W), F32) if self._alloc else self.ctx.empty((self.H, self.W), F32)
            q = int(b.ptr.value if hasattr(b, "ptr") else b)
            objs[q] = b
            return q

        def extra_release(q):
            b = objs.pop(q)
            if hasattr(b, "free"):
                b.free()
            elif self._release is not None:
                self._release(q)
        can_grow = search and (self._alloc is None or self._release is not None)

        def spacer_alloc(nbytes):
            rows = max(int(nbytes) // (self.W * 4), 1)
            if self._alloc:
                return ("user", self._alloc((rows, self.W), F32))
            return ("own", self.ctx.empty((rows, self.W), F32))

        def spacer_release(h):
            kind, b = h
            if kind == "own":
                b.free()
            else:
                self._release(int(b.ptr.value if hasattr(b, "ptr") else b))
        groups = [[k for k in g if k in four] for g in WRITE_GROUPS]  # (float64 heights: hand has 8-byte cells)
        roles, info = placement.assign(self.ctx, self.N * 4, list(objs), [g for g in groups if g],
                                       extra_alloc if can_grow else None, extra_release if can_grow else None,
                                       spacer_alloc=spacer_alloc if can_grow else None,
                                       spacer_release=spacer_release if can_grow else None, search=search)
        self.placement = info
        if info.get("spacer_GiB"):
            # the runtime defers the release of the spacers: take the wait here, where it was caused
            for gib in (2, 16):
                try:
                    self.ctx.empty((gib << 30,), np.uint8).free()
                except MemoryError:
                    break
        if roles is None:
            return
        dts = dict(self.outputs)
        for name, q in roles.items():
            b = objs[q]
            if hasattr(b, "dtype"):
                b.dtype = np.dtype(dts[name])  # a block is just memory: it takes the dtype of the role it serves
            self.buf[name] = b

    def _lift_ptr(self):
        if self._lift is None:
            self._lift_bytes = int(_lib.lib().dt_downslope_lift_workspace(self.H, self.W))
            self._lift = self.ctx.empty((self._lift_bytes,), np.uint8)
        return self._lift.ptr

    def _queue_downslope(self, side, dem_ptr):
        L = _lib.lib()
        if self._lift_q is None:
            self._lift_q_bytes = int(L.dt_downslope_queue_workspace(self.H, self.W))
            self._lift_q = self.ctx.empty((self._lift_q_bytes,), np.uint8)
        self._lift_dem = dem_ptr
        return L.dt_dev_downslope_queue(side.h, dem_ptr, self.p("fdr"), self.H, self.W, self.px, self.dz, 0,
                                        self.p("down"), self._lift_q.ptr, self._lift_q_bytes)

    def finish_long_walks(self):
        """long_walks="auto": wait for the step, look at the queue of long downslope walks and finish them (skip tables
        only when there are enough of them to pay for a pass over the raster).  Returns the number of walks queued."""
        if self.long_walks != "auto" or self._lift_q is None:
            return 0
        L, c = _lib.lib(), self.ctx
        n = C.c_int64(0)
        check(L.dt_dev_downslope_queued(c.h, self._lift_q.ptr, C.byref(n)))
        if n.value == 0:
            return 0
        tables, tb = None, 0
        if n.value >= int(L.dt_downslope_tables_threshold(self.H, self.W)):
            # the skip tables (25 bytes per cell) are kept once a step needed them: a raster that has long walks has
            # them in every step, and allocating 5 GB per step is not free
            tb = int(L.dt_downslope_tables_workspace(self.H, self.W))
            if self._lift_tables is None:
                try:
                    self._lift_tables = c.empty((tb,), np.uint8)
                except MemoryError:  # (DT_ENOMEM: the walks are then made move by move)
                    tb = 0
            tables = self._lift_tables
        check(L.dt_dev_downslope_finish(c.h, self._lift_dem, self.p("fdr"), self.H, self.W, self.px, self.dz, 0,
                                        self.p("down"), self._lift_q.ptr, self._lift_q_bytes,
                                        tables.ptr if tables is not None else None, tb if tables is not None else 0))
        c.sync()
        return int(n.value)

    def p(self, name):
        b = self.buf[name]
        return b.ptr if hasattr(b, "ptr") else b

    def ops(self, dem_ptr, want_a_river=False, serial=False):
        """The step as a list of (name, context, call) in launch order -- THE definition of the chain: run()
        executes it, bench.py times it op by op.  With `overlap` the downslope and slope_twi ops belong to the side
        context (run() forks it before each of them and joins at the end); serial=True binds every op to the main
        context (one stream, back to back), whatever the chain was built with."""
        L, c, H, W = _lib.lib(), self.ctx, self.H, self.W
        p = self.p
        side = self.side if (self.side is not None and not serial) else c
        if getattr(self, "_full", None) is None:
            self._full = _lib.Window(H, W, W, 0, 0, H, W, 0)
        full = self._full
        if self.wide:
            return self._ops_f64(dem_ptr, want_a_river, side)
        rad = p("slope_rad") if self.want_slope_rad else None
        m4 = self._nodata4.ptr if self._nodata4 is not None else None
        first = ("d8", c, lambda: L.dt_dev_slope_d8_m(c.h, dem_ptr, H, W, self.px, p("fdr"), m4))
        flow = ((lambda: L.dt_dev_flowacc_river_flowhand_local_m(c.h, p("fdr"), dem_ptr, m4, H, W, self.river_threshold,
                                                                 p("fac"), p("river"))) if m4 is not None else
                (lambda: L.dt_dev_flowacc_river_flowhand_local(c.h, p("fdr"), dem_ptr, H, W, self.river_threshold,
                                                               p("fac"), p("river"))))
        twi = lambda: L.dt_dev_slope_twi(side.h, dem_ptr, p("fac"), H, W, self.px, self.n_top, p("slope"), rad, p("ti"),
                                         p("mti"))
        if self._from_d8(dem_ptr):
            # The same five ops without a slope + TI + MTI pass over the raster: the D8 kernel writes the slope from the
            # neighbourhood it holds (marking the cells whose float32 slope is not proven), flow accumulation's last
            # tile pass writes TI / MTI from that slope and the accumulation in its registers (marking the cells its
            # fast path rejects), and "slope_twi" is the exact recomputation of the marked cells alone -- bit for bit
            # what dt_dev_slope_twi writes.
            marks = self._marks.ptr
            first = ("d8", c, lambda: L.dt_dev_slope_d8_ms(c.h, dem_ptr, H, W, self.px, p("fdr"), m4, p("slope"), marks))
            flow = lambda: L.dt_dev_flowacc_river_flowhand_local_ms(
                c.h, p("fdr"), dem_ptr, m4, H, W, self.river_threshold, p("fac"), p("river"), self.px, self.n_top,
                p("slope"), p("ti"), p("mti"), marks)
            twi = lambda: L.dt_dev_slope_twi_fix(side.h, dem_ptr, p("fac"), H, W, self.px, self.n_top, p("slope"),
                                                 p("ti"), p("mti"), marks)
        if self.condition:
            first = ("condition_d8", c, lambda: L.dt_dev_condition_d8_async(c.h, dem_ptr, H, W, self.px, p("filled"),
                                                                             p("fdr"), self.condition_rounds))
        return ([] if self.external_fdr else [first]) + [
            ("downslope", side, (lambda: L.dt_dev_downslope_lift(side.h, dem_ptr, p("fdr"), H, W, self.px, self.dz, 0,
                                                                  p("down"), self._lift_ptr(), self._lift_bytes))
             if self.long_walks is True else
             (lambda: self._queue_downslope(side, dem_ptr)) if self.long_walks == "auto" else
             (lambda: L.dt_dev_downslope(side.h, dem_ptr, p("fdr"), H, W, self.px, self.dz, 0, p("down")))),
            ("flowacc_flowhand_local", c, flow),
            ("slope_twi", side, twi),
            ("flowhand_gfi_finish", c, lambda: L.dt_dev_flowhand_gfi_finish_w(
                c.h, C.byref(full), dem_ptr, p("fdr"), p("river"), p("fac"), self.px, self.n_gfi, self.b, None, None,
                None, None, None, None, p("fdist"), p("idx"), None, p("hand"),
                p("a_river") if want_a_river else None, p("gfi"), p("lnhlh"))),
        ]

    def _from_d8(self, dem_ptr=None):
        """does the step take slope from the D8 kernel and TI / MTI from the accumulation pass?  (the plain float32
        chain without slope_rad, on rows of whole 64-cell tiles and 16-byte aligned rasters; same rasters either way)"""
        if self._marks is None:  # (allocated only without slope_rad and on a shape dt_slope_from_d8_ok accepts)
            return False
        ptrs = [self.p(k) for k in ("slope", "fac", "ti", "mti", "river", "fdr")] + ([dem_ptr] if dem_ptr else [])
        return all((int(q.value if hasattr(q, "value") else q) & 15) == 0 for q in ptrs)

    def _ops_f64(self, dem_ptr, want_a_river, side):
        """ops() of a heights="float64" chain (OPS_F64): the DEM pointer is a float64 raster.  The flow-accumulation /
        HAND-index kernels are the float32 chain's, reading the nodata proxy in place of the DEM; HAND's last pass
        writes fdist / idx only, and a pass of its own takes HAND in float64 and GFI / ln(hl/H) from it."""
        L, c, H, W, p = _lib.lib(), self.ctx, self.H, self.W, self.p
        prox = self._proxy.ptr
        rad = p("slope_rad") if self.want_slope_rad else None
        first = ("d8", c, lambda: L.dt_dev_slope_d8_f64(c.h, dem_ptr, H, W, self.px, p("fdr"), prox))
        if self.external_fdr:  # the codes are given: the first kernel writes the proxy only
            first = ("nodata_proxy", c, lambda: L.dt_dev_slope_d8_f64(c.h, dem_ptr, H, W, self.px, None, prox))
        return [
            first,
            ("downslope", side, lambda: L.dt_dev_downslope_f64(side.h, dem_ptr, p("fdr"), H, W, self.px, self.dz, 0,
                                                               p("down"))),
            ("flowacc_flowhand_local", c, lambda: L.dt_dev_flowacc_river_flowhand_local(
                c.h, p("fdr"), prox, H, W, self.river_threshold, p("fac"), p("river"))),
            ("slope_twi", side, lambda: L.dt_dev_slope_twi_f64(side.h, dem_ptr, p("fac"), H, W, self.px, self.n_top,
                                                               p("slope"), rad, p("ti"), p("mti"))),
            ("flowhand_finish", c, lambda: L.dt_dev_flowhand_finish_w(
                c.h, C.byref(self._full), None, p("fdr"), p("river"), p("fac"), self.px, None, None, None, None, None,
                None, p("fdist"), p("idx"), None, None, p("a_river") if want_a_river else None)),
            ("hand_gfi", c, lambda: L.dt_dev_hand_gfi_f64(c.h, dem_ptr, p("idx"), p("fac"), H, W, self.px, self.n_gfi,
                                                          self.b, p("hand"), p("gfi"), p("lnhlh"))),
        ]

    def run(self, dem_ptr, want_a_river=True):
        """Enqueue the whole chain (asynchronous).  With `overlap` the side context's stream carries a second branch:
        downslope (needs only the DEM and the D8 codes) from the D8 kernel on, then the slope + TI + MTI stencil (needs
        the accumulation) beside HAND's last pass; the branches join at the end.  Of the two-stream schedules tried
        (tools/schedule_probe.py, profiles/r3/schedule_probe.txt) this is the fastest by a small margin: every
        split of these kernels over two streams lands within 0.3 ms of the serial order, stream priorities and the
        fork point make no difference -- concurrent kernels share LDS and bandwidth, they do not add them."""
        for name, ctx, call in self.ops(dem_ptr, want_a_river):
            if ctx is not self.ctx:
                self.ctx.fork(ctx)  # the branch sees everything enqueued on the main stream so far
            check(call())
        if self.side is not None:
            self.ctx.join(self.side)

    def check_status(self):
        """raise if a kernel of the steps so far flagged a condition that invalidates their rasters (conditioning out
        of rounds); synchronises"""
        self.ctx.raise_on_status()

    def capture(self, dem_ptr, want_a_river=True):
        """The step as a HIP graph: runs it once (workspaces, tables), records a second run, returns a `Graph` whose
        launch() replays the ~45 kernel launches with one.  It takes the host out of the step (one call instead
        of 45 through ctypes), not time off it: measured 0.213 / 0.324 / 9.05 ms direct against 0.226 / 0.336 /
        8.98 ms replayed at 1024^2 / 2048^2 / 16384^2 -- the asynchronous launches already keep ahead of the GPU,
        and what a small step costs is the ~5 us each dependent kernel takes to start, which a graph of the same
        kernels keeps.  Baked into the graph: the DEM pointer, this chain's buffers AND the context's workspaces
        (scratch, stencil marks).  The graph keeps the chain and its context alive; it becomes invalid -- launch()
        raises -- when the chain is freed, or when a later call on the context needs a larger workspace and
        reallocates it (a bigger raster, conditioning, a rank-level solve): capture again then."""
        self.run(dem_ptr, want_a_river)
        self.ctx.sync()
        L = _lib.lib()
        check(L.dt_ctx_capture_begin(self.ctx.h))
        g = C.c_void_p()
        try:
            self.run(dem_ptr, want_a_river)
        except BaseException:
            # end the capture and drop whatever was recorded: no half-built graph is handed out or leaked
            if L.dt_ctx_capture_end(self.ctx.h, C.byref(g)) == 0 and g:
                L.dt_graph_destroy(g)
            raise
        check(L.dt_ctx_capture_end(self.ctx.h, C.byref(g)))
        gr = Graph(g, self.ctx, self)
        self._graphs.append(gr)
        return gr

    def free(self):
        for gr in self._graphs:  # their kernels point into the buffers that go away now
            gr.invalidate("the chain it was captured from has been freed")
        self._graphs = []
        if self._own_side:
            self.side.close()
            self.side, self._own_side = None, False
        for b in list(self.buf.values()):
            if hasattr(b, "free"):
                b.free()
        self.buf = {}
        for name in ("_lift", "_lift_q", "_lift_tables", "_nodata4", "_proxy", "_marks"):
            if getattr(self, name) is not None:
                getattr(self, name).free()
                setattr(self, name, None)


class Graph:
    """A captured step (Chain.capture).  Holds its chain and context (their buffers and workspaces are what the
    recorded kernels address)."""

    def __init__(self, handle, ctx, chain=None):
        self.h, self.ctx, self.chain, self._dead = handle, ctx, chain, None

    def invalidate(self, why):
        self._dead = why

    def launch(self):
        if self._dead:
            raise RuntimeError("captured step cannot be replayed: " + self._dead)
        check(_lib.lib().dt_graph_launch(self.h, self.ctx.h))

    def free(self):
        if self.h:
            check(_lib.lib().dt_graph_destroy(self.h))
            self.h = None
        if self.chain is not None and self in self.chain._graphs:
            self.chain._graphs.remove(self)
        self.chain = None


def run_host(dem, px, timings=None, heights="float32", **kw):
    """Convenience: host DEM in, dict of host rasters out (fac / idx widened to int64 on the device).
    timings (optional dict): filled with the seconds spent per phase (set-up, H2D, host blocks + copies, release).
    heights: "float32" (default) -- float32-exact heights only (_lib.dem_f32: ValueError otherwise); "float64" -- the
    float64 chain (Chain(heights="float64")): hand comes back as float64, long_walks defaults to False; "auto" -- the
    float64 chain exactly when float32 cannot hold the DEM (_lib.heights, the drop-in functions' rule).
    condition=True on the float64 tier: the codes are conditioned in float64 (dt_dev_condition_d8_f64_async,
    `condition_rounds` rounds, default 64) and fed to a Chain(heights="float64", external_fdr=True) -- the resident
    recipe of INTEGRATION.md; the same keys come back as on the float32 tier."""
    import time
    t0 = time.perf_counter()
    d, wide = _lib.dem_tier(dem, heights)
    H, W = d.shape
    cond64 = None  # the float64 tier's conditioning rounds, when it conditions
    if wide:  # (out-of-scope arguments are refused before any device work)
        if kw.get("long_walks", False) is not False:
            raise ValueError("long_walks is float32-only: the float64 chain walks on its window kernel (long_walks=False)")
        if kw.pop("condition", False):
            if kw.get("external_fdr"):
                raise ValueError("condition=True computes the codes itself: external_fdr must be False")
            cond64 = int(kw.pop("condition_rounds", 64))
            kw["external_fdr"] = True
    ctx = Context()
    kw.setdefault("tune_placement", False)  # one step: the ~0.1 s of measurement would buy 0.3 ms
    # real terrain: long downslope walks are finished with skip tables (float32 heights only)
    kw.setdefault("long_walks", False if wide else "auto")
    ch = Chain(H, W, ctx=ctx, px=px, heights="float64" if wide else "float32", **kw)
    t1 = time.perf_counter()
    d_dem = ctx.to_device(d)
    widened = {k: ctx.empty((H, W), np.int64) for k in ("fac", "idx")}  # the reference's dtypes for these are int64
    filled = ctx.empty((H, W), np.float64) if cond64 is not None else None
    t2 = t3 = t4 = time.perf_counter()
    try:
        if filled is not None:
            check(_lib.lib().dt_dev_condition_d8_f64_async(ctx.h, d_dem.ptr, H, W, float(px), filled.ptr, ch.p("fdr"),
                                                           cond64))
        ch.run(d_dem.ptr)
        ch.check_status()  # (condition=True: raises when the budget of conditioning rounds was too small)
        if filled is not None:
            filled.free()
        ch.finish_long_walks()
        # rasters come back into page-locked host memory from a recycling pool (device.PinnedPool): the copies are
        # the cost of this call, not the kernels.  Copies are only enqueued: raster k crosses PCIe while the host
        # block of raster k + 1 is being mapped and touched; one synchronisation at the end.
        out = {}
        for k, _ in ch.outputs:
            if k in widened:
                check(_lib.lib().dt_dev_i32_to_i64(ctx.h, ch.buf[k].ptr, ch.N, widened[k].ptr))
                out[k] = widened[k].to_host_async()
            else:
                out[k] = ch.buf[k].to_host_async()
        t3 = time.perf_counter()
        ctx.sync()
        t4 = time.perf_counter()
    finally:
        d_dem.free()
        for w_ in widened.values():
            w_.free()
        if filled is not None:
            filled.free()
        ch.free()
        ctx.close()
    if timings is not None:
        timings.update({"setup_s": round(t1 - t0, 4), "h2d_s": round(t2 - t1, 4),
                        "host_blocks_and_enqueue_s": round(t3 - t2, 4), "wait_for_copies_s": round(t4 - t3, 4),
                        "release_s": round(time.perf_counter() - t4, 4)})
    return out
