"""GPU (-m gpu): what the device tier (dt_dev_*) answers to calls it must refuse -- (entry, case) -> (rc, message).

Every case is refused on the host before anything is enqueued (or, for the empty rasters and the first phases that set
a case up, is a valid call on real rasters): no case hands a kernel a bad pointer or a wrong size.  EXPECTED was
recorded by running table() on the commit BEFORE the device tier moved onto the DevCall scaffold and the named
scratch-owner protocol (csrc/dt_capi.hip) and is never taken from the tree under test: the rejections, their order where
two can fail at once, their messages, and which empty call keeps or drops a two-phase claim are that commit's.

Each phase pair completing normally is covered by test_gpu_tiling.py, test_gpu_dinf.py and the chain tests."""
import ctypes as C
import os
import re

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 128
BIG = (65536, 32768)  # 2^31 cells: every shape check precedes any allocation
ZBYTES = 4 << 20      # the zero block that stands for "some raster": larger than any raster or workspace at 128 x 128

# scalars by parameter name (include/descriptools_hip.h); every other scalar is 0
SCALARS = dict(H=H, W=W, Hg=H, Wg=W, h=H, w=W, px=10.0, rounds=1, hand_bytes=4, idx_bytes=8, K=1, R=1, n=1, N=16, ty=1,
               tx=1, threshold=10, elevation_difference=5.0, dz=5.0, n_top=0.1, n_gfi=0.4, b=0.1, scale_factor=0.1,
               size=10.0, reps=1, blocks=1)
# workspaces are NULL unless a case gives one: a call that got past its raster checks would stop at the workspace rule
WORK = ("work", "qwork", "twork", "table", "walkers")
# overrides that a loop over many entries gives to all of them, whether they have the parameter or not
BROADCAST = {"stage", "H", "W", "h", "w", "work", "work_bytes", "qwork", "qbytes"}
# the first REQUIRED pointer, where it is not the first pointer
FIRST_REQUIRED = dict(dt_dev_flowhand="fdr", dt_dev_flowhand_local_w="fdr", dt_dev_flowhand_local_w_a64="fdr",
                      dt_dev_flowhand_finish_w="fdr", dt_dev_flowhand_finish_w_a64="fdr",
                      dt_dev_condition_stage_m_w="nsame", dt_dev_downslope_walk_w="dem")
# (entries without a pointer rule of their own: the stage launcher checks per stage)
NO_POINTER_RULE = ("dt_dev_condition_stage_w",)


def prototypes():
    """name -> [(parameter name, is a pointer)] of every dt_dev_* prototype of the header"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "descriptools_hip.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dt_dev_\w+)\s*\((.*?)\)\s*;", txt, re.S):
        ps = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        out[m.group(1)] = [(re.search(r"(\w+)$", p).group(1), "*" in p) for p in ps]
    return out


class Table:
    """runs the cases in order and keeps (case id, rc, message); message is "" for rc 0"""

    def __init__(self):
        import torch
        from descriptools_amd import _lib, device, tiling
        self.lib, self.L, self.protos = _lib, _lib.lib(), prototypes()
        self.rows = []
        self.t = t = tiling.RankTile(tiling.Layout([H], [W]), 0, device=0, river_threshold=10, tune_placement=False)
        t.synth_dem(3)
        t.d8()
        t.ctx.sync()
        self.h = t.ctx.h
        self.fresh = device.Context()
        self.z = torch.zeros(ZBYTES, dtype=torch.uint8, device=t.dev)
        self.z2 = torch.zeros(ZBYTES, dtype=torch.uint8, device=t.dev)
        self.angle = torch.full((H, W), -1.0, dtype=torch.float32, device=t.dev)  # no flow anywhere: done in round 0
        self.acc = torch.zeros((H, W), dtype=torch.float64, device=t.dev)
        self.out3 = torch.zeros(3, dtype=torch.float32, device=t.dev)
        # the ring summaries the first phases write: one entry per cell of the window's perimeter
        P = int(self.L.dt_perim_cells(H, W))
        ring = lambda *dts: [torch.zeros(P, dtype=dt, device=t.dev) for dt in dts]
        self.fa_ring = ring(torch.int64, torch.int32, torch.uint8)                       # A, xr, code
        self.fh_ring = ring(torch.uint8, torch.int32, torch.int32, torch.int32, torch.float32, torch.int64)
        torch.cuda.synchronize()
        self.Z = self.z.data_ptr()
        self.win = t.win
        self.win_other = _lib.Window(H, 64, t.We, 0, 0, H, W, t.halo)  # 128 x 64 of the same rasters
        self.host = {}

    # ---- calls --------------------------------------------------------------------------------------------------
    def args(self, name, **over):
        """the entry's arguments by parameter name: the context, the tile's window, SCALARS, the zero block for every
        pointer but the workspaces; `over` replaces any of them"""
        _, argtypes = self.lib._SIGS[name]
        unknown = set(over) - {p for p, _ in self.protos[name]} - BROADCAST
        assert not unknown, "%s has no parameter %s" % (name, sorted(unknown))
        out = []
        for (pname, is_ptr), ct in zip(self.protos[name], argtypes):
            if pname in over:
                v = over[pname]
            elif pname == "ctx":
                v = self.h
            elif pname == "win":
                v = C.byref(self.win)
            elif is_ptr and ct is not C.c_void_p:  # a host array
                v = self.host.setdefault((name, pname), (ct._type_ * 8)(*([1] + [0] * 7)))
            elif is_ptr:
                v = None if pname in WORK else self.Z
            else:
                v = SCALARS.get(pname, 0)
            out.append(v)
        return out

    def call(self, case, name, **over):
        rc = getattr(self.L, name)(*self.args(name, **over))
        self.rows.append(("%s: %s" % (name, case), rc, self.L.dt_last_error().decode() if rc else ""))
        return rc

    def ok(self, name, *a):
        """a valid call that sets a case up"""
        self.lib.check(getattr(self.L, name)(*a))

    # ---- the first phases and the six sites that check a claim, on the tile's own rasters --------------------------
    def fa_local(self, win=None):
        t = self.t
        self.ok("dt_dev_flowacc_local_w", self.h, C.byref(win or self.win), t.p("fdr"), t.p("fac"),
                *[r.data_ptr() for r in self.fa_ring])

    def fh_local(self, win=None):
        t = self.t
        self.ok("dt_dev_flowhand_local_w", self.h, C.byref(win or self.win), t.p("dem"), t.p("fdr"), t.p("river"),
                t.p("fac"), *[r.data_ptr() for r in self.fh_ring])  # kind, ref, nc, nd, zr, ar

    def dinf_start(self, shape=(H, W)):
        self.ok("dt_dev_dinf_accumulate", self.h, self.angle.data_ptr(), None, shape[0], shape[1], 10, 4,
                self.acc.data_ptr())

    def take_scratch(self):
        self.ok("dt_dev_unique_extremes_f32", self.h, self.t.p("dem"), 16, self.out3.data_ptr())

    def site(self, case, which, h=None, **over):
        t, h = self.t, h or self.h
        fh = [r.data_ptr() for r in self.fh_ring]
        hand = (t.p("fdist"), t.p("idx"), None, t.p("hand"), t.p("a_river"))
        if which == "dt_dev_flowacc_finish_w":
            a = (h, C.byref(self.win), t.p("fdr"), t.p("dem"), None, 10, t.p("fac"), t.p("river"))
        elif which == "dt_dev_flowacc_finish_flowhand_local_w":
            a = (h, C.byref(self.win), t.p("fdr"), t.p("dem"), None, 10, t.p("fac"), t.p("river"), *fh)
        elif which == "dt_dev_flowhand_finish_w":
            a = (h, C.byref(self.win), t.p("dem"), t.p("fdr"), t.p("river"), t.p("fac"), 10.0, *[None] * 6, *hand)
        elif which == "dt_dev_flowhand_gfi_finish_w":
            a = (h, C.byref(self.win), t.p("dem"), t.p("fdr"), t.p("river"), t.p("fac"), 10.0, 0.4, 0.1, *[None] * 6,
                 *hand, t.p("gfi"), t.p("lnhlh"))
        elif which == "dt_dev_dinf_accumulate":
            a = (h, over.get("angle", self.angle.data_ptr()), over.get("w"), H, W, over.get("frac_bits", 10), -1,
                 self.acc.data_ptr())
        else:
            self.info = (C.c_int64 * 4)()
            a = (h, self.info)
        rc = getattr(self.L, which)(*a)
        self.rows.append(("%s: %s" % (which, case), rc, self.L.dt_last_error().decode() if rc else ""))
        return rc


SITES = (("dt_dev_flowacc_finish_w", "fa_local", "fh_local"),
         ("dt_dev_flowacc_finish_flowhand_local_w", "fa_local", "fh_local"),
         ("dt_dev_flowhand_finish_w", "fh_local", "fa_local"),
         ("dt_dev_flowhand_gfi_finish_w", "fh_local", "fa_local"),
         ("dt_dev_dinf_accumulate", "dinf_start", "fa_local"),
         ("dt_dev_dinf_accumulate_info", "dinf_start", "fa_local"))


def table(T=None):
    """-> (rows, status words): every case in order, then dt_ctx_status of the two contexts the cases ran on"""
    T = T or Table()
    L, Z = T.L, T.Z
    nan, inf = float("nan"), float("inf")
    shaped = sorted(n for n, ps in T.protos.items() if n in T.lib._SIGS and any(p == "H" for p, _ in ps))
    windowed = sorted(n for n, ps in T.protos.items() if n in T.lib._SIGS and any(p == "win" for p, _ in ps))

    # shape rules: one entry per rule
    T.call("hw: negative H", "dt_dev_slope_d8", H=-1)
    T.call("hw: 2^31 cells", "dt_dev_slope_d8", H=BIG[0], W=BIG[1])
    T.call("ws: negative H", "dt_dev_drainage", H=-1)
    T.call("ws: 2^31 cells", "dt_dev_drainage", H=BIG[0], W=BIG[1])
    for px in (nan, inf, 0.0):
        T.call("ws: px %r" % px, "dt_dev_drainage", px=px)
    T.call("so: negative H", "dt_dev_stream_order", H=-1)
    T.call("so: too large", "dt_dev_stream_order", H=1 << 42, W=2)
    T.call("so: 2^31 cells pass the rule", "dt_dev_stream_order", H=BIG[0], W=BIG[1], fdr=None)

    # dt_convert_window's six messages, and a NULL window through every windowed entry
    Wn = T.lib.Window
    for what, win in (("bad core shape", Wn(-1, W, W, 0, 0, H, W, 0)), ("ld < W", Wn(H, W, W - 1, 0, 0, H, W, 0)),
                      ("outside the global raster", Wn(H, W, W, 1, 0, H, W, 1)),
                      ("negative halo", Wn(H, W, W, 0, 0, H, W, -1)),
                      ("inside a larger raster without a halo", Wn(H, W, W, 0, 0, 2 * H, W, 0))):
        T.call("window: " + what, "dt_dev_slope_d8_w", win=C.byref(win))
    for name in windowed:
        T.call("window: NULL", name, win=None)

    # the first required pointer NULL on a non-empty shape
    for name in shaped + windowed + ["dt_dev_synth_dem"]:
        if name in NO_POINTER_RULE:
            continue
        ptrs = [p for p, is_ptr in T.protos[name] if is_ptr and p not in ("ctx", "win")]
        first = FIRST_REQUIRED.get(name, ptrs[0])
        T.call("NULL %s" % first, name, **{first: None, "stage": 2})
    # the paired rules
    T.call("no output", "dt_dev_slope_d8", slope=None, fdr=None, slope_rad=None)
    T.call("bad shape", "dt_dev_synth_dem", Hg=0)
    for name in ("dt_dev_flowhand", "dt_dev_flowhand_finish_w", "dt_dev_flowhand_finish_w_a64"):
        T.call("hand needs dem", name, dem=None)
        T.call("a_river needs the accumulation", name, **{"acc64" if name.endswith("a64") else "acc32": None})
    for name in ("dt_dev_flowhand_finish_w", "dt_dev_flowhand_gfi_finish_w", "dt_dev_flowhand_gfi_finish_w_a64"):
        T.call("incomplete rank-exit results", name, res_nc=None)
    T.call("fused: gfi NULL", "dt_dev_flowhand_gfi_finish_w", gfi=None)
    T.call("fused: gfi NULL", "dt_dev_flowhand_gfi", gfi=None)
    T.call("label requires pour", "dt_dev_drainage", pour=None)
    T.call("catch needs idx", "dt_dev_reach_catchments", idx=None)
    T.call("catch needs idx: element size", "dt_dev_reach_catchments", idx_bytes=3)
    T.call("negative capacity", "dt_dev_reach_catchments", cap=-1)
    for R in (-1, 1 << 31):
        for name in ("dt_dev_reach_channels", "dt_dev_reach_tables", "dt_dev_inundate"):
            T.call("reach count %d" % R, name, R=R)
    T.call("NULL output", "dt_dev_reach_channels", end=None)
    T.call("NULL table", "dt_dev_reach_tables", cells=None)
    for name in ("dt_dev_reach_tables", "dt_dev_inundate"):
        T.call("hand_bytes 2", name, hand_bytes=2)
    f64 = lambda *v: (C.c_double * 8)(*(list(v) + [0.0] * (8 - len(v))))
    T.call("stages: K 0", "dt_dev_reach_tables", K=0)
    T.call("stages: K 1025", "dt_dev_reach_tables", K=1025)
    T.call("stages: NULL", "dt_dev_reach_tables", stages=None)
    T.call("stages: nan", "dt_dev_reach_tables", stages=f64(nan))
    T.call("stages: negative", "dt_dev_reach_tables", stages=f64(-1.0))
    T.call("stages: not increasing", "dt_dev_reach_tables", stages=f64(2.0, 2.0), K=2)
    T.call("stages: frac_bits too fine", "dt_dev_reach_tables", frac_bits=60)
    for name in ("dt_dev_reach_tables", "dt_dev_flowacc_weighted", "dt_dev_dinf_accumulate"):
        for fb in (2201, -2201):
            T.call("frac_bits %d" % fb, name, frac_bits=fb)
    for r in (0, 4097, -4097):
        T.call("rounds %d" % r, "dt_dev_dinf_accumulate", rounds=r)
    T.call("the nodata mask is required", "dt_dev_flowacc_river_flowhand_local_m", nodata4=None)
    T.call("marks NULL", "dt_dev_flowacc_river_flowhand_local_ms", marks=None)
    P = int(L.dt_perim_cells(H, W))
    for n in (-1, P + 1):
        T.call("ring size %d" % n, "dt_dev_flowhand_zr64_w", n=n)
    for name in ("dt_dev_downslope_walk_w", "dt_dev_downslope_walk_route_w", "dt_dev_downslope_walk_route_f64_w",
                 "dt_dev_downslope_walk_seed_w", "dt_dev_downslope_walk_seed_f64_w"):
        T.call("negative count", name, n=-1)
    for name in ("dt_dev_downslope_walk_route_w", "dt_dev_downslope_walk_route_f64_w"):
        T.call("layout: ty 0", name, ty=0)
        T.call("layout: counts NULL", name, counts=None)
    for name in ("dt_dev_hand_gfi_f64_w", "dt_dev_hand_gfi_f64_w_a64"):
        T.call("incomplete rank-exit results", name, n_remote=1, rem_gidx=None)
        T.call("negative n_remote", name, n_remote=-1)
    T.call("bad arguments", "dt_dev_unique_extremes_f32", x=None)

    # workspaces: missing, and one byte too small
    lift, queue, tables = (int(getattr(L, "dt_downslope_%s_workspace" % k)(H, W)) for k in ("lift", "queue", "tables"))
    lift_w = int(L.dt_downslope_lift_workspace_w(C.byref(T.win)))
    tab = int(L.dt_hand_f64_table_bytes(1))
    assert max(lift, lift_w, queue + tables, tab) <= ZBYTES
    T.call("work missing", "dt_dev_downslope_lift")
    T.call("work small", "dt_dev_downslope_lift", work=Z, work_bytes=lift - 1)
    for name in ("dt_dev_downslope_queue", "dt_dev_downslope_finish"):
        T.call("queue missing", name)
        T.call("queue small", name, qwork=Z, qbytes=queue - 1)
    T.call("tables small", "dt_dev_downslope_finish", qwork=Z, qbytes=queue, twork=T.z2.data_ptr(), tbytes=tables - 1)
    T.call("work missing", "dt_dev_downslope_lift_w")
    for name in ("dt_dev_downslope_lift_w", "dt_dev_downslope_emit_w", "dt_dev_downslope_walk_w",
                 "dt_dev_downslope_walk_route_w"):
        T.call("work small", name, work=Z, work_bytes=lift_w - 1)
    T.call("walkers missing", "dt_dev_downslope_emit_w")
    T.call("walkers small", "dt_dev_downslope_emit_w", walkers=Z, walkers_bytes=256 + 47)
    for name in ("dt_dev_hand_gfi_f64_w", "dt_dev_hand_gfi_f64_w_a64"):
        T.call("table missing", name, n_remote=1)
        T.call("table small", name, n_remote=1, table=T.z2.data_ptr(), table_bytes=tab - 1)

    # the owner protocol at each of the six sites that check a claim
    for which, first, other in SITES:
        T.site("fresh context", which, h=T.fresh.h)
        getattr(T, first)()
        T.take_scratch()
        T.site("scratch used in between", which)
        getattr(T, first)((H, 64) if first == "dinf_start" else T.win_other)
        T.site("first phase on 128 x 64", which)
        getattr(T, other)()
        T.site("after another owner's first phase", which)
    T.dinf_start()
    T.site("another angle raster", "dt_dev_dinf_accumulate", angle=T.acc.data_ptr())
    T.site("another weight raster", "dt_dev_dinf_accumulate", w=Z)
    T.site("another frac_bits", "dt_dev_dinf_accumulate", frac_bits=11)
    T.fh_local()
    T.site("no second region", "dt_dev_flowacc_finish_flowhand_local_w")

    # empty rasters: DT_OK, and whether the call drops a claim made before it (the matching finish tells)
    for name in shaped + ["dt_dev_synth_dem"]:
        T.fa_local()
        T.call("0 x 0", name, H=0, W=0, h=0, w=0, work=Z, work_bytes=1 << 20, qwork=Z, qbytes=1 << 20)
        T.site("the claim after %s at 0 x 0" % name, "dt_dev_flowacc_finish_w")
    st = (T.t.ctx.status(), T.fresh.status())
    T.t.ctx.sync()
    T.fresh.sync()
    T.fresh.close()
    return T.rows, st


@pytest.fixture(scope="module")
def got():
    return table()


def test_every_answer_is_the_recorded_one(got):
    rows = got[0]
    assert [r[0] for r in rows] == [e[0] for e in EXPECTED], "the case list is not the recorded one"
    diff = ["%s: %r, recorded %r" % (r[0], r[1:], e[1:]) for r, e in zip(rows, EXPECTED) if tuple(r) != tuple(e)]
    assert not diff, "\n".join(diff)


def test_the_table_leaves_the_contexts_clean(got):
    assert got[1] == (0, 0)


def test_the_recorded_table_is_one_of_refusals():
    """outside the set-ups, the empty rasters and dt_dev_dinf_accumulate_info (which asks for no shape), every case is
    a refusal: DT_EINVAL with a message"""
    for case, rc, msg in EXPECTED:
        if "0 x 0" in case or case == "dt_dev_dinf_accumulate_info: first phase on 128 x 64":
            continue
        assert rc == -1 and msg.startswith("invalid argument: "), case


# recorded on the parent commit (1b33c84), MI355X; not to be edited to fit
EXPECTED = [('dt_dev_slope_d8: hw: negative H', -1, 'invalid argument: negative raster shape'),
 ('dt_dev_slope_d8: hw: 2^31 cells',
  -1,
  'invalid argument: rasters of >= 2^31 cells must be tiled (one tile per GPU)'),
 ('dt_dev_drainage: ws: negative H', -1, 'invalid argument: negative raster shape'),
 ('dt_dev_drainage: ws: 2^31 cells', -1, 'invalid argument: raster of 2^31 cells or more'),
 ('dt_dev_drainage: ws: px nan', -1, 'invalid argument: px must be finite and > 0'),
 ('dt_dev_drainage: ws: px inf', -1, 'invalid argument: px must be finite and > 0'),
 ('dt_dev_drainage: ws: px 0.0', -1, 'invalid argument: px must be finite and > 0'),
 ('dt_dev_stream_order: so: negative H', -1, 'invalid argument: negative raster shape'),
 ('dt_dev_stream_order: so: too large', -1, 'invalid argument: raster too large'),
 ('dt_dev_stream_order: so: 2^31 cells pass the rule', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_d8_w: window: bad core shape', -1, 'invalid argument: bad core shape'),
 ('dt_dev_slope_d8_w: window: ld < W', -1, 'invalid argument: ld < W'),
 ('dt_dev_slope_d8_w: window: outside the global raster',
  -1,
  'invalid argument: core window outside the global raster'),
 ('dt_dev_slope_d8_w: window: negative halo', -1, 'invalid argument: negative halo'),
 ('dt_dev_slope_d8_w: window: inside a larger raster without a halo',
  -1,
  'invalid argument: a window inside a larger raster needs a halo of >= 1 cell'),
 ('dt_dev_condition_stage_m_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_condition_stage_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_emit_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_f64_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_lift_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_walk_route_f64_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_walk_route_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_walk_seed_f64_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_walk_seed_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_downslope_walk_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowacc_finish_flowhand_local_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowacc_finish_flowhand_local_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowacc_finish_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowacc_finish_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowacc_local_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowhand_finish_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowhand_finish_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowhand_gfi_finish_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowhand_gfi_finish_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowhand_local_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowhand_local_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_flowhand_zr64_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_hand_gfi_f64_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_hand_gfi_f64_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_slope_d8_f64_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_slope_d8_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_slope_twi_f64_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_slope_twi_f64_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_slope_twi_w: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_slope_twi_w_a64: window: NULL', -1, 'invalid argument: window is NULL'),
 ('dt_dev_condition_d8: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_condition_d8_async: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_condition_d8_f64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_condition_d8_f64_async: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_dinf_accumulate: NULL angle', -1, 'invalid argument: NULL raster'),
 ('dt_dev_dinf_direction: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_f64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_finish: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_lift: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_queue: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_drainage: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc_river: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc_river_flowhand_local: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc_river_flowhand_local_m: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc_river_flowhand_local_ms: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc_weighted: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowhand: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowhand_gfi: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_hand_gfi_f64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_inundate: NULL catch_', -1, 'invalid argument: NULL raster'),
 ('dt_dev_reach_catchments: NULL link', -1, 'invalid argument: NULL raster'),
 ('dt_dev_reach_channels: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_reach_tables: NULL catch_', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_d8: NULL dem', -1, 'invalid argument: dem is NULL'),
 ('dt_dev_slope_d8_f64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_d8_m: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_d8_ms: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_twi: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_twi_f64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_twi_fix: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_stream_order: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_upslope_length: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_condition_stage_m_w: NULL nsame', -1, 'invalid argument: the byte raster is missing'),
 ('dt_dev_downslope_emit_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_f64_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_lift_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_downslope_walk_route_f64_w: NULL dem', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_downslope_walk_route_w: NULL dem', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_downslope_walk_seed_f64_w: NULL dem', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_downslope_walk_seed_w: NULL dem', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_downslope_walk_w: NULL dem', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_flowacc_finish_flowhand_local_w: NULL fdr', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_flowacc_finish_flowhand_local_w_a64: NULL fdr', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_flowacc_finish_w: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc_finish_w_a64: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowacc_local_w: NULL fdr', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_flowhand_finish_w: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowhand_finish_w_a64: NULL fdr', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowhand_gfi_finish_w: NULL dem', -1, 'invalid argument: hand needs dem'),
 ('dt_dev_flowhand_gfi_finish_w_a64: NULL dem', -1, 'invalid argument: hand needs dem'),
 ('dt_dev_flowhand_local_w: NULL fdr', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_flowhand_local_w_a64: NULL fdr', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_flowhand_zr64_w: NULL dem', -1, 'invalid argument: NULL pointer'),
 ('dt_dev_hand_gfi_f64_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_hand_gfi_f64_w_a64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_d8_f64_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_d8_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_twi_f64_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_twi_f64_w_a64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_twi_w: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_slope_twi_w_a64: NULL dem', -1, 'invalid argument: NULL raster'),
 ('dt_dev_synth_dem: NULL out', -1, 'invalid argument: out is NULL'),
 ('dt_dev_slope_d8: no output', -1, 'invalid argument: no output requested'),
 ('dt_dev_synth_dem: bad shape', -1, 'invalid argument: bad shape'),
 ('dt_dev_flowhand: hand needs dem', -1, 'invalid argument: hand needs dem'),
 ('dt_dev_flowhand: a_river needs the accumulation', -1, 'invalid argument: a_river needs acc32'),
 ('dt_dev_flowhand_finish_w: hand needs dem', -1, 'invalid argument: hand needs dem'),
 ('dt_dev_flowhand_finish_w: a_river needs the accumulation',
  -1,
  'invalid argument: a_river needs the accumulation raster'),
 ('dt_dev_flowhand_finish_w_a64: hand needs dem', -1, 'invalid argument: hand needs dem'),
 ('dt_dev_flowhand_finish_w_a64: a_river needs the accumulation',
  -1,
  'invalid argument: a_river needs the accumulation raster'),
 ('dt_dev_flowhand_finish_w: incomplete rank-exit results', -1, 'invalid argument: incomplete rank-exit results'),
 ('dt_dev_flowhand_gfi_finish_w: incomplete rank-exit results', -1, 'invalid argument: incomplete rank-exit results'),
 ('dt_dev_flowhand_gfi_finish_w_a64: incomplete rank-exit results',
  -1,
  'invalid argument: incomplete rank-exit results'),
 ('dt_dev_flowhand_gfi_finish_w: fused: gfi NULL', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowhand_gfi: fused: gfi NULL', -1, 'invalid argument: NULL raster'),
 ('dt_dev_drainage: label requires pour', -1, 'invalid argument: label requires pour'),
 ('dt_dev_reach_catchments: catch needs idx', -1, 'invalid argument: catch needs idx with an element size of 4 or 8'),
 ('dt_dev_reach_catchments: catch needs idx: element size',
  -1,
  'invalid argument: catch needs idx with an element size of 4 or 8'),
 ('dt_dev_reach_catchments: negative capacity', -1, 'invalid argument: negative capacity'),
 ('dt_dev_reach_channels: reach count -1', -1, 'invalid argument: the number of reaches must lie in [0, 2^31)'),
 ('dt_dev_reach_tables: reach count -1', -1, 'invalid argument: the number of reaches must lie in [0, 2^31)'),
 ('dt_dev_inundate: reach count -1', -1, 'invalid argument: the number of reaches must lie in [0, 2^31)'),
 ('dt_dev_reach_channels: reach count 2147483648',
  -1,
  'invalid argument: the number of reaches must lie in [0, 2^31)'),
 ('dt_dev_reach_tables: reach count 2147483648', -1, 'invalid argument: the number of reaches must lie in [0, 2^31)'),
 ('dt_dev_inundate: reach count 2147483648', -1, 'invalid argument: the number of reaches must lie in [0, 2^31)'),
 ('dt_dev_reach_channels: NULL output', -1, 'invalid argument: NULL output'),
 ('dt_dev_reach_tables: NULL table', -1, 'invalid argument: NULL table'),
 ('dt_dev_reach_tables: hand_bytes 2', -1, "invalid argument: hand's element size must be 4 or 8"),
 ('dt_dev_inundate: hand_bytes 2', -1, "invalid argument: hand's element size must be 4 or 8"),
 ('dt_dev_reach_tables: stages: K 0', -1, 'invalid argument: 1..1024 stages per call'),
 ('dt_dev_reach_tables: stages: K 1025', -1, 'invalid argument: 1..1024 stages per call'),
 ('dt_dev_reach_tables: stages: NULL', -1, 'invalid argument: 1..1024 stages per call'),
 ('dt_dev_reach_tables: stages: nan', -1, 'invalid argument: stages must be finite and >= 0'),
 ('dt_dev_reach_tables: stages: negative', -1, 'invalid argument: stages must be finite and >= 0'),
 ('dt_dev_reach_tables: stages: not increasing',
  -1,
  'invalid argument: stages must be finite and strictly increasing'),
 ('dt_dev_reach_tables: stages: frac_bits too fine',
  -1,
  'invalid argument: frac_bits is too fine: N * rint(max(stages[K - 1], 1) * 2^frac_bits) exceeds 2^52'),
 ('dt_dev_reach_tables: frac_bits 2201', -1, 'invalid argument: frac_bits out of range'),
 ('dt_dev_reach_tables: frac_bits -2201', -1, 'invalid argument: frac_bits out of range'),
 ('dt_dev_flowacc_weighted: frac_bits 2201', -1, 'invalid argument: frac_bits out of range'),
 ('dt_dev_flowacc_weighted: frac_bits -2201', -1, 'invalid argument: frac_bits out of range'),
 ('dt_dev_dinf_accumulate: frac_bits 2201', -1, 'invalid argument: frac_bits out of range'),
 ('dt_dev_dinf_accumulate: frac_bits -2201', -1, 'invalid argument: frac_bits out of range'),
 ('dt_dev_dinf_accumulate: rounds 0',
  -1,
  'invalid argument: rounds must lie in [1, 4096] (or [-4096, -1] to continue)'),
 ('dt_dev_dinf_accumulate: rounds 4097',
  -1,
  'invalid argument: rounds must lie in [1, 4096] (or [-4096, -1] to continue)'),
 ('dt_dev_dinf_accumulate: rounds -4097',
  -1,
  'invalid argument: rounds must lie in [1, 4096] (or [-4096, -1] to continue)'),
 ('dt_dev_flowacc_river_flowhand_local_m: the nodata mask is required',
  -1,
  'invalid argument: dem and the nodata mask are both required'),
 ('dt_dev_flowacc_river_flowhand_local_ms: marks NULL', -1, 'invalid argument: NULL raster'),
 ('dt_dev_flowhand_zr64_w: ring size -1', -1, 'invalid argument: bad ring size'),
 ('dt_dev_flowhand_zr64_w: ring size 509', -1, 'invalid argument: bad ring size'),
 ('dt_dev_downslope_walk_w: negative count', -1, 'invalid argument: negative count'),
 ('dt_dev_downslope_walk_route_w: negative count', -1, 'invalid argument: negative count'),
 ('dt_dev_downslope_walk_route_f64_w: negative count', -1, 'invalid argument: negative count'),
 ('dt_dev_downslope_walk_seed_w: negative count', -1, 'invalid argument: negative count'),
 ('dt_dev_downslope_walk_seed_f64_w: negative count', -1, 'invalid argument: negative count'),
 ('dt_dev_downslope_walk_route_w: layout: ty 0', -1, 'invalid argument: layout / counts missing'),
 ('dt_dev_downslope_walk_route_w: layout: counts NULL', -1, 'invalid argument: layout / counts missing'),
 ('dt_dev_downslope_walk_route_f64_w: layout: ty 0', -1, 'invalid argument: layout / counts missing'),
 ('dt_dev_downslope_walk_route_f64_w: layout: counts NULL', -1, 'invalid argument: layout / counts missing'),
 ('dt_dev_hand_gfi_f64_w: incomplete rank-exit results', -1, 'invalid argument: incomplete rank-exit results'),
 ('dt_dev_hand_gfi_f64_w: negative n_remote', -1, 'invalid argument: incomplete rank-exit results'),
 ('dt_dev_hand_gfi_f64_w_a64: incomplete rank-exit results', -1, 'invalid argument: incomplete rank-exit results'),
 ('dt_dev_hand_gfi_f64_w_a64: negative n_remote', -1, 'invalid argument: incomplete rank-exit results'),
 ('dt_dev_unique_extremes_f32: bad arguments', -1, 'invalid argument: bad arguments'),
 ('dt_dev_downslope_lift: work missing', -1, 'invalid argument: downslope workspace missing or too small'),
 ('dt_dev_downslope_lift: work small', -1, 'invalid argument: downslope workspace missing or too small'),
 ('dt_dev_downslope_queue: queue missing', -1, 'invalid argument: queue workspace missing or too small'),
 ('dt_dev_downslope_queue: queue small', -1, 'invalid argument: queue workspace missing or too small'),
 ('dt_dev_downslope_finish: queue missing', -1, 'invalid argument: queue workspace missing or too small'),
 ('dt_dev_downslope_finish: queue small', -1, 'invalid argument: queue workspace missing or too small'),
 ('dt_dev_downslope_finish: tables small', -1, 'invalid argument: tables workspace too small'),
 ('dt_dev_downslope_lift_w: work missing', -1, 'invalid argument: downslope workspace missing or too small'),
 ('dt_dev_downslope_lift_w: work small', -1, 'invalid argument: downslope workspace missing or too small'),
 ('dt_dev_downslope_emit_w: work small', -1, 'invalid argument: downslope workspace too small'),
 ('dt_dev_downslope_walk_w: work small', -1, 'invalid argument: downslope workspace too small'),
 ('dt_dev_downslope_walk_route_w: work small', -1, 'invalid argument: downslope workspace too small'),
 ('dt_dev_downslope_emit_w: walkers missing', -1, 'invalid argument: walker buffer missing or too small'),
 ('dt_dev_downslope_emit_w: walkers small', -1, 'invalid argument: walker buffer missing or too small'),
 ('dt_dev_hand_gfi_f64_w: table missing', -1, 'invalid argument: river-height table missing or too small'),
 ('dt_dev_hand_gfi_f64_w: table small', -1, 'invalid argument: river-height table missing or too small'),
 ('dt_dev_hand_gfi_f64_w_a64: table missing', -1, 'invalid argument: river-height table missing or too small'),
 ('dt_dev_hand_gfi_f64_w_a64: table small', -1, 'invalid argument: river-height table missing or too small'),
 ('dt_dev_flowacc_finish_w: fresh context',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_finish_w: scratch used in between',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_finish_w: first phase on 128 x 64',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ("dt_dev_flowacc_finish_w: after another owner's first phase",
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_finish_flowhand_local_w: fresh context',
  -1,
  'invalid argument: dt_dev_flowacc_finish_flowhand_local_w without a matching dt_dev_flowacc_local_w on this '
  "context (another call has used the context's scratch in between)"),
 ('dt_dev_flowacc_finish_flowhand_local_w: scratch used in between',
  -1,
  'invalid argument: dt_dev_flowacc_finish_flowhand_local_w without a matching dt_dev_flowacc_local_w on this '
  "context (another call has used the context's scratch in between)"),
 ('dt_dev_flowacc_finish_flowhand_local_w: first phase on 128 x 64',
  -1,
  'invalid argument: dt_dev_flowacc_finish_flowhand_local_w without a matching dt_dev_flowacc_local_w on this '
  "context (another call has used the context's scratch in between)"),
 ("dt_dev_flowacc_finish_flowhand_local_w: after another owner's first phase",
  -1,
  'invalid argument: dt_dev_flowacc_finish_flowhand_local_w without a matching dt_dev_flowacc_local_w on this '
  "context (another call has used the context's scratch in between)"),
 ('dt_dev_flowhand_finish_w: fresh context',
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ('dt_dev_flowhand_finish_w: scratch used in between',
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ('dt_dev_flowhand_finish_w: first phase on 128 x 64',
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ("dt_dev_flowhand_finish_w: after another owner's first phase",
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ('dt_dev_flowhand_gfi_finish_w: fresh context',
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ('dt_dev_flowhand_gfi_finish_w: scratch used in between',
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ('dt_dev_flowhand_gfi_finish_w: first phase on 128 x 64',
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ("dt_dev_flowhand_gfi_finish_w: after another owner's first phase",
  -1,
  'invalid argument: flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call has '
  "used the context's scratch in between)"),
 ('dt_dev_dinf_accumulate: fresh context',
  -1,
  'invalid argument: dt_dev_dinf_accumulate cannot continue: no accumulation of this shape was started on this '
  "context (or another call has used the context's scratch in between)"),
 ('dt_dev_dinf_accumulate: scratch used in between',
  -1,
  'invalid argument: dt_dev_dinf_accumulate cannot continue: no accumulation of this shape was started on this '
  "context (or another call has used the context's scratch in between)"),
 ('dt_dev_dinf_accumulate: first phase on 128 x 64',
  -1,
  'invalid argument: dt_dev_dinf_accumulate cannot continue: no accumulation of this shape was started on this '
  "context (or another call has used the context's scratch in between)"),
 ("dt_dev_dinf_accumulate: after another owner's first phase",
  -1,
  'invalid argument: dt_dev_dinf_accumulate cannot continue: no accumulation of this shape was started on this '
  "context (or another call has used the context's scratch in between)"),
 ('dt_dev_dinf_accumulate_info: fresh context',
  -1,
  "invalid argument: no D-infinity accumulation on this context (or another call has used the context's scratch "
  'since)'),
 ('dt_dev_dinf_accumulate_info: scratch used in between',
  -1,
  "invalid argument: no D-infinity accumulation on this context (or another call has used the context's scratch "
  'since)'),
 ('dt_dev_dinf_accumulate_info: first phase on 128 x 64', 0, ''),
 ("dt_dev_dinf_accumulate_info: after another owner's first phase",
  -1,
  "invalid argument: no D-infinity accumulation on this context (or another call has used the context's scratch "
  'since)'),
 ('dt_dev_dinf_accumulate: another angle raster',
  -1,
  'invalid argument: dt_dev_dinf_accumulate continues with another angle raster, weight raster or frac_bits than it '
  'was started with'),
 ('dt_dev_dinf_accumulate: another weight raster',
  -1,
  'invalid argument: dt_dev_dinf_accumulate continues with another angle raster, weight raster or frac_bits than it '
  'was started with'),
 ('dt_dev_dinf_accumulate: another frac_bits',
  -1,
  'invalid argument: dt_dev_dinf_accumulate continues with another angle raster, weight raster or frac_bits than it '
  'was started with'),
 ('dt_dev_flowacc_finish_flowhand_local_w: no second region',
  -1,
  'invalid argument: dt_dev_flowacc_finish_flowhand_local_w without a matching dt_dev_flowacc_local_w on this '
  "context (another call has used the context's scratch in between)"),
 ('dt_dev_condition_d8: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_condition_d8 at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_condition_d8_async: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_condition_d8_async at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_condition_d8_f64: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_condition_d8_f64 at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_condition_d8_f64_async: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_condition_d8_f64_async at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_dinf_accumulate: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_dinf_accumulate at 0 x 0', 0, ''),
 ('dt_dev_dinf_direction: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_dinf_direction at 0 x 0', 0, ''),
 ('dt_dev_downslope: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_downslope at 0 x 0', 0, ''),
 ('dt_dev_downslope_f64: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_downslope_f64 at 0 x 0', 0, ''),
 ('dt_dev_downslope_finish: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_downslope_finish at 0 x 0', 0, ''),
 ('dt_dev_downslope_lift: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_downslope_lift at 0 x 0', 0, ''),
 ('dt_dev_downslope_queue: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_downslope_queue at 0 x 0', 0, ''),
 ('dt_dev_drainage: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_drainage at 0 x 0', 0, ''),
 ('dt_dev_flowacc: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowacc at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_river: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowacc_river at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_river_flowhand_local: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowacc_river_flowhand_local at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_river_flowhand_local_m: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowacc_river_flowhand_local_m at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_river_flowhand_local_ms: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowacc_river_flowhand_local_ms at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowacc_weighted: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowacc_weighted at 0 x 0', 0, ''),
 ('dt_dev_flowhand: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowhand at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_flowhand_gfi: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_flowhand_gfi at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_hand_gfi_f64: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_hand_gfi_f64 at 0 x 0', 0, ''),
 ('dt_dev_inundate: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_inundate at 0 x 0', 0, ''),
 ('dt_dev_reach_catchments: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_reach_catchments at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_reach_channels: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_reach_channels at 0 x 0', 0, ''),
 ('dt_dev_reach_tables: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_reach_tables at 0 x 0',
  -1,
  'invalid argument: dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another call '
  "has used the context's scratch in between)"),
 ('dt_dev_slope_d8: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_slope_d8 at 0 x 0', 0, ''),
 ('dt_dev_slope_d8_f64: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_slope_d8_f64 at 0 x 0', 0, ''),
 ('dt_dev_slope_d8_m: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_slope_d8_m at 0 x 0', 0, ''),
 ('dt_dev_slope_d8_ms: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_slope_d8_ms at 0 x 0', 0, ''),
 ('dt_dev_slope_twi: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_slope_twi at 0 x 0', 0, ''),
 ('dt_dev_slope_twi_f64: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_slope_twi_f64 at 0 x 0', 0, ''),
 ('dt_dev_slope_twi_fix: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_slope_twi_fix at 0 x 0', 0, ''),
 ('dt_dev_stream_order: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_stream_order at 0 x 0', 0, ''),
 ('dt_dev_upslope_length: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_upslope_length at 0 x 0', 0, ''),
 ('dt_dev_synth_dem: 0 x 0', 0, ''),
 ('dt_dev_flowacc_finish_w: the claim after dt_dev_synth_dem at 0 x 0', 0, '')]
