"""GPU (-m gpu): HAND's tile and node passes on adversarial direction fields (tests/_hand_fields.py) against the
oracle, through every form the product runs them in: the host op under both flow implementations, the device tier
(fused GFI or not, with and without A_river, outputs off the 16-byte grid), the resident chain on given codes (float32
and float64 heights: the fused accumulation + HAND tile pass with the river mask in registers) and logical ranks.

River index, HAND and A_river are compared by equality; the flow distance by equality where the path is made of one
kind of move, within rtol 1e-6 (test_gpu_parity.py's bar for this raster) where it mixes them; GFI and ln(hl/H) within
rtol 1e-5 / atol 1e-6 on the families whose accumulation is >= 0 everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from conftest import assert_float_close

import _hand_fields as F

pytestmark = pytest.mark.gpu

PX, N_GFI, B_GFI = F.PX, 0.4, 0.1
ALL = F.small_names() + F.HOP_NAMES
# the chain derives the river from the accumulation: fields that differ in the mask alone are one field to it
CHAIN = [n for n in F.small_names(shapes=F.BIG + ((512, 512),))
         if not n.startswith(("quirk_values", "quirk_corners", "quirk_all", "quirk_no"))]


def _compare(e, what, idx=None, fdist=None, hand=None, a_river=None, gfi=None, lnhlh=None):
    if idx is not None:
        assert np.array_equal(idx, e["idx"]), "%s: %d river indices differ" % (what, int((idx != e["idx"]).sum()))
    if fdist is not None:
        one = F.one_kind(e)
        assert np.array_equal(fdist[one], e["fdist"][one]), "%s: %d one-kind flow distances differ" % (
            what, int((fdist[one] != e["fdist"][one]).sum()))
        assert np.allclose(fdist[~one], e["fdist"][~one], rtol=1e-6, atol=0), what + ": flow distance"
    if hand is not None:
        assert np.array_equal(hand, e["hand"]), "%s: %d HAND cells differ" % (what, int((hand != e["hand"]).sum()))
    if a_river is not None:
        assert np.array_equal(a_river, e["a_river"]), what + ": A_river"
    if gfi is not None and (e["fac"] >= 0).all():
        assert_float_close(gfi, _gfi(e)[0], rtol=1e-5, atol=1e-6, what=what + ": gfi")
        assert_float_close(lnhlh, _gfi(e)[1], rtol=1e-5, atol=1e-6, what=what + ": lnhlh")


def _gfi(e):
    if "gfi" not in e:
        e["gfi"] = (oracle.gfi(e["hand"], e["fac"], e["idx"], N_GFI, B_GFI, PX),
                    oracle.lnhlh(e["hand"], e["fac"], N_GFI, B_GFI, PX))
    return e["gfi"]


# ---- forms 1 and 2: the host op under both flow implementations --------------------------------------------
@pytest.mark.parametrize("impl", [2, 1])
@pytest.mark.parametrize("name", ALL)
def test_host_op(name, impl):
    from descriptools_amd import _lib, flowhand
    f, e = F.field(name), F.answer(name)
    _lib.check(_lib.lib().dt_set_flow_impl(impl))
    try:
        fd, idx, hand = flowhand.flow_hand_index(f.dem, f.fdr, f.river, PX)
    finally:
        _lib.check(_lib.lib().dt_set_flow_impl(2))
    _compare(e, "%s impl %d" % (name, impl), idx=idx, fdist=fd, hand=hand)


# ---- form 3: the device tier ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_device_tier(name):
    """dt_dev_flowhand_gfi and dt_dev_flowhand on device buffers, with and without A_river, and once with every
    output 4 bytes off its block's start, so that the last tile pass writes cell by cell instead of 16 bytes at a
    time"""
    from descriptools_amd import _lib, device
    L = _lib.lib()
    f, e = F.field(name), F.answer(name)
    H, W = f.fdr.shape
    n = H * W
    ctx = device.Context()
    bufs = []

    def dev(a):
        bufs.append(ctx.to_device(a))
        return bufs[-1]
    try:
        dem, fdr, river = dev(f.dem), dev(f.fdr), dev(f.river)
        fac = dev(e["fac"].astype(np.int32))
        out = {k: ctx.empty((n + 4,), dt) for k, dt in (("fdist", np.float32), ("idx", np.int32), ("hand", np.float32),
                                                        ("a_river", np.int32), ("gfi", np.float32),
                                                        ("lnhlh", np.float32))}
        bufs += list(out.values())
        for fused, want_ar, off in ((True, True, 0), (True, False, 0), (False, True, 0), (False, False, 0),
                                    (True, True, 1), (False, True, 1)):
            for b in out.values():
                b.copy_from(np.full(n + 4, 77, b.dtype))
            p = {k: C.c_void_p(b.ptr.value + 4 * off) for k, b in out.items()}
            ar = p["a_river"] if want_ar else None
            if fused:
                _lib.check(L.dt_dev_flowhand_gfi(ctx.h, dem.ptr, fdr.ptr, river.ptr, fac.ptr, H, W, PX, N_GFI, B_GFI,
                                                 p["fdist"], p["idx"], p["hand"], ar, p["gfi"], p["lnhlh"]))
            else:
                _lib.check(L.dt_dev_flowhand(ctx.h, dem.ptr, fdr.ptr, river.ptr, fac.ptr if want_ar else None, H, W,
                                             PX, p["fdist"], p["idx"], p["hand"], ar))
            ctx.sync()
            got = {k: b.to_host() for k, b in out.items()}
            used = [k for k in out if (fused or k not in ("gfi", "lnhlh")) and (want_ar or k != "a_river")]
            for k, a in got.items():  # nothing written outside the raster, nor into a raster that was not asked for
                outside = np.concatenate([a[:off], a[off + n:]]) if k in used else a
                assert (outside == 77).all(), "%s: stray write" % k
            r = {k: got[k][off:off + n].reshape(H, W) for k in used}
            _compare(e, "%s fused=%d a_river=%d offset=%d" % (name, fused, want_ar, off), idx=r["idx"],
                     fdist=r["fdist"], hand=r["hand"], a_river=r.get("a_river"), gfi=r.get("gfi"),
                     lnhlh=r.get("lnhlh"))
    finally:
        for b in bufs:
            b.free()
        ctx.close()


# ---- forms 4 and 5: the resident chain on given codes -----------------------------------------------------------
def _chain_once(dem, fdr, heights="float32", **kw):
    from descriptools_amd import chain, device
    H, W = fdr.shape
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=PX, n_gfi=N_GFI, b=B_GFI, overlap=False, tune_placement=False,
                     external_fdr=True, heights=heights, **kw)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float64 if heights == "float64" else np.float32))
    try:
        ch.buf["fdr"].copy_from(fdr)
        ch.run(d.ptr)
        ctx.sync()
        ch.check_status()
        return {k: ch.buf[k].to_host() for k in ("fac", "river", "idx", "fdist", "hand", "a_river", "gfi", "lnhlh")}
    finally:
        d.free()
        ch.free()
        ctx.close()


@functools.lru_cache(maxsize=4)
def _chain_answer(name, thr):
    f = _chain_field(name)
    fac = oracle.flowacc(f.fdr, f.dem)
    river = (fac > thr).astype(np.int8)
    e = F.expected(f.dem, f.fdr, river, PX, fac=fac)
    e["river"] = river
    return e


@functools.lru_cache(maxsize=2)
def _chain_field(name):
    if name.startswith("hop_a_noriver"):
        return F.hop_a(river=False, flipped=name.endswith("_w"))
    return F.field(name)


def _check_chain(name, thr, out, e, hand=True):
    what = "%s thr %d" % (name, thr)
    assert np.array_equal(out["fac"], e["fac"]), what + ": fac"
    assert np.array_equal(out["river"], e["river"]), what + ": river"
    _compare(e, what, idx=out["idx"], fdist=out["fdist"], hand=out["hand"] if hand else None,
             a_river=out["a_river"], gfi=out["gfi"] if hand else None, lnhlh=out["lnhlh"] if hand else None)


@pytest.mark.parametrize("thr", [0, 300, 10 ** 9])
@pytest.mark.parametrize("name", CHAIN)
def test_chain_on_given_codes(name, thr):
    """Chain(external_fdr=True): width 320 and 512 take the fused accumulation + HAND tile pass (the river mask
    acc > thr in registers), width 300 the two separate kernels; nearly every valid cell is river, some are, none is.
    With and without slope_rad (the two set-ups of the chain)."""
    f, e = _chain_field(name), _chain_answer(name, thr)
    for rad in (True, False):
        _check_chain(name, thr, _chain_once(f.dem, f.fdr, river_threshold=thr, want_slope_rad=rad), e)


@pytest.mark.parametrize("name,thr", [(n, t) for n in ("hop_a_noriver_e", "hop_a_noriver_w")
                                      for t in (19998, 19999, 20000)])
def test_chain_river_starts_at_the_cap(name, thr):
    """the 20100-move zigzag with the river derived from its accumulation: it starts thr + 1 = 19999, 20000, 20001
    moves from the head, so the head resolves, resolves with exactly 20000 moves, is dead"""
    f, e = _chain_field(name), _chain_answer(name, thr)
    head = np.nonzero((e["fac"] == 0) & (f.fdr != 0))
    assert len(head[0]) == 1
    # (the river mask also takes the code-0 cell the path's last cell points at: accumulation 20101)
    assert (e["idx"][head][0] != -100) == (thr + 1 <= 20000) and e["river"].sum() == 20101 - thr
    if thr + 1 <= 20000:
        assert e["nd"][head][0] == thr + 1
    _check_chain(name, thr, _chain_once(f.dem, f.fdr, river_threshold=thr), e)


@pytest.mark.parametrize("name", F.small_names(["descending", "planted"], shapes=F.BIG))
def test_chain_on_given_codes_float64(name):
    """heights="float64": the same tile passes on the nodata proxy, HAND in float64"""
    f, e = _chain_field(name), _chain_answer(name, 300)
    dem64 = f.dem.astype(np.float64) + 1e-9 * np.arange(f.dem.size).reshape(f.dem.shape)
    out = _chain_once(dem64, f.fdr, heights="float64", river_threshold=300)
    _check_chain(name, 300, out, e, hand=False)
    hand = oracle.hand_f64(dem64, e["idx"])
    assert out["hand"].dtype == np.float64 and np.array_equal(out["hand"], hand)
    if (e["fac"] >= 0).all():
        assert_float_close(out["gfi"], oracle.gfi_f64h(hand, e["fac"], e["idx"], N_GFI, B_GFI, PX), rtol=1e-5,
                           atol=1e-6, what="gfi")
        assert_float_close(out["lnhlh"], oracle.lnhlh_f64h(hand, e["fac"], N_GFI, B_GFI, PX), rtol=1e-5, atol=1e-6,
                           what="lnhlh")


# ---- form 6: logical ranks ------------------------------------------------------------------------------------
def _through_ranks(f, e, heights, widths, what):
    """the field cut into ranks as test_gpu_tiling.test_move_cap_through_tiles_and_ranks does it: tile pass and node
    doubling per rank, the rank-level solve over the gathered rows, the last tile pass with the rank exits' results"""
    import torch
    from descriptools_amd import tiling
    layout = tiling.Layout(heights, widths)
    H, W = f.fdr.shape
    assert (layout.Hg, layout.Wg) == (H, W)
    h = tiling.HALO

    def padded(a, fill):
        p = np.full((H + 2 * h, W + 2 * h), fill, a.dtype)
        p[h:h + H, h:h + W] = a
        return p
    src = dict(fdr=padded(f.fdr, 0), river=padded(f.river, 0), dem=padded(f.dem, 1.0),
               fac=padded(e["fac"].astype(np.int32), 0))
    tiles = []
    try:
        for r in range(layout.size):
            t = tiling.RankTile(layout, r, device=0, px=PX, river_threshold=10, tune_placement=False)
            y0, x0 = layout.origin(r)
            for k, a in src.items():
                t.t[k].copy_(torch.as_tensor(a[y0:y0 + t.He, x0:x0 + t.We]))
            tiles.append(t)
        torch.cuda.synchronize()
        for t in tiles:
            t.fill_ring_codes()
            t.fh_local(sync=False)
        for t in tiles:
            t.ctx.sync()
        rows = torch.cat([t.fh_row for t in tiles])
        torch.cuda.synchronize()
        for t in tiles:
            t.fh_solve_finish(rows)
        for t in tiles:
            y0, x0 = layout.origin(t.rank)
            sl = (slice(y0, y0 + t.H), slice(x0, x0 + t.W))
            _compare({k: e[k][sl] for k in ("idx", "nc", "nd", "fdist", "hand", "a_river", "fac")},
                     "%s rank %d" % (what, t.rank), idx=t.host("idx"),
                     fdist=t.host("fdist"), hand=t.host("hand"), a_river=t.host("a_river"))
    finally:
        for t in tiles:
            t.free()


@functools.lru_cache(maxsize=1)
def _cap_mixed_small():
    (f,) = F.cap_mixed((256, 320))
    e = F.expected(f.dem, f.fdr, f.river, PX)
    ok = e["idx"] != -100
    assert (e["nc"] + e["nd"])[ok].max() == 20000 and (~ok & (f.fdr != 0)).sum() > 300
    return f, e


@pytest.mark.parametrize("name", ["planted-256x320", "cap_mixed-256x320"])
def test_ranks_2x2(name):
    f, e = _cap_mixed_small() if name.startswith("cap_mixed") else (F.field(name), F.answer(name))
    _through_ranks(f, e, [128, 128], [128, 192], name)


@pytest.mark.parametrize("name", ["hop_a20100_e", "hop_a20100_w", "hop_c_e", "hop_c_w"])
def test_ranks_every_move_a_rank_hop(name):
    """the rank border is the zigzag's own border: every move is a hop between ranks, the worst case for the rank
    level's launch budget and for the ghost hop's cap sum in the last tile pass"""
    _through_ranks(F.field(name), F.answer(name), [64, 64], [10112, 10112], name)
