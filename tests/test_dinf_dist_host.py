"""CPU (not gpu): descriptools_amd.dinf.distance_down / hand refuse bad arguments with ValueError before any library
call, the C entry is declared and bound, and the numpy reference the GPU tests compare against
(tests/_dinf_dist_ref.py) has the properties the definition promises: what reaches under the strict edge rule reaches
under the lenient one with the same bits, min <= ave <= max and h <= s, |v| <= s up to rounding, and on D8 angles the
three statistics agree and the horizontal distance is the length of the D8 walk."""
import functools
import math
import os

import numpy as np
import pytest

import oracle
from descriptools_amd import _lib, dinf

import _dinf_dist_ref as DR
import _dinf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 1e-12  # relative: a convex combination in floating point may overshoot an end point by an ulp


# ---- argument checks ----------------------------------------------------------------------------------------------
def _ang(shape=(5, 6)):
    return np.full(shape, -1, np.float32)


def _riv(shape=(5, 6)):
    return np.zeros(shape, np.int8)


def test_value_errors_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", no_library)
    dem = np.arange(30, dtype=np.float32).reshape(5, 6)
    for f in (lambda **kw: dinf.distance_down(kw.pop("angle", _ang()), kw.pop("river", _riv()), kw.pop("px", PX), **kw),
              lambda **kw: dinf.hand(kw.pop("angle", _ang()), kw.pop("river", _riv()), kw.pop("dem", dem),
                                     kw.pop("px", PX), **kw)):
        with pytest.raises(ValueError, match="2-D"):
            f(angle=_ang().reshape(-1))
        with pytest.raises(ValueError, match="2-D"):
            f(river=_riv().reshape(-1))
        with pytest.raises(ValueError, match="shape"):
            f(river=_riv((6, 5)))
        with pytest.raises(ValueError, match="shape"):
            f(dem=np.zeros((5, 7), np.float32))
        with pytest.raises(ValueError, match="2-D"):
            f(dem=np.zeros(30, np.float32))
        for px in (0.0, -1.0, float("nan"), float("inf"), "wide", True, "a"):
            with pytest.raises(ValueError, match="px"):
                f(px=px)
        for stat in ("mean", "AVE", 0, None):
            with pytest.raises(ValueError, match="stat"):
                f(stat=stat)
        with pytest.raises(ValueError, match="float32"):
            f(dem=dem.astype(np.float64) + 1e-9)
        for lim in (-1, 1.5, True, "2"):
            with pytest.raises(ValueError, match="_visit_limit"):
                f(_visit_limit=lim)
        for bad in (np.nan, -2.0, -0.5, -99.0, 6.2831860, np.inf, -np.inf):
            a = _ang()
            a[2, 3] = bad
            with pytest.raises(ValueError, match="angle"):
                f(angle=a)
        big = np.broadcast_to(np.float32(-1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
        with pytest.raises(ValueError, match="2\\^31"):
            f(angle=big)
    with pytest.raises(ValueError, match="dem"):
        dinf.hand(_ang(), _riv(), None, PX)


def test_entry_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    assert "int dt_dinf_distance_down(const float *angle, const int8_t *river, const float *dem, int64_t H, int64_t W," in hdr
    res, args = _lib._SIGS["dt_dinf_distance_down"]
    assert res is _lib.ci and len(args) == 13
    assert args[:3] == [_lib.c_f32p, _lib.c_i8p, _lib.c_f32p] and args[5] is _lib.f64
    assert args[6:9] == [_lib.ci] * 3 and args[9:12] == [_lib.c_f64p] * 3 and args[12] is _lib.c_i64p
    assert not any(n.startswith("dt_dev_dinf_distance") for n in _lib._SIGS)
    kh = open(os.path.join(ROOT, "descriptools_amd", "csrc", "dt_kernels.h")).read()
    assert "size_t dt_dinf_distance_scratch(int64_t H, int64_t W);" in kh and "dt_launch_dinf_distance(hipStream_t s" in kh


def test_alias_module_and_tuple():
    import descriptools.dinf
    assert descriptools.dinf.distance_down is dinf.distance_down and descriptools.dinf.hand is dinf.hand
    d = dinf.DinfDistance(1, None, 3)
    assert isinstance(d, tuple) and d.horizontal == 1 and d.vertical is None and d.surface == 3 and tuple(d) == (1, None, 3)


# ---- the reference's own properties --------------------------------------------------------------------------------
terrain, ref, PX = DR.terrain, DR.ref, DR.PX
SEEDS = [(65, 63, 0, 50), (130, 257, 2, 100), (200, 333, 2, 200)]


def _bits(m):
    return m.view(np.int64)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("surface", ["raw", "cond"])
def test_strict_reaches_implies_lenient_with_the_same_bits(seed, surface):
    for stat in DR.STATS:
        strict, lenient = ref(*seed, surface, stat, True), ref(*seed, surface, stat, False)
        m = strict[0] != -100
        assert m.any() and (lenient[0][m] != -100).all()
        for a, b in zip(strict, lenient):
            assert np.array_equal(_bits(a)[m], _bits(b)[m])
        a = terrain(*seed)[surface][0]
        assert ((strict[0] == -100) | (a != -100)).all() and (lenient[0][a == -100] == -100).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("surface", ["raw", "cond"])
@pytest.mark.parametrize("check_edges", [True, False])
def test_order_of_statistics_and_measures(seed, surface, check_edges):
    lo, av, hi = (ref(*seed, surface, stat, check_edges) for stat in ("min", "ave", "max"))
    m = av[0] != -100
    assert np.array_equal(m, lo[0] != -100) and np.array_equal(m, hi[0] != -100), "the mask does not depend on stat"
    for k in range(3):  # min <= ave <= max cell by cell, in every measure
        a, b, c = lo[k][m], av[k][m], hi[k][m]
        tol = SLACK * np.maximum(np.abs(a), np.abs(c))
        assert (a <= b + tol).all() and (b <= c + tol).all()
    for out in (lo, av, hi):
        h, v, s = (x[m] for x in out)
        assert (h >= 0).all() and (h <= s * (1 + SLACK)).all() and (np.abs(v) <= s * (1 + SLACK)).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_d8_angles_walk(seed):
    t = terrain(*seed)
    fdr, river, filled = t["fdr"], t["river"], t["cond"][1]
    a = R.d8_angles(fdr)
    a[filled <= -100] = -100
    outs = [DR.distance_down(a, river, PX, filled, stat, True) for stat in DR.STATS]
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert np.array_equal(_bits(x), _bits(y))
    h = outs[0][0]
    H, W = fdr.shape
    step = {code: (R.OCT_DY[k], R.OCT_DX[k], k & 1) for k, code in enumerate(R.OCT_CODE)}
    # a plain walk from EVERY cell down its D8 codes; a cell already walked through answers for the rest of the path
    # (the walk from it is the same walk), so the whole raster costs one step per cell
    known = {}  # (y, x) -> (n_card, n_diag), or None when the walk does not end on a river cell

    def walk(y, x):
        trail, end = [], None
        cy, cx = y, x
        while True:
            if (cy, cx) in known:
                end = known[(cy, cx)]
                break
            if river[cy, cx] == 1:
                end = (0, 0)
                known[(cy, cx)] = end
                break
            code = int(fdr[cy, cx])
            if code not in step or len(trail) > H * W:
                break
            dy, dx, d = step[code]
            ny, nx = cy + dy, cx + dx
            if not (0 <= ny < H and 0 <= nx < W) or a[ny, nx] == -100:
                break
            trail.append((cy, cx, d))
            cy, cx = ny, nx
        if end is None and (cy, cx) not in known:
            known[(cy, cx)] = None
        for py, px_, d in reversed(trail):
            end = None if end is None else (end[0] + 1 - d, end[1] + d)
            known[(py, px_)] = end
        return known[(y, x)]

    checked = 0
    want = np.full((H, W), -100.0)
    for y in range(H):
        for x in range(W):
            if a[y, x] == -100:
                continue
            r = walk(y, x)
            if r is not None:
                want[y, x] = r[0] + r[1] * math.sqrt(2.0)
                checked += 1
    m = want != -100
    assert np.array_equal(m, h != -100), "the walk ends on a river cell exactly where the reference reaches"
    assert checked > H * W // 2
    np.testing.assert_allclose(h[m] / PX, want[m], rtol=1e-9, atol=0)


def test_small_cases_by_hand():
    # a row that flows east into a target; the cell beyond the target flows off the raster
    e = R.octant_angle(0)
    a = np.array([[e, e, e, e, e]], np.float32)
    river = np.array([[0, 0, 0, 1, 0]], np.int8)
    dem = np.array([[7, 5, 4, 1, 0]], np.float32)
    (h, v, s), x = DR.distance_down(a, river, 2.0, dem, full=True)
    assert h.tolist() == [[6.0, 4.0, 2.0, 0.0, -100.0]] and v.tolist() == [[6.0, 4.0, 3.0, 0.0, -100.0]]
    assert s[0, 2] == math.sqrt(4.0 + 9.0) and s[0, 1] == math.sqrt(4.0 + 9.0) + math.sqrt(4.0 + 1.0)
    assert x["state"].tolist() == [[1, 1, 1, 1, 2]]
    # two receivers: E a target, NE dead under the strict rule, the lenient rule takes the one term
    ang = np.float32(0.3)
    a = np.array([[-1, -1], [ang, e]], np.float32)
    river = np.array([[0, 0], [0, 1]], np.int8)
    h1 = DR.distance_down(a, river, 2.0, check_edges=True)[0]
    h0 = DR.distance_down(a, river, 2.0, check_edges=False)[0]
    assert h1[1, 0] == -100 and h0[1, 0] == 2.0 and h0[0, 1] == -100
    # both receivers targets: the share-weighted average of px and px * sqrt(2)
    river = np.array([[0, 1], [0, 1]], np.int8)
    _, _, p2 = R.decode(a)
    w1 = float(p2[1, 0])
    want = ((2.0 ** 30 - w1) * 2.0 + w1 * (2.0 * DR.SQRT2)) * 2.0 ** -30
    for ce in (True, False):
        assert DR.distance_down(a, river, 2.0, check_edges=ce)[0][1, 0] == want
    assert DR.distance_down(a, river, 2.0, stat="min")[0][1, 0] == 2.0
    assert DR.distance_down(a, river, 2.0, stat="max")[0][1, 0] == 2.0 * DR.SQRT2
    # a two-cell cycle never settles
    a = np.array([[e, R.octant_angle(4), R.octant_angle(4)]], np.float32)
    (h, _, _), x = DR.distance_down(a, np.zeros((1, 3), np.int8), 1.0, full=True)
    assert (h == -100).all() and x["state"].tolist() == [[0, 0, 0]]
