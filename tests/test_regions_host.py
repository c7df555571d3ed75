"""CPU (not gpu): descriptools_amd.regions and reaches.inundate_connected refuse bad arguments with ValueError before any
library call and have no CPU fallback; the entries are declared, exported, bound and built; the alias module serves the
same objects; and the two forms of the numpy reference the GPU tests compare against (tests/_regions_ref.py) agree with
each other, with a case worked out by hand and (where it is installed) with scipy.ndimage.label's partition."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from descriptools_amd import reaches, regions

import _regions_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 17), (23, 1), (64, 64), (65, 63)]


def _masks(shape):
    H, W = shape
    p = dict(R.patterns(H, W))
    if H >= 8 and W >= 8:
        p["terrain"] = R.terrain_mask(oracle, H, W)[0]
        p["terrain_nodata"] = R.terrain_mask(oracle, H, W, nodata_pct=5)[0]
    return p


# ---- the reference's two forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_flood_equals_relax(shape, connectivity):
    for name, m in _masks(shape).items():
        f, r = R.flood(m, connectivity), R.relax(m, connectivity)
        assert f.dtype == r.dtype == np.int64 and f.tobytes() == r.tobytes(), name
        fg = m != 0
        assert np.array_equal(f == -100, ~fg), name
        flat = f.reshape(-1)
        assert (flat[f[fg]] == f[fg]).all() and (f[fg] <= np.flatnonzero(fg.reshape(-1))).all(), name
        s = R.sizes(f)
        assert s.sum() == sum(int(v) ** 2 for v in np.bincount(f[fg])) and (s[~fg] == 0).all(), name


@pytest.mark.parametrize("connectivity", [4, 8])
def test_partition_equals_scipy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    st = np.ones((3, 3), int) if connectivity == 8 else None
    for name, m in _masks((65, 63)).items():
        ours = R.flood(m, connectivity)
        theirs, n = ndi.label(m != 0, structure=st)
        fg = m != 0
        assert np.array_equal(theirs != 0, fg), name
        pairs = np.unique(np.stack([ours[fg], theirs[fg]]), axis=1)
        assert pairs.shape[1] == n == np.unique(ours[fg]).size, name  # one-to-one


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_pairs_the_kernels_unite_suffice(connectivity):
    """the unions of csrc/dt_regions.hip (tests/_regions_ref.pairing_model), made sequentially, give the reference's
    labels: random masks around the percolation thresholds at small tile edges, so that seams and tile corners are
    everywhere, and the patterns at the kernels' own edge"""
    rng = np.random.default_rng(3)
    for _ in range(120):
        H, W = (int(v) for v in rng.integers(1, 14, 2))
        tile = int(rng.integers(2, 6))
        m = (rng.random((H, W)) < rng.choice([0.3, 0.41, 0.5, 0.59, 0.8])).astype(np.uint8)
        assert np.array_equal(R.pairing_model(m, connectivity, tile), R.flood(m, connectivity)), (m, tile)
    for name, m in R.patterns(13, 11).items():
        assert np.array_equal(R.pairing_model(m, connectivity, 4), R.flood(m, connectivity)), name
    for name, m in R.patterns(65, 67).items():
        assert np.array_equal(R.pairing_model(m, connectivity, regions.TILE), R.flood(m, connectivity)), name


MASK = np.array([[1, 1, 0, 0, 1],
                 [0, 0, 1, 0, 1],
                 [1, 0, 0, 0, 0],
                 [1, 1, 0, 1, 1]], np.uint8)
_ = -100
LABEL8 = [[0, 0, _, _, 4], [_, _, 0, _, 4], [10, _, _, _, _], [10, 10, _, 18, 18]]
SIZE8 = [[3, 3, 0, 0, 2], [0, 0, 3, 0, 2], [3, 0, 0, 0, 0], [3, 3, 0, 2, 2]]
LABEL4 = [[0, 0, _, _, 4], [_, _, 7, _, 4], [10, _, _, _, _], [10, 10, _, 18, 18]]  # (0, 1) and (1, 2) touch diagonally
SIZE4 = [[2, 2, 0, 0, 2], [0, 0, 1, 0, 2], [3, 0, 0, 0, 0], [3, 3, 0, 2, 2]]


def test_by_hand():
    for form in (R.flood, R.relax):
        for cn, lab, size in ((8, LABEL8, SIZE8), (4, LABEL4, SIZE4)):
            got = form(MASK, cn)
            assert got.dtype == np.int64 and np.array_equal(got, lab), (form.__name__, cn)
            assert np.array_equal(R.sizes(got), size)
    seeds = np.zeros_like(MASK)
    seeds[1, 2] = 1   # the diagonal cell
    seeds[2, 2] = 1   # on background: seeds nothing
    assert np.array_equal(R.connected(MASK, seeds, 8), np.isin(LABEL8, [0]).astype(np.uint8))
    assert np.array_equal(R.connected(MASK, seeds, 4), np.isin(LABEL4, [7]).astype(np.uint8))
    assert np.array_equal(R.connected(MASK, seeds, 4, min_cells=2), np.zeros_like(MASK))
    assert np.array_equal(R.sieve(MASK, 3, 8), np.isin(LABEL8, [0, 10]).astype(np.uint8))
    assert np.array_equal(R.sieve(MASK, 3, 4), np.isin(LABEL4, [10]).astype(np.uint8))
    assert R.sieve(MASK, 1).dtype == np.uint8 and np.array_equal(R.sieve(MASK, 1), MASK)


def test_serpentine_size_in_closed_form():
    for H, W in ((1, 1), (2, 5), (7, 4), (65, 63), (64, 64)):
        m = R.serpentine(H, W)
        assert int(m.sum()) == R.serpentine_cells(H, W)
        for cn in (4, 8):
            assert (R.flood(m, cn)[m != 0] == 0).all()


# ---- argument checks ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    from descriptools_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def _calls(mask, seeds=None, **kw):
    """every public function on the mask (seeds default to the mask)"""
    sd = mask if seeds is None else seeds
    yield lambda: regions.label(mask, **kw)
    yield lambda: regions.label(mask, sizes=True, **kw)
    yield lambda: regions.connected(mask, sd, **kw)
    yield lambda: regions.sieve(mask, 2, **kw)


def test_value_errors_before_any_library_call(no_library):
    mask = np.zeros((5, 6), np.uint8)
    for bad in (mask.reshape(-1), mask.reshape(5, 6, 1), np.uint8(1)):
        for call in _calls(bad):
            with pytest.raises(ValueError, match="2-D"):
                call()
    for other in (np.zeros((6, 5), np.uint8), np.zeros((5, 7), bool), np.zeros(30, np.uint8)):
        with pytest.raises(ValueError, match="2-D|shape"):
            regions.connected(mask, other)
    for dt in (np.float32, np.float64, np.float16, np.complex64, object):
        for call in _calls(np.zeros((5, 6), dt)):
            with pytest.raises(ValueError, match="dtype"):
                call()
        with pytest.raises(ValueError, match="dtype"):
            regions.connected(mask, np.zeros((5, 6), dt))
    for cn in (0, 1, 6, -8, 4.0, 8.0, "8", None, True):
        for call in _calls(mask, connectivity=cn):
            with pytest.raises(ValueError, match="connectivity"):
                call()
    for mc in (0, -1, 1.0, 2.5, "3", None, True, False, np.bool_(True)):
        with pytest.raises(ValueError, match="min_cells"):
            regions.sieve(mask, mc)
        with pytest.raises(ValueError, match="min_cells"):
            regions.connected(mask, mask, min_cells=mc)


def test_2_31_cells_refused(no_library):
    big = np.broadcast_to(np.uint8(0), (1 << 16, 1 << 15))  # 2^31 cells, 1 byte of memory
    for call in _calls(big):
        with pytest.raises(ValueError, match="2\\^31"):
            call()


def test_inundate_connected_refuses_before_the_library(no_library):
    cat = np.zeros((5, 7), np.int32)
    hand = np.zeros((5, 7), np.float32)
    river = np.zeros((5, 7), np.int8)
    stage = np.array([1.0])
    ok = dict(catchment=cat, hand=hand, stage=stage, river=river)
    bad = [("catchment", cat.astype(np.float32)), ("catchment", cat.reshape(-1)), ("hand", hand[:, :6]),
           ("hand", hand.astype(np.complex64)), ("stage", np.zeros((2, 2))), ("stage", "high"),
           ("river", river[:4]), ("river", river.reshape(-1)), ("river", river.astype(np.float32)),
           ("connectivity", 6), ("connectivity", 8.0), ("connectivity", True), ("connectivity", None)]
    for name, value in bad:
        with pytest.raises(ValueError):
            reaches.inundate_connected(**dict(ok, **{name: value}))
    big = np.broadcast_to(np.int32(0), (1 << 16, 1 << 15))
    with pytest.raises(ValueError, match="2\\^31"):
        reaches.inundate_connected(big, np.broadcast_to(np.float32(0), big.shape), stage,
                                   np.broadcast_to(np.int8(0), big.shape))


# ---- the entries and their plumbing -----------------------------------------------------------------------------------
def test_entries_are_declared_exported_bound_and_built():
    from descriptools_amd import _lib, build
    L = _lib
    assert "dt_regions.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "dt_regions.hip"))
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"#define\s+DT_REGIONS_TILE\s+%d\b" % regions.TILE, header)
    want = {
        "dt_regions_label": [L.c_u8p, L.i64, L.i64, L.ci, L.c_i64p, L.c_i64p],
        "dt_regions_select": [L.c_u8p, L.c_u8p, L.i64, L.i64, L.ci, L.i64, L.c_u8p],
        "dt_inundate_connected": [L.c_i32p, L.vp, L.ci, L.c_f64p, L.c_i8p, L.i64, L.i64, L.i64, L.ci, L.c_f32p],
        "dt_dev_regions_label": [L.vp, L.vp, L.i64, L.i64, L.ci, L.vp, L.vp],
        "dt_dev_regions_select": [L.vp, L.vp, L.vp, L.i64, L.i64, L.ci, L.i64, L.vp],
        "dt_dev_inundate_connected": [L.vp, L.vp, L.vp, L.ci, L.vp, L.vp, L.i64, L.i64, L.i64, L.ci, L.vp],
    }
    so = ctypes.CDLL(build.build())
    for name, args in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        res, got = _lib._SIGS[name]
        assert res is ctypes.c_int and got == args, name
        assert hasattr(so, name) and hasattr(_lib.lib(), name), name
    capi = open(os.path.join(build.CSRC, "dt_capi.hip")).read()
    for name in ("dt_dev_regions_label", "dt_dev_regions_select", "dt_dev_inundate_connected"):
        assert re.search(r'^extern "C" int %s\(' % name, capi, re.M), name


def test_alias_module():
    import descriptools.regions
    for name in ("label", "connected", "sieve", "Regions", "TILE"):
        assert getattr(descriptools.regions, name) is getattr(regions, name), name
    r = regions.Regions(1, 2)
    assert isinstance(r, tuple) and r.label == 1 and r.size == 2
    assert regions.TILE == 64


def test_module_docstring_carries_the_definitions():
    doc = regions.__doc__
    for phrase in ("mask != 0", "connectivity=8", "smallest flat index", "-100 on background", "0 on background",
                   "size[c] >= min_cells", "seeds nothing"):
        assert phrase in doc, phrase


def test_no_cpu_fallback_without_gpu():
    from descriptools_amd import _lib
    if _lib.lib().dt_device_count() > 0:
        pytest.skip("a GPU is visible")
    m = np.ones((8, 8), np.uint8)
    for call in _calls(m):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):
        reaches.inundate_connected(np.zeros((8, 8), np.int32), np.zeros((8, 8), np.float32), [1.0],
                                   np.ones((8, 8), np.int8))
