"""CPU (not gpu): descriptools_amd.cost refuses bad arguments with ValueError before any library call; the reference of
its GPU tests (tests/_cost_ref.py) is the unique solution the definition claims -- a heap Dijkstra and a randomly ordered
tile relaxation agree to the bit; the absorption example leaves one cell without a back-link; the entries are declared,
exported, bound and built; the alias module imports."""
import ctypes
import os
import re

import numpy as np
import pytest

import _cost_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- argument checks ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    from descriptools_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def test_value_errors_before_any_library_call(no_library):
    from descriptools_amd import cost
    f = np.ones((5, 6), np.float32)
    s = np.zeros((5, 6), np.int8)
    for bad in (f.reshape(-1), f.reshape(5, 6, 1), np.float32(1)):
        with pytest.raises(ValueError, match="2-D"):
            cost.cost_distance(bad, s, 10.0)
        with pytest.raises(ValueError, match="2-D"):
            cost.cost_hand(bad, s, 10.0)
    for bad in (s.reshape(-1), s.reshape(5, 6, 1), np.int8(1)):
        with pytest.raises(ValueError, match="2-D"):
            cost.cost_distance(f, bad, 10.0)
        with pytest.raises(ValueError, match="2-D"):
            cost.cost_hand(f, bad, 10.0)
    for other in (np.zeros((6, 5), np.int8), np.zeros((5, 7), np.int8)):
        with pytest.raises(ValueError, match="shape"):
            cost.cost_distance(f, other, 10.0)
        with pytest.raises(ValueError, match="shape"):
            cost.cost_hand(f, other, 10.0)
        with pytest.raises(ValueError, match="shape"):
            cost.cost_hand(f, s, 10.0, friction=other.astype(np.float32))
    for px in (0.0, -1.0, float("nan"), float("inf"), None, True, "a"):
        with pytest.raises(ValueError, match="px"):
            cost.cost_distance(f, s, px)
        with pytest.raises(ValueError, match="px"):
            cost.cost_hand(f, s, px)
    for conn in (0, 6, 16, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            cost.cost_distance(f, s, 10.0, connectivity=conn)
        with pytest.raises(ValueError, match="connectivity"):
            cost.cost_hand(f, s, 10.0, connectivity=conn)
    with pytest.raises(ValueError, match="_visit_limit"):
        cost.cost_distance(f, s, 10.0, _visit_limit=-1)


def test_2_31_cells_refused(no_library):
    from descriptools_amd import cost
    big = np.broadcast_to(np.float32(1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
    src = np.broadcast_to(np.int8(0), big.shape)
    with pytest.raises(ValueError, match="2\\^31"):
        cost.cost_distance(big, src, 10.0)
    with pytest.raises(ValueError, match="2\\^31"):
        cost.cost_hand(big, src, 10.0)


# ---- the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_dijkstra_equals_a_randomly_ordered_tile_relaxation(kind):
    """the uniqueness claim: the greatest solution does not depend on the order or the tiling"""
    f, s = R.random_case((65, 63), kind, 7)
    A = R.dijkstra(f, s, 12.3)
    assert np.isfinite(A).sum() >= 0.7 * R.passable(f).sum()
    for tile, seed in ((16, 3), (64, 4)):
        B = R.tile_relaxation(f, s, 12.3, 8, tile, seed)
        assert np.array_equal(A.view(np.int64), B.view(np.int64)), (tile, seed)


def test_reference_by_hand():
    """a wall with one gap: the cost goes round it; ties take the first neighbour of the scan order"""
    f = np.ones((3, 5), np.float32)
    f[0:2, 2] = 0
    s = np.zeros((3, 5), np.int8)
    s[0, 0] = 1
    cost, indices, link, linkless, reached = R.reference(f, s, 2.0, 4)
    assert linkless == 0 and reached == 13
    assert cost[0, 4] == 2.0 * 8 and cost[0, 2] == -100 and indices[0, 2] == -100 and link[0, 2] == 0
    assert (indices[f > 0] == 0).all() and link[0, 0] == 0
    assert link[0, 1] == 16 and link[2, 2] == 16 and link[1, 3] == 4 and link[1, 0] == 64
    assert link[1, 1] == 64  # N and W tie: N comes first
    assert link[0, 4] == 16  # W and S tie: W comes first
    cost8 = R.reference(f, s, 2.0, 8)[0]
    assert cost8[2, 2] == 2.0 * R.SQRT2 + 2.0 * R.SQRT2  # two diagonal steps, one rounding per operation
    assert cost8[1, 1] == 2.0 * R.SQRT2


def test_absorption_example_leaves_one_linkless_cell():
    f = np.array([[1, 1e30, 1e-30, 1e-30]], np.float32)
    s = np.array([[1, 0, 0, 0]], np.int8)
    cost, indices, link, linkless, reached = R.reference(f, s, 1.0)
    assert linkless == 1 and reached == 4
    assert cost[0, 3] == cost[0, 2] and link[0, 3] == 0 and indices[0, 3] == -100
    assert list(link[0, :3]) == [0, 16, 16] and list(indices[0, :3]) == [0, 0, 0]


def test_serpentine_path():
    """the case of the multi-round test: every passable cell is reached, none is linkless, and the farthest cell's
    path winds through 135 tiles of 64 x 64"""
    f, s = R.serpentine()
    cost, indices, link, linkless, reached = R.reference(f, s, 1.0)
    assert linkless == 0 and reached == int(R.passable(f).sum())
    parent = R.backlinks(f, s, 1.0, 8, np.where(cost >= 0, cost, np.inf))[1]
    cells, entries = R.path_tile_entries(parent, int(np.argmax(cost)), 64)
    assert (cells, entries) == (8386, 135)


# ---- the entries and their plumbing ---------------------------------------------------------------------------------
def test_entries_are_declared_exported_bound_and_built():
    from descriptools_amd import _lib, build
    assert "dt_cost.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "dt_cost.hip"))
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    assert re.search(r"#define\s+DT_STATUS_NO_BACKLINK\s+256\b", header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+dt_cost_distance\s*\(\s*const\s+float\s*\*", header)
    assert re.search(r"\bint\s+dt_dev_cost_distance\s*\(\s*dt_ctx\s*\*", header)
    res, args = _lib._SIGS["dt_cost_distance"]
    assert res is ctypes.c_int
    assert args == [_lib.c_f32p, _lib.c_i8p, _lib.i64, _lib.i64, _lib.f64, _lib.ci, _lib.ci, _lib.c_f64p,
                    _lib.c_i64p, _lib.c_u8p, _lib.c_i64p]
    so = ctypes.CDLL(build.build())
    assert hasattr(so, "dt_cost_distance") and hasattr(so, "dt_dev_cost_distance")
    L = _lib.lib()
    # the device tier refuses a NULL context before anything else (tests/test_dev_tier_contract.py)
    assert L.dt_dev_cost_distance(None, None, None, 4, 4, 1.0, 8, 0, 1, None, None, None) == -1
    assert L.dt_last_error() == b"invalid argument: ctx is NULL"


def test_raise_on_status_knows_no_backlink():
    from descriptools_amd import device

    class Ctx(device.Context):
        def __init__(self, st):
            self._st = st

        def status(self):
            return self._st

    with pytest.raises(RuntimeError, match="DT_STATUS_NO_BACKLINK"):
        Ctx(256).raise_on_status()
    Ctx(0).raise_on_status()


def test_alias_module():
    import descriptools.cost as alias
    from descriptools_amd import cost
    assert alias.cost_distance is cost.cost_distance
    assert alias.cost_hand is cost.cost_hand
    assert alias.CostDistance is cost.CostDistance
    assert "cost_distance" in alias.__all__
