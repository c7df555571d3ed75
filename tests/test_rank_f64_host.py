"""CPU: the rank-tiled step on float64 heights (tiling.RankTile(heights="float64")) -- what is refused before any device
work, and the C ABI of its windowed entry points."""
import numpy as np
import pytest

NEW = {"dt_dev_slope_d8_f64_w", "dt_dev_slope_twi_f64_w", "dt_dev_slope_twi_f64_w_a64", "dt_dev_downslope_f64_w",
       "dt_dev_downslope_walk_seed_f64_w", "dt_dev_downslope_walk_route_f64_w", "dt_dev_flowhand_zr64_w",
       "dt_dev_rank_solve_flowhand_f64", "dt_hand_f64_table_bytes", "dt_dev_hand_gfi_f64_w",
       "dt_dev_hand_gfi_f64_w_a64"}


@pytest.fixture
def no_context(monkeypatch):
    from descriptools_amd import device

    def refuse(*a, **k):
        raise AssertionError("a Context was created before the arguments were checked")
    monkeypatch.setattr(device, "Context", refuse)


def _wide_tile():
    """a float64 RankTile as far as the refusals look at it: no device behind it"""
    from descriptools_amd import tiling
    t = tiling.RankTile.__new__(tiling.RankTile)
    t.wide = True
    return t


def test_constructor_refuses_before_device_work(no_context):
    from descriptools_amd import tiling
    layout = tiling.Layout([64, 64], [64, 64])
    with pytest.raises(ValueError, match="heights must be one of"):
        tiling.RankTile(layout, 0, heights="float16")
    with pytest.raises(ValueError, match="long_walks is float32-only"):
        tiling.RankTile(layout, 0, heights="float64", long_walks=True)
    with pytest.raises(ValueError, match="emit_walkers is float32-only"):
        tiling.RankTile(layout, 0, heights="float64", emit_walkers=True)


def test_conditioning_and_evaluation_are_refused_on_float64_tiles():
    from descriptools_amd import tiling
    layout = tiling.Layout([64], [64])
    t = _wide_tile()
    for call in (t.cond_alloc, lambda: t.cond_stage(1), t.cond_d8, t.cond_flag,
                 lambda: tiling.condition_ranks([t], None, any), lambda: tiling.condition_local([t], layout),
                 lambda: tiling.condition_rank(t, layout)):
        with pytest.raises(ValueError, match="float32-only"):
            call()
    with pytest.raises(ValueError, match="evaluate_rank is float32-only"):
        tiling.evaluate_rank(t, None, None)
    with pytest.raises(ValueError, match="float32-only"):
        tiling.simulate([t], layout)


def test_float64_hand_row_extends_the_float32_row():
    from descriptools_amd import tiling
    assert tiling.FH_FIELDS_F64[:len(tiling.FH_FIELDS)] == tiling.FH_FIELDS
    name, dt, off = tiling.FH_FIELDS_F64[-1]
    assert (name, dt) == ("zr64", "float64") and off % 8 == 0
    assert off + 8 == tiling.FH_ROW_BYTES_F64 and off >= tiling.FH_ROW_BYTES


def test_rank_f64_entry_points_are_declared_and_exported():
    from test_cabi import header_symbols
    from descriptools_amd import _lib
    assert NEW <= set(header_symbols()) and NEW <= set(_lib.exported_symbols())
    L = _lib.lib()
    for n in (0, 1, 100, 5000):
        b = int(L.dt_hand_f64_table_bytes(n))
        slots = b // 16
        assert b % 16 == 0 and slots & (slots - 1) == 0 and slots >= 2 * n
    assert int(L.dt_hand_f64_table_bytes(-1)) == -1
