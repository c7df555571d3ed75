"""CPU: the interface of the float64 height tier (chain.Chain / run_host / flowdir.d8 `heights=`) -- what is refused
before anything reaches a GPU, how "auto" picks the tier, and the C ABI of the tier."""
import numpy as np
import pytest

from conftest import golden


def test_default_tier_still_refuses_float64_heights():
    from descriptools_amd import chain, flowdir
    dem64 = golden("f64")["dem"]
    for call in (lambda: chain.run_host(dem64, 10.0), lambda: flowdir.d8(dem64, 10.0),
                 lambda: chain.run_host(dem64, 10.0, heights="float32"),
                 lambda: flowdir.d8(dem64, 10.0, heights="float32")):
        with pytest.raises(ValueError, match="not exactly representable in float32"):
            call()


def test_bogus_tier_and_out_of_scope_combinations_raise():
    from descriptools_amd import chain, flowdir
    dem = np.zeros((8, 8), np.float32)
    for call in (lambda: chain.run_host(dem, 10.0, heights="bogus"), lambda: flowdir.d8(dem, 10.0, heights="bogus"),
                 lambda: chain.Chain(8, 8, heights="bogus"), lambda: chain.Chain(8, 8, heights="auto")):
        with pytest.raises(ValueError, match="heights must be one of"):
            call()
    with pytest.raises(ValueError, match="condition=True"):
        chain.Chain(8, 8, heights="float64", condition=True)
    for lw in (True, "auto"):
        with pytest.raises(ValueError, match="long_walks"):
            chain.Chain(8, 8, heights="float64", long_walks=lw)


def test_auto_picks_the_tier():
    from descriptools_amd import _lib
    rng = np.random.default_rng(1)
    a32 = (rng.random((20, 30)) * 3000).astype(np.float32)
    d, wide = _lib.dem_tier(a32.astype(np.float64), "auto")
    assert not wide and d.dtype == np.float32 and np.array_equal(d, a32)
    dem64 = golden("f64")["dem"]
    d, wide = _lib.dem_tier(dem64, "auto")
    assert wide and d.dtype == np.float64 and np.array_equal(d, dem64)
    d, wide = _lib.dem_tier(a32, "float64")  # explicit: always the float64 tier
    assert wide and d.dtype == np.float64 and np.array_equal(d, a32.astype(np.float64))
    d, wide = _lib.dem_tier(np.full((4, 4), 2 ** 24 + 1, np.int32), "auto")
    assert wide and d[0, 0] == 2 ** 24 + 1
    with pytest.raises(ValueError, match="float64 cannot represent"):
        _lib.dem_tier(np.full((4, 4), 2 ** 53 + 1, np.int64), "float64")


def test_float64_entry_points_are_declared_and_bound():
    from test_cabi import header_symbols
    from descriptools_amd import _lib
    new = {"dt_d8_f64", "dt_dev_slope_d8_f64", "dt_dev_slope_twi_f64", "dt_dev_downslope_f64", "dt_dev_hand_gfi_f64"}
    assert new <= set(header_symbols()) and new <= set(_lib.exported_symbols())


def test_float64_step_is_a_separate_op_list():
    from descriptools_amd import chain
    assert [o[0] for o in chain.OPS] == ["d8", "downslope", "flowacc_flowhand_local", "slope_twi", "flowhand_gfi_finish"]
    assert [o[0] for o in chain.OPS_F64] == ["d8", "downslope", "flowacc_flowhand_local", "slope_twi",
                                             "flowhand_finish", "hand_gfi"]


def test_numpy_d8_restatement_matches_the_float32_oracle():
    """the test-side float64 D8 restatement gives the oracle's codes on float32 heights (where both are exact)"""
    import oracle
    from test_gpu_chain_f64 import d8_f64_np
    for seed, nod in ((2, 0), (4, 5)):
        d32 = oracle.synth_dem(seed, 256, 256, 10, 20, 90, 130, nod)
        assert np.array_equal(d8_f64_np(d32, 10.0), oracle.slope_d8(d32, 10.0)[1])
