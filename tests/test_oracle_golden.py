"""CPU (not gpu): the oracle (oracle/dt_oracle.c) against the golden vectors generated from the
reference's unmodified source (oracle/gen_golden.py) -- this is what pins the oracle."""
import numpy as np
import pytest

import oracle
from conftest import assert_float_close, golden, load_example

CASES = ["syn_a", "syn_b", "syn_c", "ex_river", "ex_head", "ex_edge"]


@pytest.mark.parametrize("name", CASES)
def test_slope(name):
    g = golden(name)
    sl, _ = oracle.slope_d8(g["dem"].astype(np.float32), float(g["px"]))
    assert np.array_equal(sl, g["slope"]), "slope must be bit-identical (one f32 rounding)"


@pytest.mark.parametrize("name", CASES)
def test_twi(name):
    g = golden(name)
    ti, mti = oracle.twi(g["fac"], g["slope_rad"], float(g["px"]), float(g["n_top"]))
    assert_float_close(ti, g["ti"], rtol=1e-6, what="ti")
    assert_float_close(mti, g["mti"], rtol=1e-6, atol=1e-7, what="mti")


@pytest.mark.parametrize("name", CASES)
def test_flowhand(name):
    g = golden(name)
    fd, idx, hand = oracle.flowhand(g["dem"].astype(np.float32), g["fdr"], g["river"], float(g["px"]))
    assert np.array_equal(idx, g["idx"])
    assert np.array_equal(fd, g["fdist"]), "sequential f64 sum: bit-identical"
    assert np.array_equal(hand, g["hand"].astype(np.float32))
    # the fast propagation used for large rasters agrees with the literal walk
    idx2, nc, nd = oracle.flowhand_fast(g["fdr"], g["river"])
    assert np.array_equal(idx2, idx)
    px = float(g["px"])
    d2 = np.where(idx2 != -100, nc * px + nd * (px * np.sqrt(2.0)), -100.0)
    assert_float_close(d2.astype(np.float32), fd, rtol=2e-7, what="count-form distance")


@pytest.mark.parametrize("name", CASES)
def test_gfi_lnhlh(name):
    g = golden(name)
    hand = g["hand"].astype(np.float32)
    out = oracle.gfi(hand, g["fac"], g["idx"], float(g["n_gfi"]), float(g["b"]), float(g["px"]))
    assert_float_close(out, g["gfi"], rtol=1e-6, atol=1e-7, what="gfi")
    out = oracle.lnhlh(hand, g["fac"], float(g["n_gfi"]), float(g["b"]), float(g["px"]))
    assert_float_close(out, g["lnhlh"], rtol=1e-6, atol=1e-7, what="lnhlh")


@pytest.mark.parametrize("name", CASES)
def test_downslope(name):
    g = golden(name)
    out = oracle.downslope(g["dem"].astype(np.float32), g["fdr"], float(g["px"]), float(g["dz"]))
    ref = g["down"]
    # valid-DEM pits (fdr == 0): the reference computes 0/0 (NaN under numpy, ZeroDivisionError
    # under real Numba -- SURVEY 2.3: undefined); the build defines the result as 0.
    pit = np.isnan(ref)
    assert (g["fdr"][pit] == 0).all()
    assert np.array_equal(out, np.where(pit, 0, ref))


def test_edge_flowhand():
    g = golden("edge")
    fd, idx, hand = oracle.flowhand(g["fh_dem"].astype(np.float32), g["fh_fdr"], g["fh_river"], 10.0)
    assert np.array_equal(idx, g["fh_idx"])
    assert np.array_equal(fd, g["fh_fdist"])
    assert np.array_equal(hand, g["fh_hand"].astype(np.float32))
    assert (idx == -100).sum() > 10 and (idx != -100).sum() > 10
    idx2, _, _ = oracle.flowhand_fast(g["fh_fdr"], g["fh_river"])
    assert np.array_equal(idx2, idx)


def test_edge_cap_20000():
    g = golden("edge")
    W = int(g["cap_W"])
    fdr = np.ones((1, W), np.uint8)
    river = np.zeros((1, W), np.int8)
    river[0, W - 1] = 1
    dem = np.full((1, W), 5, np.float32)
    fd, idx, _ = oracle.flowhand(dem, fdr, river, 10.0)
    sel = g["cap_sel"]
    assert np.array_equal(idx[0, sel], g["cap_idx"])
    assert np.array_equal(fd[0, sel], g["cap_fdist"])
    # exactly 20000 moves is valid, 20001 is not (flowhand.py:834-837)
    assert idx[0, W - 1 - 20000] == W - 1 and idx[0, W - 1 - 20001] == -100
    idx2, nc, nd = oracle.flowhand_fast(fdr, river)
    assert np.array_equal(idx2, idx)


def test_edge_diag():
    g = golden("edge")
    n = int(g["diag_n"])
    fdr = np.full((n, n), 2, np.uint8)
    river = np.zeros((n, n), np.int8)
    river[n - 1, n - 1] = 1
    fd, idx, _ = oracle.flowhand(np.full((n, n), 5, np.float32), fdr, river, 12.5)
    sel = g["diag_sel"]
    assert np.array_equal(idx.reshape(-1)[sel], g["diag_idx"])
    assert np.array_equal(fd.reshape(-1)[sel], g["diag_fdist"])


def test_edge_downslope():
    g = golden("edge")
    out = oracle.downslope(g["ds_dem"].astype(np.float32), g["ds_fdr"], 10.0, 5.0)
    assert np.array_equal(out, g["ds_out"])
    out = oracle.downslope(g["dcap_dem"].astype(np.float32), np.ones(g["dcap_dem"].shape, np.uint8), 10.0, 5.0)
    assert np.array_equal(out[0, g["dcap_sel"]], g["dcap_out"])


def test_edge_pointwise():
    g = golden("edge")
    ti, mti = oracle.twi(g["pw_fac"], g["pw_slr"], 12.5, 0.1)
    assert_float_close(ti, g["pw_ti"], rtol=1e-6, what="ti")
    assert_float_close(mti, g["pw_mti"], rtol=1e-6, what="mti")
    hand = g["pw_hand"].astype(np.float32)
    assert_float_close(oracle.gfi(hand, g["pw_fac"], g["pw_idx"], 0.4, 0.1, 12.5), g["pw_gfi"], rtol=1e-6)
    assert_float_close(oracle.lnhlh(hand, g["pw_fac"], 0.4, 0.1, 12.5), g["pw_lnhlh"], rtol=1e-6)


def test_eval_counts():
    g = golden("eval")
    for k in range(3):
        under = str(g["e%d_under" % k]) == "under"
        desc, flood = g["e%d_desc" % k], g["e%d_flood" % k]
        th = float(g["e%d_th" % k])
        counts = oracle.confusion_multi(desc, flood, [th, 0.25, 0.5], under)
        ref = np.bincount(g["e%d_class" % k].reshape(-1).astype(np.int64), minlength=4)
        assert np.array_equal(counts[0], ref)
        assert counts[0, 3] / (counts[0, 2] + counts[0, 3]) == float(g["e%d_c" % k])
        assert counts[0, 3] / (counts[0, 3] + counts[0, 2] + counts[0, 1]) == float(g["e%d_f" % k])


def test_flowacc_vs_bundled_fac():
    """N2 convention check: Kahn accumulation over 12_fdr.tif equals 12_fac.tif on
    >= 98 % of valid cells and every mismatch has fac > acc (inflow from outside the clip)."""
    dem, fdr, fac, _, _, _ = load_example()
    acc = oracle.flowacc(fdr, dem.astype(np.float32))
    valid = dem != -100
    same = (acc == fac) & valid
    assert same.sum() / valid.sum() > 0.98
    mism = valid & ~same
    assert (fac[mism] > acc[mism]).all()


def test_d8_vs_bundled_fdr():
    """N1 rule check: on cells with a strictly lower neighbour, first-max-in-scan-
    order D8 agrees with the externally produced 12_fdr.tif on > 97 %."""
    dem, fdr, _, _, _, _ = load_example()
    sl, d8 = oracle.slope_d8(dem.astype(np.float32), 12.5)
    has_lower = (sl > 0) & (dem != -100)
    inner = np.zeros_like(has_lower)
    inner[1:-1, 1:-1] = True
    m = has_lower & inner
    assert (d8[m] == fdr[m]).mean() > 0.97


def test_synth_dem_properties():
    for seed in (1, 2, 3):
        dem = oracle.synth_dem(seed, 512, 640)
        assert (dem[1:, :] < dem[:-1, :]).all(), "every cell's S neighbour is strictly lower"
        u = dem * 256.0
        assert np.array_equal(u, np.round(u)) and dem.max() < 65536
        # tile-local generation: any window equals the same window of the full raster
        win = oracle.synth_dem(seed, 512, 640, 100, 37, 50, 61)
        assert np.array_equal(win, dem[100:150, 37:98])
        _, fdr = oracle.slope_d8(dem, 10.0)
        assert (fdr != 0).all()


def test_example_known_answer_oracle():
    """The reference's KAT through the oracle: HAND -> calibration counts -> class map equals
    Example/output/hand_class.tif and the full-size reference outputs (example_full.npz)."""
    dem, fdr, fac, river, flood, klass = load_example()
    g = golden("example_full")
    idx, nc, nd = oracle.flowhand_fast(fdr, river)
    assert np.array_equal(idx, g["idx"].astype(np.int64))
    d32 = dem.astype(np.float32).reshape(-1)
    hand = np.where((d32 != -100) & (idx.reshape(-1) != -100), d32 - d32[idx.reshape(-1)], -100)
    hand = np.where((hand < 0) & (hand != -100), 0, hand).reshape(dem.shape)
    assert np.array_equal(hand.astype(np.int16), g["hand"])
    desc = np.where(hand == -100, np.nan, (hand - float(g["mn"])) / (float(g["mx"]) - float(g["mn"])))
    desc[0, 0] = np.nan
    counts = oracle.confusion_multi(np.nan_to_num(desc, nan=-7.0), flood, [float(g["th"])], True)
    # nodata was mapped to -7 and desc[0] == -7 marks it as the nodata value (evaluation.py:111)
    assert np.array_equal(counts[0], g["counts"])
    assert np.array_equal(np.bincount(klass.reshape(-1).astype(np.int64), minlength=4), g["counts"])


# ------------------------------------------------------------------------------------------
# Non-finite heights (tests/golden/nonfinite*.npz, oracle/gen_golden.py nonfinite): NaN, +inf, -inf and finite
# heights below the sentinel on the border, in the interior and touching one another.  The reference under IEEE math.

def _nonfinite_pits(g):
    """downslope: the reference's 0/0 at valid-height pits (fdr == 0) is defined as 0 by the build; its
    NaN at a NaN or +inf start cell is kept (dt_oracle.c, dt_oracle_downslope)."""
    dem, ref = g["dem"], g["down"]
    start = np.isnan(dem) | np.isposinf(dem)
    pit = np.isnan(ref) & ~start
    assert (g["fdr"][pit] == 0).all() and np.isnan(ref[start]).all()
    return np.where(pit, 0, ref)


def test_nonfinite_fixture_holds_the_special_values():
    for name in ("nonfinite", "nonfinite_f64"):
        dem = golden(name)["dem"]
        H, W = dem.shape
        nan = np.isnan(dem)
        for edge in (nan[0], nan[-1], nan[:, 0], nan[:, -1]):
            assert edge.any()
        assert nan[0, 0] and nan[-1, -1]
        assert np.isposinf(dem[1:-1, 1:-1]).any() and np.isposinf(dem[[0, -1]]).any()
        assert np.isneginf(dem).sum() >= 3 and (dem == -250).any() and (dem == -9999).any()
        nod = dem == -100
        near = np.zeros_like(nod)
        near[1:, :] |= nod[:-1, :]
        near[:-1, :] |= nod[1:, :]
        near[:, 1:] |= nod[:, :-1]
        near[:, :-1] |= nod[:, 1:]
        assert (nan & near).any()


def test_nonfinite_d8_and_flowacc():
    g = golden("nonfinite")
    dem = g["dem"]
    sl, fdr = oracle.slope_d8(dem, float(g["px"]))
    assert np.array_equal(sl, g["slope"])
    assert np.array_equal(fdr, g["fdr"])
    # NaN centre: slope 0, code 0 inside, the out-code on the border; +inf centre: slope inf and a code
    nan = np.isnan(dem)
    assert (sl[nan] == 0).all() and (fdr[1:-1, 1:-1][nan[1:-1, 1:-1]] == 0).all()
    assert (fdr[0][nan[0]] == 64).all() and (fdr[-1][nan[-1]] == 4).all()
    assert (fdr[1:-1, 0][nan[1:-1, 0]] == 16).all() and (fdr[1:-1, -1][nan[1:-1, -1]] == 1).all()
    assert np.isposinf(sl[np.isposinf(dem)]).all() and (fdr[np.isposinf(dem)] != 0).all()
    acc = oracle.flowacc(g["fdr"], dem)
    assert np.array_equal(acc, g["fac"])
    assert np.array_equal(acc == -100, dem <= -100)   # the nodata of accumulation is exactly dem <= -100


@pytest.mark.parametrize("name", ["nonfinite"])
def test_nonfinite_descriptors(name):
    g = golden(name)
    dem, px = g["dem"], float(g["px"])
    ti, mti = oracle.twi(g["fac"], g["slope_rad"], px, float(g["n_top"]))
    assert_float_close(ti, g["ti"], rtol=1e-6, what="ti")
    assert_float_close(mti, g["mti"], rtol=1e-6, atol=1e-7, what="mti")
    assert np.array_equal(np.isnan(ti), np.isnan(g["ti"])) and np.array_equal(np.isinf(ti), np.isinf(g["ti"]))
    fd, idx, hand = oracle.flowhand(dem, g["fdr"], g["river"], px)
    assert np.array_equal(idx, g["idx"])
    assert np.array_equal(fd, g["fdist"])
    assert np.array_equal(hand, g["hand"], equal_nan=True)
    idx2, _, _ = oracle.flowhand_fast(g["fdr"], g["river"])
    assert np.array_equal(idx2, idx)
    out = oracle.gfi(hand, g["fac"], g["idx"], float(g["n_gfi"]), float(g["b"]), px)
    assert_float_close(out, g["gfi"], rtol=1e-6, atol=1e-7, what="gfi")
    out = oracle.lnhlh(hand, g["fac"], float(g["n_gfi"]), float(g["b"]), px)
    assert_float_close(out, g["lnhlh"], rtol=1e-6, atol=1e-7, what="lnhlh")
    down = oracle.downslope(dem, g["fdr"], px, float(g["dz"]))
    assert np.array_equal(down, _nonfinite_pits(g), equal_nan=True)


def test_nonfinite_f64_descriptors():
    g = golden("nonfinite_f64")
    dem, px = g["dem"], float(g["px"])
    assert np.array_equal(oracle.slope_f64(dem, px), g["slope"])
    assert np.array_equal(oracle.hand_f64(dem, g["idx"]), g["hand"], equal_nan=True)
    assert np.array_equal(oracle.downslope_f64(dem, g["fdr"], px, float(g["dz"])), _nonfinite_pits(g),
                          equal_nan=True)
    assert_float_close(oracle.gfi_f64h(g["hand"], g["fac"], g["idx"], 0.4, 0.1, px), g["gfi"], rtol=1e-6,
                       what="gfi")
    assert_float_close(oracle.lnhlh_f64h(g["hand"], g["fac"], 0.4, 0.1, px), g["lnhlh"], rtol=1e-6, atol=1e-7,
                       what="lnhlh")
    # D8 of the float64 tier (the float32-rounded heights' codes are the fixture's inputs)
    _, fdr = oracle.slope_d8(dem.astype(np.float32), px)
    assert np.array_equal(fdr, g["fdr"])
    assert np.array_equal(oracle.flowacc(g["fdr"], dem.astype(np.float32)), g["fac"])


# ------------------------------------------------------------------------------------------
# Off the Example's parameters (tests/golden/params_*.npz, oracle/gen_golden.py params): pixel sizes whose products are
# inexact in float64 (30, 0.1, 1/3, 30.922..., 2500), exponents of one, a scale factor >= 1 and values of dz that
# float32 cannot hold -- the same assertions as above: integers, slope, HAND, flow distance and downslope bit for bit,
# the float descriptors through assert_float_close.
PARAM_FILES = ["params_syn_%d" % i for i in range(5)] + ["params_ex_%d" % i for i in range(5)]


def test_params_cover_the_pixel_sizes_and_sets():
    pxs, sets = set(), {}
    for name in PARAM_FILES:
        g = golden(name)
        pxs.add(float(g["px"]))
        for s in g["sets"]:
            sets.setdefault(tuple(g[str(s) + "__params"]), set()).add(float(g["px"]))
    assert pxs >= {30.0, 0.1, 1.0 / 3.0, 30.922080775909325, 2500.0}
    assert len(sets) >= 4 and all(len(v) >= 2 for v in sets.values())
    assert any(n_top == 1.0 and n_gfi == 1.0 for n_top, n_gfi, b, dz in sets)
    assert any(b >= 1.0 for n_top, n_gfi, b, dz in sets)
    assert any(float(np.float32(dz)) != dz for n_top, n_gfi, b, dz in sets)


@pytest.mark.parametrize("name", PARAM_FILES)
def test_params_against_the_reference(name):
    g = golden(name)
    dem, px = g["dem"].astype(np.float32), float(g["px"])
    assert np.array_equal(oracle.slope_d8(dem, px)[0], g["slope"]), "slope must be bit-identical"
    fd, idx, hand = oracle.flowhand(dem, g["fdr"], g["river"], px)
    assert np.array_equal(idx, g["idx"])
    assert np.array_equal(fd, g["fdist"]), "sequential f64 sum: bit-identical"
    assert np.array_equal(hand, g["hand"])
    for s in g["sets"]:
        n_top, n_gfi, b, dz = (float(v) for v in g[str(s) + "__params"])
        ref = {k: g["%s__%s" % (s, k)] for k in ("ti", "mti", "gfi", "lnhlh", "down")}
        ti, mti = oracle.twi(g["fac"], g["slope_rad"], px, n_top)
        assert_float_close(ti, ref["ti"], rtol=1e-6, what="ti")
        assert_float_close(mti, ref["mti"], rtol=1e-6, atol=1e-7, what="mti")
        assert_float_close(oracle.gfi(hand, g["fac"], g["idx"], n_gfi, b, px), ref["gfi"], rtol=1e-6, atol=1e-7,
                           what="gfi")
        assert_float_close(oracle.lnhlh(hand, g["fac"], n_gfi, b, px), ref["lnhlh"], rtol=1e-6, atol=1e-7,
                           what="lnhlh")
        pit = np.isnan(ref["down"])   # the reference's 0 / 0 at valid-DEM pits: defined as 0 (test_downslope)
        assert (g["fdr"][pit] == 0).all()
        assert np.array_equal(oracle.downslope(dem, g["fdr"], px, dz), np.where(pit, 0, ref["down"]))


def test_params_hard_cases_against_the_reference():
    """the hard-case rasters of tests/test_gpu_pixel_size.py, shrunk to golden size: the reference's own values on the
    cells where the product form of the slope and the count form of the walk's length round differently"""
    g = golden("params_hard")
    dem, px = g["planted_dem"], float(g["planted_px"])
    slope, fdr = oracle.slope_d8(dem, px)
    assert np.array_equal(fdr, g["planted_fdr"])
    # The golden values are the reference's on a float64 copy: they are those of the float32 raster where the height
    # differences are exact in float32 -- on the planted cells by construction, on every cell whose descents are exact
    # for the slope (the 50 m cells beside a planted drop of 24 bits are not).
    H, W = dem.shape
    p = np.pad(dem, 1, mode="edge")
    exact = np.ones((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            nb = p[dy:dy + H, dx:dx + W]
            d64 = dem.astype(np.float64) - nb.astype(np.float64)   # (a rise never sets the maximum, however rounded)
            exact &= (d64 <= 0) | ((dem - nb).astype(np.float64) == d64)
    ys, xs = g["planted_cells"].T
    assert exact[ys, xs].all() and exact.mean() > 0.8
    assert np.array_equal(slope[exact], g["planted_slope"][exact])
    for dz in (5.0, 0.3, 0.1):
        assert np.array_equal(oracle.downslope(dem, fdr, px, dz)[ys, xs], g["planted_down_%g" % dz][ys, xs])
    # the product form is NOT the reference on the planted cells (so the fixture does hold them)
    product = np.float32(np.float64(dem) * (100.0 / px))
    assert ((product != slope) & (fdr == 16)).sum() >= 12
    dem = g["long_dem"]
    for j in (0, 1):
        px, sel = float(g["long_px%d" % j]), g["long_sel%d" % j]
        assert np.array_equal(oracle.slope_d8(dem, px)[1], g["long_fdr%d" % j])
        down = oracle.downslope(dem, g["long_fdr%d" % j], px, 5.0).reshape(-1)[sel]
        assert np.array_equal(down, g["long_down%d" % j])
        # ... and the count form of the path length is not, on the cells picked for that (all cardinal: nd = 0)
        x = sel % dem.shape[1]
        row = dem.reshape(-1)
        count = np.empty(len(sel), np.float32)
        for i, (s, x0) in enumerate(zip(sel, x)):
            n = 0
            while np.float32(row[s] - row[s + n]) < 5.0 and x0 + n < dem.shape[1] - 1 and row[s + n + 1] != -100.0:
                n += 1
            count[i] = np.float32(np.float64(np.float32(row[s] - row[s + n])) / (px * n)) if n else 0.0
        assert (count != down).sum() >= min(8, int(g["long_divergent%d" % j]))
