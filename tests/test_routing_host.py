"""descriptools_amd.routing on the host: every bad argument raises ValueError before a library call (no GPU needed: the
library is never reached), and the integer reference (tests/_routing_ref.py) gives three hand-worked 1 x 6 eastward
chains, one per transfer function, written out here as literals.  sink_capacity is built on watershed.drainage, which
runs on the GPU, so its check against a plain path walk carries the gpu mark."""
import numpy as np
import pytest

from descriptools_amd import routing

import _dinf_ref
import _mfd_ref
import _routing_ref as R

INF = float("inf")

# 1 x 6, every cell flows east, the last one off the raster; frac_bits = 0.  Worked by hand from the definition:
# T = w + what the western neighbour sends, O = f(T, p), R = T - O.
CHAINS = {
    # 9 * 0.5 = 4.5 -> 4 | 4 * 1 | (4 + 4) * 0.25 | 2 * 0 | 0 | 16 * 0.75
    "decay": dict(w=[9, 0, 4, 0, 0, 16], p=[0.5, 1, 0.25, 0, 0.5, 0.75],
                  inflow=[0, 4, 4, 2, 0, 0], load=[9, 4, 8, 2, 0, 16], outflow=[4, 4, 2, 0, 0, 12],
                  retained=[5, 0, 6, 2, 0, 4]),
    # 5 > 2 -> 3 | 1 + 3 <= 10 -> 0 | 0 | 7 > 3 -> 4 | 2 + 4 < inf -> 0 | C = rint(0.5) = 0: 1 -> 1
    "retain": dict(w=[5, 1, 0, 7, 2, 1], p=[2, 10, 0, 3, INF, 0.5],
                   inflow=[0, 3, 0, 0, 4, 0], load=[5, 4, 0, 7, 6, 1], outflow=[3, 0, 0, 4, 0, 1],
                   retained=[2, 4, 0, 3, 6, 0]),
    # min(5, 2) | min(1 + 2, 10) | min(3, 0) | min(7, 3) | min(2 + 3, inf) | C = rint(1.5) = 2: min(1 + 5, 2)
    "limit": dict(w=[5, 1, 0, 7, 2, 1], p=[2, 10, 0, 3, INF, 1.5],
                  inflow=[0, 2, 3, 0, 3, 5], load=[5, 3, 3, 7, 5, 6], outflow=[2, 3, 0, 3, 5, 2],
                  retained=[3, 0, 3, 4, 0, 4]),
}


def chain_inputs(transfer):
    """-> (fdr uint8[1, 6], weights float64, param float64, {output: float64[1, 6]})"""
    c = CHAINS[transfer]
    want = {k: np.array([c[k]], np.float64) for k in R.OUTPUTS}
    return np.full((1, 6), 1, np.uint8), np.array([c["w"]], np.float64), np.array([c["p"]], np.float64), want


@pytest.mark.parametrize("transfer", ["decay", "retain", "limit"])
def test_reference_on_the_hand_worked_chains(transfer):
    fdr, w, p, want = chain_inputs(transfer)
    for flow in (_mfd_ref.d8_shares(fdr), _dinf_ref.d8_angles(fdr)):
        got, x = R.route(flow, p, transfer, w, 0, full=True)
        for k in R.OUTPUTS:
            assert np.array_equal(got[k], want[k]), (transfer, k, got[k])
        # what the chain's cells keep and what its last cell sends off the raster is what was put in
        assert int(x["q"].sum()) == int((x["T"] - x["O"]).sum()) + x["left"]
        assert x["left"] == CHAINS[transfer]["outflow"][-1]
        for T, O, Q in zip(x["T"], x["O"], R.quantise_param(transfer, p, 0)[0]):
            assert int(O) == R.transfer_exact(transfer, T, Q)


def test_reference_identities_are_the_accumulations():
    rng = np.random.default_rng(3)
    dem = rng.integers(0, 60, (23, 31)).astype(np.float32)
    dem[5, 7] = dem[20, 2] = -100
    shares = _mfd_ref.flow_shares(dem, 1)
    angle = _dinf_ref.flow_direction(dem, 10.0)[0]
    w = rng.uniform(0, 4, dem.shape)
    for transfer, ident in (("decay", 1.0), ("retain", 0.0), ("limit", INF)):
        p = np.full(dem.shape, ident)
        assert np.array_equal(R.route(shares, p, transfer, w)["inflow"], _mfd_ref.accumulate(shares, w))
        assert np.array_equal(R.route(angle, p, transfer, w)["inflow"], _dinf_ref.accumulate(angle, w))
        out = R.route(shares, p, transfer, w)
        assert np.array_equal(out["outflow"], out["load"]) and (out["retained"][out["load"] != -100] == 0).all()


def test_reference_bad_parameter_is_the_identity():
    fdr, w, p, _ = chain_inputs("retain")
    s = _mfd_ref.d8_shares(fdr)
    for transfer, ident, bads in (("decay", 1.0, (np.nan, -0.5, 1.5)), ("retain", 0.0, (np.nan, -1.0)),
                                  ("limit", INF, (np.nan, -1.0))):
        base = np.clip(p, 0, 1) if transfer == "decay" else p
        for bad in bads:
            a, b = base.copy(), base.copy()
            a[0, 2], b[0, 2] = bad, ident
            got, x = R.route(s, a, transfer, w, 0, full=True)
            want = R.route(s, b, transfer, w, 0)
            assert x["bad"].sum() == 1 and x["bad"][2]
            for k in R.OUTPUTS:
                assert np.array_equal(got[k], want[k])


# ---- every bad argument is refused before the library is reached ----------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from descriptools_amd import _lib

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", boom)


def test_bad_arguments_raise_before_any_library_call(no_library):
    fdr = np.full((4, 5), 1, np.uint8)
    shares = _mfd_ref.d8_shares(fdr)
    angle = _dinf_ref.d8_angles(fdr)
    ok = np.full((4, 5), 0.5)
    bad_calls = [
        lambda: routing.route(fdr, ok, "spill"),                                  # transfer
        lambda: routing.route(fdr, ok, None),
        lambda: routing.route(fdr, ok, "decay", outputs="outflow"),              # outputs
        lambda: routing.route(fdr, ok, "decay", outputs=()),
        lambda: routing.route(fdr, ok, "decay", outputs=("outflow", "outflow")),
        lambda: routing.route(fdr, ok, "decay", outputs=("flux",)),
        lambda: routing.route(fdr.astype(np.int32), ok, "decay"),                 # flow
        lambda: routing.route(fdr.astype(np.float64), ok, "decay"),
        lambda: routing.route(shares.astype(np.int16), ok, "decay"),
        lambda: routing.route(shares[:, :, :7], ok, "decay"),
        lambda: routing.route(fdr[0], ok[0], "decay"),
        lambda: routing.route(ok, ok, "decay"),
        lambda: routing.route(ok.astype(np.float32) * 20, ok, "decay"),           # an angle beyond 2 pi
        lambda: routing.route(np.full((4, 5), np.nan, np.float32), ok, "decay"),
        lambda: routing.route(fdr, ok[:3], "decay"),                              # param
        lambda: routing.route(fdr, ok.astype(complex), "decay"),
        lambda: routing.route(fdr, ok * 2.5, "decay"),
        lambda: routing.route(fdr, -ok, "decay"),
        lambda: routing.route(fdr, -ok, "retain"),
        lambda: routing.route(fdr, -ok, "limit"),
        lambda: routing.route(fdr, ok * INF, "decay"),
        lambda: routing.route(fdr, ok * -INF, "limit"),
        lambda: routing.route(fdr, ok, "decay", weights=-ok),                     # weights, frac_bits
        lambda: routing.route(fdr, ok, "decay", weights=ok * INF),
        lambda: routing.route(fdr, ok, "decay", weights=ok[:, :4]),
        lambda: routing.route(fdr, ok, "decay", frac_bits=1.5),
        lambda: routing.route(fdr, ok, "decay", frac_bits=60),
        lambda: routing.route(fdr, ok, "decay", frac_bits=True),
        lambda: routing.decayed_accumulation(angle, ok * 3),
        lambda: routing.retention_limited(shares, -ok),
        lambda: routing.transport_limited(fdr, -ok, ok),
        lambda: routing.transport_limited(fdr, ok, -ok),
        lambda: routing.sink_capacity(ok, ok[:3], fdr, 10.0),                     # sink_capacity
        lambda: routing.sink_capacity(ok, ok, fdr[:3], 10.0),
        lambda: routing.sink_capacity(ok, ok, fdr, 0.0),
        lambda: routing.sink_capacity(ok, ok, fdr, np.nan),
        lambda: routing.sink_capacity(ok[0], ok[0], fdr[0], 10.0),
        lambda: routing.sink_capacity(ok, ok + 1, fdr, 10.0, frac_bits=60),
        lambda: routing.sink_capacity(ok, ok + 1, fdr, 10.0, frac_bits=0.5),
        lambda: routing.sink_capacity(ok, ok * INF, fdr, 10.0),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("bad call %d was accepted" % i)
    nan = ok.copy()
    nan[2, 3] = np.nan
    for transfer in routing.TRANSFERS:
        with pytest.raises(ValueError, match="flat index 13"):
            routing.route(fdr, nan, transfer)
    # +inf is a capacity, and the three flow rasters are told apart
    for flow in (fdr, shares, angle):
        for transfer in ("retain", "limit"):
            with pytest.raises(AssertionError, match="the library was reached"):
                routing.route(flow, ok * INF, transfer)
    assert routing.sink_capacity(ok, ok, fdr, 10.0).sum() == 0   # no lake cell: no library call either


def test_alias_module_serves_the_same_functions():
    import descriptools.routing as alias
    for name in ("route", "decayed_accumulation", "retention_limited", "transport_limited", "sink_capacity"):
        assert getattr(alias, name) is getattr(routing, name)
    assert "T(c) = q(c) + arrivals" in routing.__doc__ and "floor(T * D / 2^30)" in routing.__doc__


# ---- sink_capacity ---------------------------------------------------------------------------------------------------
def _three_pits():
    yy, xx = np.mgrid[0:40, 0:40]
    dem = (200 + 2.0 * yy + 0.5 * xx).astype(np.float32)  # drains north
    dem[8:13, 6:12] -= 9
    dem[10, 8] -= 3
    dem[22:25, 20:30] -= 6
    dem[30:36, 31:35] -= 14
    dem[33, 33] -= 1.5
    return dem


@pytest.mark.gpu
def test_sink_capacity_against_a_path_walk():
    from descriptools_amd import flowdir
    dem, px = _three_pits(), 2.5
    fdr, filled = flowdir.d8_conditioned(dem, px, return_filled=True)
    filled = np.asarray(filled, np.float64)
    lake = filled > dem
    assert 30 <= lake.sum() <= 84, "the three lowered blocks hold 84 cells"
    s = 20
    cap = routing.sink_capacity(dem, filled, fdr, px, frac_bits=s)
    H, W = dem.shape
    step = dict(zip(_dinf_ref.OCT_CODE, zip(_dinf_ref.OCT_DY, _dinf_ref.OCT_DX)))
    total = {}
    for y, x in np.argwhere(lake):
        q = int(np.rint(np.ldexp((filled[y, x] - np.float64(dem[y, x])) * px * px, s)))
        cy, cx = y, x
        for _ in range(H * W):  # walk to the first lake cell whose receiver is not a lake cell
            d = step.get(int(fdr[cy, cx]))
            if d is None:
                break
            ny, nx = cy + d[0], cx + d[1]
            if not (0 <= ny < H and 0 <= nx < W and lake[ny, nx]):
                break
            cy, cx = ny, nx
        else:
            raise AssertionError("the walk did not end")
        total[(cy, cx)] = total.get((cy, cx), 0) + q
    assert len(total) >= 3, "three pits: at least an exit each"
    want = np.zeros((H, W), np.float64)
    for (y, x), v in total.items():
        want[y, x] = np.ldexp(float(v), -s)
    assert np.array_equal(cap.view(np.int64), want.view(np.int64))
    # the default scale keeps the whole volume: the capacities sum to the volume within the quantisation
    vol = ((filled - dem)[lake] * px * px).sum()
    assert abs(routing.sink_capacity(dem, filled, fdr, px).sum() - vol) <= lake.sum() * 2.0 ** -20
