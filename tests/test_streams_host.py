"""CPU (not gpu): streams.stream_network / strahler / shreve refuse bad arguments with ValueError before any library
call, call the bound dt_stream_order, and the entry points are declared and bound.  The pure-numpy reference that the
GPU tests hold the kernels to (tests/_streams_ref.py) is checked here on hand-built networks."""
import os
import re

import numpy as np
import pytest

from descriptools_amd import _lib, streams

import _streams_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(streams._lib, "lib", boom)


FDR = np.full((5, 7), R.E, np.uint8)


@pytest.mark.parametrize("fn", [streams.stream_network, streams.strahler, streams.shreve])
@pytest.mark.parametrize("fdr, river, what", [
    (np.ones(7, np.uint8), np.ones(7, np.int8), "2-D"),
    (np.ones((2, 3, 4), np.uint8), np.ones((2, 3, 4), np.int8), "2-D"),
    (FDR, np.ones((5, 6), np.int8), "shape"),
    (FDR, np.ones((7, 5), bool), "shape"),
    (FDR, np.ones((5, 7), np.float32), "bool or integer"),
    (FDR, np.ones((5, 7), np.float64), "bool or integer"),
    (FDR, np.full((5, 7), "a"), "bool or integer"),
])
def test_bad_arguments_refused_before_the_library(no_library, fn, fdr, river, what):
    with pytest.raises(ValueError, match=what):
        fn(fdr, river)


class _FakeLib:
    """records dt_stream_order calls and fills the outputs it is given"""

    def __init__(self):
        self.calls = []

    def dt_stream_order(self, f, r, H, W, so, sh, lk):
        self.calls.append((H, W, so is not None, sh is not None, lk is not None))
        n = H * W
        if so:
            np.ctypeslib.as_array(so, (n,))[:] = 7
        if sh:
            np.ctypeslib.as_array(sh, (n,))[:] = 8
        if lk:
            np.ctypeslib.as_array(lk, (n,))[:] = 9
        return 0


def test_entry_points_call_the_bound_symbol(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(streams._lib, "lib", lambda: fake)
    river = np.zeros((5, 7), bool)
    net = streams.stream_network(FDR, river)
    assert isinstance(net, streams.StreamNetwork) and net._fields == ("strahler", "shreve", "link")
    assert net.strahler.dtype == np.int8 and net.shreve.dtype == np.int64 and net.link.dtype == np.int64
    assert (net.strahler == 7).all() and (net.shreve == 8).all() and (net.link == 9).all()
    so = streams.strahler(FDR, river.astype(np.uint16))
    assert so.dtype == np.int8 and so.shape == (5, 7) and (so == 7).all()
    sh = streams.shreve(FDR, river.astype(np.int32))
    assert sh.dtype == np.int64 and (sh == 8).all()
    assert fake.calls == [(5, 7, True, True, True), (5, 7, True, False, False), (5, 7, True, True, True)]


def test_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    for name in ("dt_stream_order", "dt_dev_stream_order"):
        assert re.search(r"\bint %s\(" % name, hdr), name
    assert "dt_stream_order" in _lib._SIGS
    assert "dt_dev_stream_order" in _lib._SIGS
    from descriptools_amd import build
    assert "dt_streams.hip" in build.SOURCES


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_reference_on_hand_built_networks(name):
    fdr, river, so, sh, lk = R.hand_cases()[name]
    got = R.reference(fdr, river)
    assert got[0].dtype == np.int8 and got[1].dtype == np.int64 and got[2].dtype == np.int64
    np.testing.assert_array_equal(got[0], so)
    np.testing.assert_array_equal(got[1], sh)
    np.testing.assert_array_equal(got[2], lk)


def test_reference_rules():
    """the hand cases cover each rule the issue names"""
    c = R.hand_cases()
    assert c["y"][2].max() == 2                        # two 1s give 2
    assert c["two_joined_by_one"][2][3, 1] == 2         # a 2 joined by a 1 stays 2
    assert c["two_twos"][2].max() == 3                  # two 2s give 3
    assert c["three_sources"][2][1, 1] == 2 and c["three_sources"][3][1, 1] == 3
    assert (c["gap"][4] == [[0, 0, -100, 3, 3]]).all()  # a gap splits the network
    assert (c["pure_cycle"][2][:, :2] == -100).all()
    assert c["cycle_with_tributary"][2][2, 2] == 1 and (c["cycle_with_tributary"][2][:2, :2] == -100).all()


def test_reference_link_constancy():
    """Strahler and Shreve are constant along a link (random south-draining field)"""
    rng = np.random.default_rng(3)
    fdr = rng.choice(np.array([R.SW, R.S, R.SE], np.uint8), size=(40, 33))
    river = rng.random((40, 33)) < 0.7
    so, sh, lk = R.reference(fdr, river)
    net = lk >= 0
    heads = lk[net]
    assert (so[net] == so.reshape(-1)[heads]).all()
    assert (sh[net] == sh.reshape(-1)[heads]).all()
    assert (so[~river] == 0).all() and (sh[~river] == 0).all() and (lk[~river] == -100).all()
