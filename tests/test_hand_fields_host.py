"""CPU only: the reference of test_gpu_hand_fields.py checked against itself before it judges a kernel -- the closed
form over the oracle's O(N) solve (_hand_fields.expected) against the oracle's literal per-cell walk on every family
-- and the conditions the families are built for: which tiles the narrow tile solve keeps and which it gives up, the
255 / 256 in-tile counts, the 20000 / 20001 cap boundaries."""
import numpy as np
import pytest

import oracle

import _hand_fields as F


def _check_against_walk(name):
    f, e = F.field(name), F.answer(name)
    fd, idx, hand = oracle.flowhand(f.dem, f.fdr, f.river, F.PX)
    assert np.array_equal(idx, e["idx"]), "%d river indices differ" % int((idx != e["idx"]).sum())
    assert np.array_equal(hand, e["hand"])
    one = F.one_kind(e)
    assert np.array_equal(fd[one], e["fdist"][one])
    # mixed paths: the closed form rounds once, the walk sums move by move
    assert np.allclose(fd[~one], e["fdist"][~one], rtol=1e-6, atol=0)
    ok = e["idx"] != -100
    assert np.array_equal(e["a_river"][ok], e["fac"].ravel()[e["idx"][ok]]) and (e["a_river"][~ok] == -100).all()


@pytest.mark.parametrize("name", F.small_names())
def test_expected_equals_the_literal_walk(name):
    _check_against_walk(name)


def test_expected_equals_the_literal_walk_on_the_long_zigzag():
    """hop_dense: one literal run, member (a); the others rest on flowhand_fast alone"""
    _check_against_walk("hop_a20100_e")
    e = F.answer("hop_a20100_e")
    ok = e["idx"] != -100
    assert int(ok.sum()) == 20001 and e["nd"][ok].max() == 20000 and e["nc"][ok].max() == 0


def test_from_path_and_the_in_tile_walk():
    cells = [(0, 0), (0, 1), (1, 2), (2, 2), (3, 1), (3, 0), (2, 0)]
    fdr = F.from_path((5, 4), cells, 64)
    assert [int(fdr[c]) for c in cells] == [1, 2, 4, 8, 16, 64, 64] and int((fdr != 0).sum()) == 7
    river = np.zeros((5, 4), np.int8)
    river[3, 0] = 1
    nc, nd = F.intile_counts(fdr, river)
    assert (nc[0, 0], nd[0, 0]) == (3, 2) and (nc[2, 0], nd[2, 0]) == (1, 0) and nc[3, 0] == 0
    # leaving the tile ends the walk: E along row 0 of a 1 x 130 raster
    nc, nd = F.intile_counts(np.full((1, 130), 1, np.uint8), np.zeros((1, 130), np.int8))
    assert nc[0, 0] == 63 and nc[0, 63] == 0 and nc[0, 64] == 63 and nc[0, 128] == 1 and nc[0, 129] == 0
    # an in-tile cycle runs into the walk's cap
    nc, nd = F.intile_counts(F.from_path((2, 2), [(0, 0), (0, 1)], 16), np.zeros((2, 2), np.int8))
    assert nc[0, 0] == 4096


@pytest.mark.parametrize("name", F.small_names(["descending", "uniform", "quirk", "cap_mixed"]) + F.HOP_NAMES)
def test_every_tile_stays_narrow(name):
    f = F.field(name)
    assert not F.wide_tiles(f.fdr, f.river).any()


@pytest.mark.parametrize("name", F.small_names(["random_codes"]))
def test_random_codes_send_every_tile_wide(name):
    f = F.field(name)
    assert F.wide_tiles(f.fdr, f.river).all()


@pytest.mark.parametrize("name", F.small_names(["planted"]))
def test_planted_has_both_kinds_of_tile_and_paths_between_them(name):
    f, e = F.field(name), F.answer(name)
    wide = F.wide_tiles(f.fdr, f.river)
    assert wide.any() and not wide.all()
    cross = F.tile_crossings(f.fdr)
    both = [(a, b) for a, b in cross if wide[a] and not wide[b] and (b, a) in cross]
    assert both, "no wide tile exchanges paths with a narrow neighbour in both directions"
    # the cycles and what feeds them are dead; the four-corner cycle lies in narrow tiles
    for y, x in ((10, 10), (10, 11), (63, 63), (63, 64), (64, 64), (64, 63), (84, 148), (157, 215), (226, 296)):
        assert e["idx"][y, x] == -100 or f.river[y, x] == 1
    assert not wide[0, 1] and not wide[1, 0] and not wide[1, 1] and wide[1, 2]
    assert np.isin(f.fdr, F.NON_D8).sum() > 0.005 * f.fdr.size


@pytest.mark.parametrize("shape", F.BIG)
@pytest.mark.parametrize("seed", [0, 1])
def test_count_edges_hit_255_and_256(shape, seed):
    (f,), plan = F.count_edges(shape, seed)
    nc, nd = F.intile_counts(f.fdr, f.river)
    wide = F.wide_tiles(f.fdr, f.river)
    e = F.expected(f.dem, f.fdr, f.river, F.PX)
    assert sorted((c, d, l) for c, d, l, _ in plan.values()) == sorted(
        (c, d, l) for c, d in F.COUNT_EDGES for l in (False, True))
    for tile, (c, d, leaves, head) in plan.items():
        y0, x0 = tile[0] * F.TILE, tile[1] * F.TILE
        t = (slice(y0, y0 + F.TILE), slice(x0, x0 + F.TILE))
        assert (nc[head], nd[head]) == (c, d) and nc[t].max() == c and nd[t].max() == d
        assert wide[tile] == (max(c, d) > 255)
        # the path that leaves has the river 3 moves on
        assert (e["nc"][head], e["nd"][head]) == ((c + 3, d) if leaves else (c, d))
    assert wide.sum() == 4 and not wide.all()
    interior = [t for t in plan if 0 < t[0] < wide.shape[0] - 1 and 0 < t[1] < wide.shape[1] - 1]
    assert any(plan[t][2] for t in interior) if seed == 0 else any(not plan[t][2] for t in interior)


def test_cap_boundaries_exist():
    for name, least in (("cap_mixed-512x512", 4), ("hop_d19990_e", 1), ("hop_d20010_w", 1)):
        f, e = F.field(name), F.answer(name)
        # distance to the river along the codes whatever the cap says: the oracle's answer with the river moved
        moves = e["nc"] + e["nd"]
        ok = e["idx"] != -100
        assert (moves[ok] == 19999).sum() >= least and (moves[ok] == 20000).sum() >= least
        # a cell at 20001 moves: dead, and its successor resolves with 20000
        H, W = f.fdr.shape
        ys, xs = np.nonzero(ok & (moves == 20000))
        ups = 0
        for y, x in zip(ys.tolist(), xs.tolist()):
            for c, (dy, dx) in F.DELTA.items():
                py, px = y - dy, x - dx
                if 0 <= py < H and 0 <= px < W and f.fdr[py, px] == c and f.river[py, px] != 1:
                    assert e["idx"][py, px] == -100
                    ups += 1
        assert ups >= least
        if name.startswith("cap_mixed"):
            assert (e["nc"][ok] > 5000).any() and (e["nd"][ok] > 5000).any()
    # member (d): the boundary lies in the feeder, off the zigzag's rows
    for name in ("hop_d19990_e", "hop_d20010_e"):
        e = F.answer(name)
        ok = e["idx"] != -100
        ys = np.nonzero(ok & (e["nc"] + e["nd"] == 20000))[0]
        assert ((ys < 63) | (ys > 64)).any()


def test_cycles_across_tiles_are_dead():
    for name in ("hop_c_e", "hop_c_w"):
        f, e = F.field(name), F.answer(name)
        coded = f.fdr != 0
        assert int(coded.sum()) == 15000 + 25000 + 2 * 6 + 40
        assert int((e["idx"] != -100).sum()) == 40
