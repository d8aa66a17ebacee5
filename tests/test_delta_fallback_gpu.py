"""The fallback inside k_trunk_delta<15> (csrc/az_delta.h): a board with more than 8 changed cells, or more conv3
tiles than az_delta_max_tiles, is evaluated in full by the delta workgroup itself -- 15 tiles per layer through the delta chunk
loops, zero-filled images, nothing read from the base -- where a second launch ran the fused trunk's code before.  Every output
element is still the same k-ordered chain over the same window, so everything is compared as uint32 bit patterns: with net_eval
on the same engine and with the CPU oracle; lock-step runs with the switch on against the switch off and the oracle's games.
15x15, at most 6 slots, the border-sharp "ring" and "negative" weight sets of tests/test_delta_eval_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from tests import delta_cases as dc
from tests.test_delta_eval_gpu import K, MAX_CHANGED, MAX_TILES, N, NN, _assert_rows, _oracle_rows, _stack, _start_positions, _weight_sets
from tests.test_delta_shapes_gpu import _assert_counters, _assert_oracle, _assert_switch, _lockstep, _open_fours, _oracle_games

SLOTS = 6
TAGS = ["ring", "negative"]
C = dc.C


@pytest.fixture(scope="module")
def weight_sets():
    return _weight_sets()


def _nine():
    """9 changed cells in a 3x3 block from the empty board: beyond the changed-cell limit although its footprint is 5 tiles"""
    return [C(7, 6) + j for j in range(3)] + [C(8, 6) + j for j in range(3)] + [C(9, 6) + j for j in range(3)]


def _leaves():
    """[(root name, leaf cells)]: the cases of tests/delta_cases.py above 2 conv3 tiles, the smallest and the largest windows, and
    a leaf with 9 changed cells"""
    out = [(k, cells) for _, k, cells in dc.cases() if dc.tile_counts(cells)[2] > 2]
    out += [("empty", [0]),                                                        # a corner: one tile, the smallest windows
            ("empty", [C(3, 3), C(3, 7), C(3, 11), C(11, 3), C(11, 7), C(11, 11), C(7, 3), C(7, 10)]),    # 8 cells, 14 tiles: the largest
            ("empty", _nine())]
    return out


@pytest.fixture(scope="module")
def reference(weight_sets):
    """per weight set: ONE engine, kept open for the tests (net_eval and net_eval_delta on the same engine), and the leaves by
    root with net_eval's rows and the oracle's, computed once"""
    R = dc.roots()
    ref, engines = {}, {}
    try:
        for tag in TAGS:
            sd = weight_sets[tag]
            o, onet = orc.Oracle(N, K, 1), orc.Net(N, sd)
            e = engines[tag] = az.Engine(N, K, 4, SLOTS, model="plain")
            e.load_weights(sd, 0)
            by_root = {}
            for k, root in R.items():
                cells = [cs for kk, cs in _leaves() if kk == k]
                leaves = [dc.leaf_of(root, cs) for cs in cells]
                boards, players, lasts = _stack(leaves)
                by_root[k] = dict(cells=cells, leaves=_stack(leaves), want=e.net_eval(boards, players, lasts),
                                  oracle=_oracle_rows(onet, o, leaves), tiles=[dc.tile_counts(cs)[2] for cs in cells])
            ref[tag] = by_root
        yield R, ref, engines
    finally:
        for e in engines.values():
            e.close()


def _path(tiles, cells, threshold):
    return [-1 if len(cs) > MAX_CHANGED or t > threshold else t for t, cs in zip(tiles, cells)]


@pytest.mark.parametrize("tag", TAGS)
def test_every_case_above_two_tiles_in_full_at_threshold_2(weight_sets, reference, tag):
    R, ref, engines = reference
    e = engines[tag]
    try:
        assert e.delta_max_tiles(2) == 2
        n_full = 0
        for k, root in R.items():
            r = ref[tag][k]
            got = e.net_eval_delta(root[0], root[1], *r["leaves"])
            want_path = _path(r["tiles"], r["cells"], 2)
            assert got[3].tolist() == want_path, f"{tag}, root {k}: path taken"
            _assert_rows(got, r["want"], r["oracle"], f"{tag}, root {k}, threshold 2")
            n_full += want_path.count(-1)
        assert n_full >= 100
    finally:
        e.delta_max_tiles(MAX_TILES)                     # the engine is shared: back to the default


@pytest.mark.parametrize("tag", TAGS)
def test_default_threshold_13_and_14_tiles_nine_cells_and_a_mixed_launch(weight_sets, reference, tag):
    """one launch of 6 boards: the corner leaf (1 tile, the smallest windows) and the 8-cell 14-tile leaf at threshold 15 (the
    largest), then at the default threshold the 13- and 14-tile cases and the 9-cell leaf in full beside delta boards"""
    R, ref, engines = reference
    e = engines[tag]
    try:
        r = ref[tag]["empty"]
        root = R["empty"]
        tiles, cells = r["tiles"], r["cells"]
        big = [i for i, t in enumerate(tiles) if t in (13, 14)]
        assert {tiles[i] for i in big} == {13, 14}
        corner, widest, nine = len(cells) - 3, len(cells) - 2, len(cells) - 1
        assert tiles[corner] == 1 and tiles[widest] == 14 and len(cells[widest]) == 8 and len(cells[nine]) == 9
        small = [i for i, t in enumerate(tiles) if 3 <= t <= 6][:2]
        pick = np.array([corner, big[0], small[0], nine, widest, small[1]])       # delta and full boards side by side, one pass
        sub = lambda rows: [x[pick] for x in rows]
        for threshold in (MAX_TILES, 15):
            assert e.delta_max_tiles(threshold) == threshold
            got = e.net_eval_delta(root[0], root[1], *sub(r["leaves"]))
            assert got[3].tolist() == _path([tiles[i] for i in pick], [cells[i] for i in pick], threshold), f"{tag}: path at threshold {threshold}"
            assert (-1 in got[3].tolist()) and any(t > 0 for t in got[3].tolist())
            _assert_rows(got, sub(r["want"]), [r["oracle"][i] for i in pick], f"{tag}, mixed launch, threshold {threshold}")
        # every 13- and 14-tile case of every root, in full at the default threshold
        assert e.delta_max_tiles(MAX_TILES) == MAX_TILES
        for k, rt in R.items():
            rr = ref[tag][k]
            idx = np.array([i for i, t in enumerate(rr["tiles"]) if t > MAX_TILES or len(rr["cells"][i]) > MAX_CHANGED], int)
            if not len(idx):
                continue
            got = e.net_eval_delta(rt[0], rt[1], *[x[idx] for x in rr["leaves"]])
            assert got[3].tolist() == [-1] * len(idx), f"{tag}, root {k}"
            _assert_rows(got, [x[idx] for x in rr["want"]], [rr["oracle"][i] for i in idx], f"{tag}, root {k}, 13 and 14 tiles in full")
    finally:
        e.delta_max_tiles(MAX_TILES)                     # the engine is shared: back to the default


@pytest.mark.parametrize("tiles", [2, 0])
def test_lockstep_six_slots_24_simulations(weight_sets, tiles):
    """Positions hugging a corner, an edge and the opposite corner: at threshold 2 interior leaves are evaluated in full beside
    border leaves on the delta path in the same launches; at the default (0 = leave it) through the changed-cell limit only.
    Records and counters as with the switch off, and as the oracle's games; the counter identities of 5g unchanged."""
    S, G, seed, max_plies = 24, 6, 1613, 7
    sd = weight_sets["ring"]
    start = _start_positions()
    on = _lockstep(sd, True, S, G, G, seed, max_plies, start, tiles)
    off = _lockstep(sd, False, S, G, G, seed, max_plies, start, tiles)
    what = f"threshold {tiles or MAX_TILES}"
    _assert_switch(on, off, what)
    games = _oracle_games(sd, S, start, G, seed, max_plies)
    _assert_oracle(on, games, what)
    _assert_counters(on, what)
    st = on["st"]
    assert st["delta"] > 0 and st["full"] > 0, st              # "ring": priors so sharp that lines run past 8 stones
    lim = tiles or MAX_TILES
    assert not any(st["by_tiles"][lim + 1:]) and st["tiles"] <= lim * st["delta"]


def test_inactive_slots_and_leaves_without_evaluation_beside_full_boards(weight_sets, monkeypatch):
    """4 games on 6 slots from open fours on nearly full boards, threshold 2, AZ_COMPACT=0: without compaction every launch has
    the grid of all 6 slots, so slots 4 and 5, which never get a game, are inactive workgroups in every k_trunk_delta launch, and
    so is the slot of every game that has ended.  The winning moves are met as terminal leaves (no evaluation), holes inside
    the board give boards in full and holes in corners delta boards."""
    monkeypatch.setenv("AZ_COMPACT", "0")                # read when the engine is created
    S, slots, G, seed = 24, SLOTS, 4, 1614
    sd = weight_sets["negative"]
    start = _open_fours()
    on = _lockstep(sd, True, S, slots, G, seed, 0, start, 2)
    off = _lockstep(sd, False, S, slots, G, seed, 0, start, 2)
    _assert_switch(on, off, "open fours, threshold 2")
    _assert_oracle(on, _oracle_games(sd, S, start, G, seed, 0), "open fours, threshold 2")
    _assert_counters(on, "open fours, threshold 2")
    assert on["c"]["games"] == G < slots and on["c"]["terminal_hits"] > 0
    assert len(set(on["nply"].tolist())) > 1             # games end at different plies: their slots idle beside the others
    assert on["st"]["full"] > 0 and on["st"]["delta"] > 0
