"""k_trunk_delta<15> (csrc/az_delta.h) at every tile count, chunk sequence and last-tile fill it can be given, and the
lock-step plies tests/test_delta_eval_gpu.py does not reach.

The shapes are those of tests/delta_cases.py (tests/test_delta_shapes_cpu.py asserts what the set holds): conv1 on 1 .. 5 tiles,
conv2 on 1 .. 13, conv3 on 1 .. 14 up to the 224-cell maximum, every last chunk behind every number of chunks of 4, last tiles
full and with one cell.  Every case is compared as uint32 bit patterns with net_eval (the full fused trunk) on the same engine
and with the CPU oracle, a few slots at a time, so that leaves of very different tile counts share a launch.

Lock-step: the tile threshold taken inside a search (k_trunk_rest beside k_trunk_delta in one batch), and games that end in
mid-episode -- terminal leaves, and freed slots that take new roots while their neighbours search on -- with the switch on
against the switch off and the oracle's games."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from tests import delta_cases as dc
from tests.test_delta_eval_gpu import K, MAX_TILES, N, NN, REC_KEYS, _assert_rows, _bits, _mid_root, _oracle_rows, _stack, _start_positions, _weight_sets
from tests.test_start_positions_gpu import _has_line

SLOTS = 5                                # net_eval_delta takes a pass per 5 leaves: about nine passes per root


@pytest.fixture(scope="module")
def weight_sets():
    return _weight_sets()


@pytest.fixture(scope="module")
def case_set():
    """(roots, {root name: [leaf cells, ...]}), the cases of a root in the generator's order: tile counts of neighbours differ"""
    R = dc.roots()
    mid = _mid_root()
    assert np.array_equal(R["mid"][0], mid[0]) and R["mid"][1:] == mid[1:]         # the mid-game root of the existing tests
    by_root = {k: [cells for _, kk, cells in dc.cases() if kk == k] for k in R}
    return R, by_root


# ---------------------------------------------------------------------------------------------------------------------
# the kernel at every shape
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ring", "negative"])
def test_every_shape_equals_the_full_trunk_and_the_oracle(weight_sets, case_set, tag):
    sd = weight_sets[tag]
    R, by_root = case_set
    o, onet = orc.Oracle(N, K, 1), orc.Net(N, sd)
    e = az.Engine(N, K, 4, SLOTS, model="plain")
    e.load_weights(sd, 0)
    try:
        seen = set()
        for k, root in R.items():
            cells = by_root[k]
            leaves = [dc.leaf_of(root, cs) for cs in cells]
            boards, players, lasts = _stack(leaves)
            oracle = _oracle_rows(onet, o, leaves)
            want = e.net_eval(boards, players, lasts)
            tiles = [dc.tile_counts(cs)[2] for cs in cells]
            # every case has at most 8 changed cells: at 15 tiles every one of them takes the delta path, -1 nowhere
            assert e.delta_max_tiles(15) == 15
            got = e.net_eval_delta(root[0], root[1], boards, players, lasts)
            assert got[3].tolist() == tiles, f"{tag}, root {k}: path taken"
            _assert_rows(got, want, oracle, f"{tag}, root {k}, threshold 15")
            # at the default threshold the cases above 12 tiles go to k_trunk_rest, in launches they share with every third of
            # the others, which stay where they were
            assert e.delta_max_tiles(MAX_TILES) == MAX_TILES
            pick = [i for i, t in enumerate(tiles) if t > MAX_TILES or i % 3 == 0]
            again = e.net_eval_delta(root[0], root[1], boards[pick], players[pick], lasts[pick])
            assert again[3].tolist() == [tiles[i] if tiles[i] <= MAX_TILES else -1 for i in pick], f"{tag}, root {k}: path at the default threshold"
            _assert_rows(again, [w[pick] for w in want], [oracle[i] for i in pick], f"{tag}, root {k}, default threshold")
            seen |= {t for t in tiles}
        assert seen == set(range(1, 15))                                     # (tests/test_delta_shapes_cpu.py has the rest)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# lock-step plies
# ---------------------------------------------------------------------------------------------------------------------
def _lockstep(sd, on, S, slots, G, seed, max_plies, start=None, tiles=0):
    e = az.Engine(N, K, S, slots, model="plain", log_table=orc.numpy_log_table(S))
    try:
        e.load_weights(sd, 0)
        e.set_delta_eval(on)
        if tiles:
            assert e.delta_max_tiles(tiles) == tiles
        if start is not None:
            e.set_start_positions(*start)
        c = e.selfplay(G, seed0=seed, max_plies=max_plies)
        nply, res = e.games()
        return dict(c=c, rec=e.records(), nply=nply, res=res, st=e.delta_stats(by_tiles=True))
    finally:
        e.close()


def _oracle_games(sd, S, start, G, seed, max_plies):
    """the oracle's games from the start positions (game g from position g % count), searched ply by ply with the game's own
    tape by absolute ply: [dict(nply, result, boards, movers, lasts, visits, pis, actions, maxd)]"""
    o, onet = orc.Oracle(N, K, S, log_table=orc.numpy_log_table(S)), orc.Net(N, sd)
    T = orc.selfplay_T_table(NN)
    last_ply = max_plies or NN

    def one(g):
        i = g % len(start[0])
        b, pl, last = start[0][i].copy(), int(start[1][i]), int(start[2][i])
        noise, us = orc.selfplay_tape(seed + g, N, maxply=last_ply)
        out = dict(boards=[], movers=[], lasts=[], visits=[], pis=[], actions=[], result=0, maxd=0)
        while True:
            m = int(np.count_nonzero(b))
            if m >= last_ply:
                break
            off = sum(NN - j for j in range(m))
            r = o.search(onet, b, pl, last, float(T[m]), noise[off:off + NN - m], float(us[m]))
            for key, v in (("boards", b.copy()), ("movers", pl), ("lasts", last), ("visits", r["N"]), ("pis", r["pi"]), ("actions", r["action"])):
                out[key].append(v)
            out["maxd"] = max(out["maxd"], r["maxd"])
            last = r["action"]
            b[last] = pl
            if _has_line(b, N, K):
                out["result"] = pl
                break
            if m + 1 == NN:
                out["result"] = 3
                break
            pl = 3 - pl
        out["nply"] = len(out["actions"])
        return out
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(one, range(G)))


def _assert_oracle(run, games, what):
    assert run["nply"].tolist() == [g["nply"] for g in games], f"{what}: plies per game"
    assert run["res"].tolist() == [g["result"] for g in games], f"{what}: results"
    rec = run["rec"]
    for key in ("boards", "movers", "lasts", "visits", "actions"):
        want = np.concatenate([np.asarray(g[key]).reshape(g["nply"], -1) for g in games])
        assert np.array_equal(rec[key].reshape(len(want), -1), want), f"{what}: {key} differ from the oracle"
    assert np.array_equal(_bits(rec["pis"]), _bits(np.concatenate([np.stack(g["pis"]) for g in games]))), f"{what}: pis differ from the oracle"


def _assert_switch(on, off, what):
    assert on["nply"].tolist() == off["nply"].tolist() and on["res"].tolist() == off["res"].tolist(), what
    for key in REC_KEYS:
        assert np.array_equal(on["rec"][key], off["rec"][key]), f"{what}: {key}: switch on and off differ"
    assert np.array_equal(_bits(on["rec"]["pis"]), _bits(off["rec"]["pis"])), what
    for key in ("games", "plies", "expansions", "simulations", "terminal_hits", "depth_sum", "root_evals", "cache_hits", "trunk_boards"):
        assert on["c"][key] == off["c"][key], f"{what}: {key}"
    assert off["st"] == dict(delta=0, full=0, tiles=0, base=0, by_tiles=[0] * 16), what


def _assert_counters(run, what):
    """what the per-slot counters of k_trunk_base / k_trunk_delta must add up to"""
    st, c = run["st"], run["c"]
    assert sum(st["by_tiles"]) == st["delta"], what
    assert sum(t * x for t, x in enumerate(st["by_tiles"])) == st["tiles"], what
    assert st["delta"] + st["full"] == c["trunk_boards"] == c["expansions"] + c["root_evals"] - c["cache_hits"], what
    assert st["base"] == 2 * c["plies"], what


def _start_list(start):
    return [(start[0][i], int(start[1][i]), int(start[2][i])) for i in range(len(start[0]))]


@pytest.mark.parametrize("tiles", [2, 4])
def test_tile_threshold_taken_inside_a_search(weight_sets, tiles):
    """Positions hugging a corner, an edge and the opposite corner, 24 simulations, threshold 2 and 4: border leaves stay on the
    delta path (a corner footprint is one tile, an edge footprint two), interior ones (4 tiles at depth 1, more below) go to
    k_trunk_rest in the same batch -- through the tile count, where the "ring" case of tests/test_delta_eval_gpu.py gets there
    through the changed-cell limit."""
    S, G, seed, max_plies = 24, 6, 1512, 7
    sd = weight_sets["synthetic"]
    start = _start_positions()
    on = _lockstep(sd, True, S, G, G, seed, max_plies, start, tiles)
    off = _lockstep(sd, False, S, G, G, seed, max_plies, start, tiles)
    what = f"threshold {tiles}"
    _assert_switch(on, off, what)
    games = _oracle_games(sd, S, start, G, seed, max_plies)
    _assert_oracle(on, games, what)
    _assert_counters(on, what)
    st = on["st"]
    assert max(g["maxd"] for g in games) <= 8                    # no leaf beyond the changed-cell limit: every fallback is the threshold's
    assert st["full"] > 0 and st["delta"] > 0
    assert not any(st["by_tiles"][tiles + 1:]) and st["tiles"] <= tiles * st["delta"]


def _dense(four, ends, mover, holes):
    """a nearly full board without a line of five on which `mover` has the open `four`: its `ends` and the `holes` are empty.
    The filling is a pattern of period 4 whose runs are 2 long in a row and on both diagonals and 1 long in a column; a stone
    that would still close a line (beside the four) takes the other colour or stays away."""
    b = np.zeros(NN, np.uint8)
    b[four] = mover
    keep = set(ends) | set(holes)
    for c in range(NN):
        if b[c] or c in keep:
            continue
        r, cc = divmod(c, N)
        b[c] = 1 if (cc + 2 * r) % 4 < 2 else 2
        if _has_line(b, N, K):
            b[c] = 3 - b[c]
        if _has_line(b, N, K):
            b[c] = 0
    for c in range(NN - 1, -1, -1):                              # player 1 moved first: as many stones as player 2, one more if 2 is to move
        d = int((b == 1).sum()) - int((b == 2).sum()) - (0 if mover == 1 else 1)
        if d == 0:
            break
        if c not in four and b[c] == (1 if d > 0 else 2):
            b[c] = 0
    assert not _has_line(b, N, K) and all(b[c] == 0 for c in keep)
    return b, mover, int(np.flatnonzero(b == 3 - mover)[0])


def _open_fours():
    """three positions with 9, 8 and 13 empty cells: a row four in the middle, a diagonal four near a corner with player 2 to move,
    a column four on the right edge; the other holes lie in corners, on edges and inside, far from one another"""
    C = dc.C
    return _stack([_dense([C(7, 4), C(7, 5), C(7, 6), C(7, 7)], [C(7, 3), C(7, 8)], 1, [0, N - 1, C(14, 0), C(3, 11), C(11, 3)]),
                   _dense([C(2, 2), C(3, 3), C(4, 4), C(5, 5)], [C(1, 1), C(6, 6)], 2, [C(0, 7), C(14, 14), C(12, 8), C(7, 14)]),
                   _dense([C(9, 14), C(10, 14), C(11, 14), C(12, 14)], [C(8, 14), C(13, 14)], 1, [C(0, 0), C(2, 7), C(7, 0), C(14, 6), C(5, 10)])])


def test_games_end_and_slots_take_new_roots_in_mid_episode(weight_sets):
    """7 games on 3 slots from positions in which the mover has an open four on a nearly full board: 24 simulations cover the few
    legal moves, meet the winning ones as terminal leaves, and the games end after 1 to 5 plies -- at different plies, so a freed
    slot takes the next game's root (and its two base evaluations) while its neighbours are in mid-game."""
    S, slots, G, seed = 24, 3, 7, 1600
    sd = weight_sets["synthetic"]
    start = _open_fours()
    on = _lockstep(sd, True, S, slots, G, seed, 0, start)
    off = _lockstep(sd, False, S, slots, G, seed, 0, start)
    _assert_switch(on, off, "open fours")
    games = _oracle_games(sd, S, start, G, seed, 0)
    _assert_oracle(on, games, "open fours")
    _assert_counters(on, "open fours")
    # every game was played and ended by a win, more games than slots, not all of the same length: slots were refilled in mid-episode
    assert on["c"]["games"] == G > slots and len(on["nply"]) == G
    assert all(r in (1, 2) for r in on["res"].tolist()) and len(set(on["nply"].tolist())) > 1
    assert int(on["nply"].sum()) == on["c"]["plies"] > G
    assert on["c"]["terminal_hits"] > 0 and on["st"]["delta"] > 0
