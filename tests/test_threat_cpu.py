"""az_threat_solve, the host form of the root threat search, against the numpy restatement in tests/threat.py and against brute
force (no GPU needed).  The restatement is the rule of include/az_engine.h as written; the brute force knows nothing of fours."""
import functools

import numpy as np
import pytest

from tests import threat as th

from alphazero_piskvorky_amd import _capi

DEPTHS = (1, 2, 4, 6)
BUDGETS = (1, 3, 65535)
# (n, k, ((stones, positions), ..)): the counts and the seed are chosen so that the restatement alone satisfies the counts below
SIZES = {"5x5": (5, 4, ((8, 150), (12, 150))), "7x7": (7, 4, ((14, 450),)), "9x9": (9, 5, ((30, 240),))}
SEED = 7


@functools.lru_cache(maxsize=None)
def sample(size, rule):
    n, k, sets = SIZES[size]
    bs, ps = zip(*(th.positions(n, k, rule, stones, count, SEED + stones) for stones, count in sets))
    return n, k, np.concatenate(bs), np.concatenate(ps)


def assert_equal(got, want, what):
    for key in ("status", "move", "depth", "nodes"):
        assert got[key] == want[key], f"{what}: {key} {got[key]} != {want[key]}"
    assert got["edges"].dtype == np.int8 and np.array_equal(got["edges"], want["edges"]), f"{what}: edges"


def test_the_vectorised_win_sets_are_the_definition():
    rs = np.random.RandomState(1)
    for n, k in ((3, 3), (5, 4), (9, 5), (15, 5)):
        for rule in th.RULES:
            for _ in range(10):
                b = rs.choice(3, size=n * n, p=[.5, .25, .25]).astype(np.uint8)
                for colour in (1, 2):
                    want = [a for a in range(n * n) if b[a] == 0 and th.stone_wins(b, a, n, k, rule, colour)]
                    assert th.win_set(b, n, k, rule, colour) == want


@pytest.mark.parametrize("rule", th.RULES)
@pytest.mark.parametrize("size", list(SIZES))
def test_threat_solve_equals_the_restatement(size, rule):
    """status, move, depth, nodes and every edge.  Every position is solved at max_depth 6 without a budget limit and at one
    small budget; the other (max_depth, node_budget) pairs go round the positions, so each pair meets a few dozen of them."""
    n, k, boards, players = sample(size, rule)
    pairs = [(d, b) for d in DEPTHS for b in BUDGETS]
    d2 = d3 = loss = exhausted = 0
    for i, (board, player) in enumerate(zip(boards, players)):
        runs = [(6, 65535), (6, BUDGETS[i % 2]), pairs[i % len(pairs)]]
        for max_depth, budget in runs:
            want = th.solve(board, n, k, rule, player, max_depth, budget)
            got = _capi.threat_solve(board, n, k, rule, int(player), max_depth, budget)
            assert_equal(got, want, f"{size} {rule} position {i} depth {max_depth} budget {budget}")
            if (max_depth, budget) == (6, 65535) and runs.index((max_depth, budget)) == 0:
                d2 += want["depth"] == 2
                d3 += want["depth"] >= 3
                loss += bool((want["edges"] == th.LOSS).any())
            elif budget in (1, 3) and max_depth == 6 and (max_depth, budget) == runs[1]:
                exhausted += want["nodes"] > budget
                if want["nodes"] > budget:
                    assert want["depth"] == 0 and want["move"] == -1 and want["status"] != th.WIN
    assert d2 >= 10 and d3 >= 10 and loss >= 10 and exhausted >= 5, (d2, d3, loss, exhausted)


@pytest.mark.parametrize("rule", th.RULES)
@pytest.mark.parametrize("stones,count,max_win", [(12, 120, 3), (14, 100, 4)])
def test_soundness_by_brute_force(stones, count, max_win, rule):
    """5x5 / k = 4: every win of depth d <= max_win is a forced win within 2d - 1 plies by brute force (a win of depth 4 only
    with 14 stones, where 11 cells are left), and after every LOSS edge the opponent has an immediate win."""
    n, k = 5, 4
    boards, players = th.positions(n, k, rule, stones, count, 100 + stones)
    wins = losses = 0
    for board, player in zip(boards, players):
        player = int(player)
        got = _capi.threat_solve(board, n, k, rule, player, 6, 65535)
        if 0 < got["depth"] <= max_win:
            assert got["status"] == th.WIN and got["edges"][got["move"]] == th.WIN
            after = board.copy()
            if got["depth"] == 1:
                for a in np.flatnonzero(got["edges"] == th.WIN):
                    assert th.stone_wins(board, int(a), n, k, rule, player)
            else:
                # the move itself, then any defence: the mover wins within 2d - 1 plies in all
                assert th.forced_win_within(after, n, k, rule, player, 2 * got["depth"] - 1)
                after[got["move"]] = player
                for b in np.flatnonzero(after == 0):
                    after[b] = 3 - player
                    assert th.forced_win_within(after, n, k, rule, player, 2 * got["depth"] - 3), (board, got)
                    after[b] = 0
            wins += 1
        for a in np.flatnonzero(got["edges"] == th.LOSS):
            after = board.copy()
            after[a] = player
            assert any(th.stone_wins(after, int(b), n, k, rule, 3 - player) for b in np.flatnonzero(after == 0))
            losses += 1
    assert wins >= 8 and losses > 0, (wins, losses)


@pytest.mark.parametrize("rule", th.RULES)
def test_a_proven_win_is_found_again_after_the_forced_reply(rule):
    """Carry-through without the budget: after the winning four and the forced reply, the search at the same max_depth -- one
    level deeper than the first search's recursion was -- finds a win again.  With a budget it can run out first: the follow-up
    may need more nodes than the whole first search did, and then no win is reported (counted here, not asserted away)."""
    n, k, depth, budget = 9, 5, 6, 256
    boards, players = sample("9x9", rule)[2:]
    deep = lost = 0
    for board, player in zip(boards, players):
        player = int(player)
        t = _capi.threat_solve(board, n, k, rule, player, depth, budget)
        if t["depth"] < 3:
            continue
        after = board.copy()
        after[t["move"]] = player
        W = th.win_set(after, n, k, rule, player)
        assert len(W) == 1
        after[W[0]] = 3 - player
        again = _capi.threat_solve(after, n, k, rule, player, depth, 65535)
        assert again["status"] == th.WIN and again["depth"] >= 2
        lost += _capi.threat_solve(after, n, k, rule, player, depth, budget)["status"] != th.WIN
        deep += 1
    assert deep >= 20
    print(f"{rule}: {deep} wins of depth >= 3, {lost} lost again under node_budget {budget}")


def solve9(pos, rule, max_depth=8, budget=256):
    board, player = pos[0], pos[1]
    want = th.solve(board, 9, 5, rule, player, max_depth, budget)
    got = _capi.threat_solve(board, 9, 5, rule, player, max_depth, budget)
    assert_equal(got, want, "crafted")
    return got


@pytest.mark.parametrize("rule", th.RULES)
def test_crafted_double_four(rule):
    pos = th.crafted_double_four()
    got = solve9(pos, rule, 2)
    assert (got["status"], got["move"], got["depth"], got["nodes"]) == (th.WIN, pos[2], 2, 1)
    assert np.flatnonzero(got["edges"]).tolist() == [pos[2]]
    assert solve9(pos, rule, 1)["status"] == th.UNKNOWN            # depth 1 sees only immediate wins


def test_crafted_four_whose_completion_is_an_overline():
    pos = th.crafted_overline_four()
    free, exact = solve9(pos, "freestyle"), solve9(pos, "exact")
    assert free["nodes"] >= 1 and exact["nodes"] == 0               # a four under freestyle, none under the exact rule
    assert free["status"] == exact["status"] == th.UNKNOWN and not free["edges"].any() and not exact["edges"].any()
    after = pos[0].copy()
    after[pos[2]] = 1
    assert th.win_set(after, 9, 5, "freestyle", 1) == [4 * 9 + 4] and th.win_set(after, 9, 5, "exact", 1) == []


@pytest.mark.parametrize("rule", th.RULES)
def test_crafted_single_forced_block_that_is_no_four(rule):
    board, player, block = th.crafted_single_block()
    got = solve9((board, player), rule)
    assert (got["status"], got["move"], got["depth"], got["nodes"]) == (th.UNKNOWN, -1, 0, 0)
    want = np.where(board == 0, th.LOSS, 0)
    want[block] = th.UNKNOWN
    assert np.array_equal(got["edges"], want)
    assert np.array_equal(solve9((board, player), rule, 1, 1)["edges"], want)      # the marks depend on neither depth nor budget


@pytest.mark.parametrize("rule", th.RULES)
def test_crafted_two_opposing_completions(rule):
    board, player, cells = th.crafted_two_completions()
    got = solve9((board, player), rule)
    assert (got["status"], got["move"], got["depth"]) == (th.LOSS, -1, 0)
    assert np.array_equal(got["edges"], np.where(board == 0, th.LOSS, 0)) and all(got["edges"][c] == th.LOSS for c in cells)


@pytest.mark.parametrize("rule", th.RULES)
def test_crafted_block_that_is_itself_a_four(rule):
    board, player, move = th.crafted_block_is_four()
    got = solve9((board, player), rule)
    assert (got["status"], got["move"], got["depth"], got["nodes"]) == (th.WIN, move, 2, 1)
    assert np.flatnonzero(got["edges"]).tolist() == [move]          # a win found: no LOSS marks


@pytest.mark.parametrize("rule", th.RULES)
@pytest.mark.parametrize("n", [9, 15])
def test_crafted_depth_three(n, rule):
    board, player, move = th.crafted_depth3(n)
    want = th.solve(board, n, 5, rule, player, 8, 256)
    got = _capi.threat_solve(board, n, 5, rule, player, 8, 256)
    assert_equal(got, want, "depth 3")
    assert (got["status"], got["move"], got["depth"]) == (th.WIN, move, 3)
    assert _capi.threat_solve(board, n, 5, rule, player, 2, 256)["status"] == th.UNKNOWN
    assert th.forced_win_within(board.copy(), n, 5, rule, player, 3) is False       # no shorter forced win exists


def test_argument_checks():
    board, player, _ = th.crafted_double_four()
    ok = dict(board=board, n=9, k=5, rule="freestyle", player=1, max_depth=8, node_budget=256)
    assert _capi.threat_solve(**ok)["status"] == th.WIN
    for bad in (dict(max_depth=0), dict(max_depth=17), dict(node_budget=0), dict(node_budget=65536), dict(player=0), dict(player=3),
                dict(k=0), dict(k=10), dict(n=16, board=np.zeros(256, np.uint8)), dict(board=np.full(81, 3, np.uint8)),
                dict(board=np.where(np.arange(81) % 2, 1, 2).astype(np.uint8))):
        with pytest.raises(ValueError):
            _capi.threat_solve(**{**ok, **bad})
    won = np.zeros(81, np.uint8)
    won[:5] = 1
    won[9:13] = 2
    with pytest.raises(ValueError):                                  # already won
        _capi.threat_solve(**{**ok, "board": won})
    six = np.zeros(81, np.uint8)
    six[:6] = 1
    six[9:15] = 2
    assert _capi.threat_solve(**{**ok, "board": six, "rule": "exact"})["status"] == th.UNKNOWN       # overlines only: a legal position
    with pytest.raises(ValueError):
        _capi.threat_solve(**{**ok, "rule": "renju"})
    lib = _capi.lib()
    assert lib.az_threat_solve(None, 9, 5, 0, 1, 8, 256, None, None, None, None) < 0
    b = np.ascontiguousarray(board, np.uint8)
    assert lib.az_threat_solve(b.ctypes.data, 9, 5, 0, 1, 8, 256, None, None, None, None) == th.WIN  # every output may be NULL


def test_option_checks_of_the_seams():
    assert _capi.check_threat_search(None) is None and _capi.check_threat_search(False) is None
    assert _capi.check_threat_search(True) == dict(max_depth=8, node_budget=256)
    assert _capi.check_threat_search({"max_depth": 4}) == dict(max_depth=4, node_budget=256)
    for bad in ({"max_depth": 0}, {"max_depth": 17}, {"node_budget": 0}, {"node_budget": 65536}, {"depth": 3}):
        with pytest.raises(ValueError):
            _capi.check_threat_search(bad)
    with pytest.raises(ValueError):
        _capi.check_threat_search(True, solver=False)
