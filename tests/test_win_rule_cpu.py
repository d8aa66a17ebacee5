"""The win rule (az_set_win_rule) without a GPU: the host scan az_rules_winner and the Gomoku class against the numpy
restatement in tests/win_rule.py, the default rule against the reference's golden vectors, brute-force minimax under both rules
(the small boards of the GPU tests can tell the rules apart), and the new symbols."""
import ctypes

import numpy as np
import pytest

from tests import forced, solver
from tests import win_rule as wr
from tests.util import SIZES, load

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi, constants
from alphazero_piskvorky_amd.games import Gomoku
from alphazero_piskvorky_amd.mcts import MCTS


def _random_board(rs, n, fill):
    return (rs.random_sample(n * n) < fill).astype(np.uint8) * rs.randint(1, 3, n * n).astype(np.uint8)


@pytest.mark.parametrize("n", range(3, 16))
def test_rules_winner_equals_the_scan(n):
    """random boards of every density, every k in 2..n, both rules; a board on which both colours hold a winning run is refused"""
    rs = np.random.RandomState(7 * n)
    seen = set()
    for k in range(2, n + 1):
        for i in range(12):
            board = _random_board(rs, n, (0.3, 0.6, 0.9, 1.0)[i % 4])
            for rule in wr.RULES:
                want = wr.winner_scan(board, n, k, rule)
                seen.add(want)
                if want < 0:
                    with pytest.raises(ValueError):
                        _capi.rules_winner(board, n, k, rule)
                else:
                    assert _capi.rules_winner(board, n, k, rule) == want, (n, k, rule, board.reshape(n, n))
                    assert _capi.rules_winner(board.reshape(n, n), n, k, wr.RULES.index(rule)) == want
    assert {0, 1, 2}.issubset(seen)


@pytest.mark.parametrize("n,k", [(5, 4), (9, 5), (15, 5), (6, 3)])
def test_rules_winner_along_playouts(n, k):
    """random play-outs: the scan after every move says what the last stone's test says, under both rules (a new winning run
    contains the new stone); under freestyle that test is tests.forced.wins_through"""
    rs = np.random.RandomState(n * 31 + k)
    for rule in wr.RULES:
        wins = forced.wins_through if rule == "freestyle" else wr.wins_exact
        ended = 0
        for _ in range(6):
            board, pl = np.zeros(n * n, np.uint8), 1
            for a in rs.permutation(n * n):
                board[a] = pl
                w = wins(board, int(a), n, k)
                got = _capi.rules_winner(board, n, k, rule)
                assert got == (pl if w else (3 if not (board == 0).any() else 0)), (rule, board.reshape(n, n))
                if got:
                    ended += 1
                    break
                pl = 3 - pl
        assert ended == 6


def test_crafted_cases():
    n, k = 9, 5
    row = np.zeros(n * n, np.uint8)
    row[9:15] = 1                                               # six in a row: an overline
    assert _capi.rules_winner(row, n, k, "freestyle") == 1 and _capi.rules_winner(row, n, k, "exact") == 0
    row[9 + 3 + 9 * np.arange(1, 5)] = 1                         # ... crossed by a column of exactly five through (1, 3)
    assert wr.run_through(row, 12, n, 1, 0) == 5
    assert _capi.rules_winner(row, n, k, "exact") == 1 and wr.winner_scan(row, n, k, "exact") == 1
    edge = np.zeros(n * n, np.uint8)
    edge[[4 + 9 * i for i in range(5)]] = 2                      # exactly five from the top edge
    assert _capi.rules_winner(edge, n, k, "exact") == 2
    full = np.array([1, 1, 2, 2, 2, 2, 1, 1, 1, 1, 2, 2, 2, 2, 1, 1], np.uint8)     # a full 4x4 whose longest run is two
    assert _capi.rules_winner(full, 4, 3, "exact") == _capi.rules_winner(full, 4, 3, "freestyle") == 3
    for bad in ((row, n, 0, "exact"), (row, n, n + 1, "exact"), (row[:-1], n, k, "exact"), (np.full(n * n, 3, np.uint8), n, k, "exact")):
        with pytest.raises(ValueError):
            _capi.rules_winner(*bad)
    with pytest.raises(ValueError):
        _capi.rules_winner(row, n, k, "renju")
    assert _capi.lib().az_rules_winner(None, n, k, 0) == -1 and _capi.lib().az_rules_winner(_capi._p(row), n, k, 2) == -1


@pytest.mark.parametrize("n,k", [(5, 3), (5, 4), (7, 4), (9, 5)])
def test_gomoku_exact_equals_the_scan(n, k):
    """Gomoku(win_rule="exact") along random play-outs and on the gap position; clone, rot90, flip and apply_action carry the rule"""
    rs = np.random.RandomState(n + 100 * k)
    names = {1: "X", 2: "O", 3: "D"}
    for _ in range(8):
        g = Gomoku(n, k, win_rule="exact")
        for a in rs.permutation(n * n):
            g = g.apply_action((int(a) // n, int(a) % n))
            assert g.win_rule == "exact" and g.clone().win_rule == g.rot90().win_rule == g.flip().win_rule == "exact"
            want = wr.winner_scan(g.cells, n, k, "exact")
            assert g.is_terminal() == (want != 0) and g.get_game_result() == names.get(want)
            if want:
                break
    board, player, last, gap = wr.gap_position(n, k)
    for rule, ends in (("exact", False), ("freestyle", True), (None, True)):
        g = Gomoku(n, k, win_rule=rule)
        g.cells = board.copy()
        g = g.apply_action((gap // n, gap % n))
        assert g.is_terminal() == ends and (g.get_game_result() == "X") == ends
    with pytest.raises(ValueError):
        Gomoku(n, k, win_rule="renju")


@pytest.mark.parametrize("n,k", SIZES)
def test_default_gomoku_is_the_reference(n, k):
    """the default rule against the reference's play-outs and crafted cases (tests/golden/rules_*.npz)"""
    assert constants.WIN_RULE == "freestyle" and Gomoku(n, k).win_rule == "freestyle"
    z = load(f"rules_{n}x{k}.npz")
    code = {None: 0, "X": 1, "O": 2, "D": 3}
    for acts, want in list(zip(z["actions"], z["result"]))[:8] + list(zip(z["crafted_actions"], z["crafted_result"])):
        g, first = Gomoku(n, k), 0
        for a in acts:
            if a < 0:
                break
            g = g.apply_action((int(a) // n, int(a) % n))
            if not first and g.is_terminal():
                first = code[g.get_game_result()]
        assert (first or code[g.get_game_result()]) == int(want)
        assert first == wr.replay(acts, n, k, "freestyle")[3]


def test_minimax_differs_between_the_rules(monkeypatch):
    """4x4 / k = 3 from the empty board: the values of 330 of the 19 837 positions both searches reach differ, so searches and
    proofs on the small boards can tell the rules apart"""
    n, k = 4, 3
    memo = {}
    for rule in wr.RULES:
        wr.use_rule(monkeypatch, rule)
        memo[rule] = {}
        solver.minimax(np.zeros(n * n, np.uint8), 1, n, k, memo[rule])
    shared = set(memo["freestyle"]) & set(memo["exact"])
    differ = sum(memo["freestyle"][key] != memo["exact"][key] for key in shared)
    print(f"shared {len(shared)}, differ {differ}")
    assert len(shared) == 19837 and differ == 330


def test_symbols_and_argument_errors():
    L = _capi.lib()
    for name in ("az_set_win_rule", "az_get_win_rule", "az_rules_winner"):
        assert name in _capi.EXPORTS and isinstance(getattr(L, name), ctypes._CFuncPtr)
    assert L.az_set_win_rule(None, 1) == -1 and L.az_get_win_rule(None) == -1
    assert _capi.WIN_RULES == {"freestyle": 0, "exact": 1}
    assert _capi.win_rule_id(None) == 0 and _capi.win_rule_id("exact") == 1 and _capi.win_rule_name(1) == "exact"
    for bad in ("renju", 2, -1, True, 1.5):
        with pytest.raises(ValueError):
            _capi.win_rule_id(bad)
    e = object.__new__(az.Engine)                               # no device: the rule's name is checked before the engine is touched
    with pytest.raises(ValueError):
        az.Engine.set_win_rule(e, "renju")
    assert callable(az.Engine.win_rule)
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    assert ModelEvaluator(win_rule="exact").win_rule == "exact" and ModelEvaluator().win_rule == "freestyle"
    assert SelfPlayManager(None, "cuda:0", win_rule="exact").win_rule == "exact"
    with pytest.raises(ValueError):
        SelfPlayManager(None, "cuda:0", win_rule="renju")
    m = MCTS(lambda s: (None, 0.0), 8, 2.0)
    with pytest.raises(ValueError, match="win rule"):
        m.run_many([Gomoku(5, 4), Gomoku(5, 4, win_rule="exact")], 1.0)
