"""Start positions, the parts that need no GPU: the action-list helper of games.py, the binding's argument checks, and the
C ABI declaring what the binding calls."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests.util import ROOT

from alphazero_piskvorky_amd import _capi, games
from alphazero_piskvorky_amd.evaluator import ModelEvaluator
from alphazero_piskvorky_amd.parallel import arena_block
from alphazero_piskvorky_amd.self_play import SelfPlayManager


def test_position_from_actions_is_the_oracles_replay():
    n, k = 6, 4
    o = orc.Oracle(n, k, 1)
    rs = np.random.RandomState(5)
    for stones in (0, 1, 2, 7, 12):
        acts = [int(a) for a in rs.permutation(n * n)[:stones]]
        rc, _, board, pl, _ = o.replay(acts)
        assert rc == 0
        cells, player, last = games.position_from_actions(acts, n)
        assert cells.dtype == np.uint8 and np.array_equal(cells, board) and player == pl
        assert last == (acts[-1] if acts else -1)
        # (r, c) pairs are the same actions
        cells2, player2, last2 = games.position_from_actions([(a // n, a % n) for a in acts], n)
        assert np.array_equal(cells2, cells) and (player2, last2) == (player, last)
        # O first: the colours exchanged, the arena's odd games
        cells3, player3, last3 = games.position_from_actions(acts, n, first_player=2)
        assert np.array_equal(cells3, (3 - cells) * (cells != 0)) and player3 == 3 - player and last3 == last


def test_position_from_actions_refuses_what_the_rules_refuse():
    with pytest.raises(ValueError, match="Invalid move"):
        games.position_from_actions([3, 4, 3], 5)
    with pytest.raises(ValueError, match="Invalid move"):
        games.position_from_actions([25], 5)
    with pytest.raises(ValueError, match="Invalid move"):
        games.position_from_actions([-1], 5)
    with pytest.raises(ValueError, match="first_player"):
        games.position_from_actions([], 5, first_player=0)


def test_positions_from_actions_gives_the_arrays_the_engine_takes():
    n = 5
    boards, players, lasts = games.positions_from_actions([[], [12], [12, 7, 0]], n)
    assert boards.shape == (3, n * n) and boards.dtype == np.uint8
    assert players.dtype == np.uint8 and players.tolist() == [1, 2, 2]
    assert lasts.dtype == np.int16 and lasts.tolist() == [-1, 12, 0]
    assert boards[2].nonzero()[0].tolist() == [0, 7, 12] and boards[2][[12, 7, 0]].tolist() == [1, 2, 1]


def test_header_declares_the_setter_and_the_binding_exports_it():
    text = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    assert re.search(r"int az_set_start_positions\(az_engine \*e, int count, const uint8_t \*boards[^;]*"
                     r"const uint8_t \*players, const int16_t \*lasts, int64_t first\);", text)
    assert "int az_get_start_positions(const az_engine *e);" in text
    assert {"az_set_start_positions", "az_get_start_positions"} <= set(_capi.EXPORTS)
    # the ctypes contract of the episode calls is untouched: the setting is an engine option, not an argument
    assert [f for f, _ in _capi.az_selfplay_args._fields_] == ["seed0", "num_games", "max_plies", "temperature_table",
                                                               "noise_tape", "u_tape", "tape_stride"]
    assert [f for f, _ in _capi.az_arena_args._fields_] == ["seed0", "num_games", "temperature_table", "u_tape"]


def test_the_seams_take_the_option_and_arena_blocks_never_tear_a_pair():
    pos = games.positions_from_actions([[12], [12, 7]], 5)
    m = SelfPlayManager(controller=None, device="cuda:0", start_positions=pos)
    assert m.start_positions is pos and SelfPlayManager(None, "cuda:0").start_positions is None
    ev = ModelEvaluator(device="cuda:0", start_positions=pos)
    assert ev.start_positions is pos and ModelEvaluator(device="cuda:0").start_positions is None
    # games 2i and 2i+1 are one position from both sides: every rank's first game id is even
    for num_games in (1, 7, 20, 51):
        for world in (1, 2, 3, 8):
            assert all(arena_block(num_games, r, world)[0] % 2 == 0 or arena_block(num_games, r, world)[0] == num_games
                       for r in range(world))
