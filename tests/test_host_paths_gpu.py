"""The engine's shared host paths and the seams' option module on the GPU: net_eval / net_eval_delta calls that take more than
one pass through the shared evaluation body (csrc/az_engine.hip: eval_positions), the Python conflict table held against the
engine's own (options.CONFLICTS vs g_conflicts), and options.apply_options on an engine that has already played under other
options.  Everything is compared exactly: floats as uint32 bit patterns, records with np.array_equal."""
import itertools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import options
from alphazero_piskvorky_amd.weights import synthetic_state_dict
from tests.test_delta_eval_gpu import N, K, _bits, _leaf, _oracle_rows, _root, _stack, _tiles
from tests.test_engine_edge_gpu import SETTINGS
from tests.util import weights_from_fixture

REC_KEYS = ("boards", "movers", "lasts", "visits", "pis", "actions", "z")


def _assert_rows(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("logits", "P", "value")):
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: {name}"


def _assert_oracle(got, oracle, what):
    for i, (ol, oP, ov) in enumerate(oracle):
        row = (got[0][i], got[1][i], got[2][i:i + 1])
        _assert_rows(row, (ol, oP, np.float32(ov).reshape(1)), f"{what}, position {i} against the oracle")


def _episode(e, G, seed0, cut=0):
    e.selfplay(G, seed0=seed0, max_plies=cut)
    return e.records(), e.games()


def _assert_same_episode(a, b, what):
    for key in REC_KEYS:
        assert np.array_equal(a[0][key], b[0][key]), f"{what}: {key}"
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]), f"{what}: games"


# ---------------------------------------------------------------------------------------------------------------------
# more than one pass through the shared evaluation body
# ---------------------------------------------------------------------------------------------------------------------
def test_net_eval_in_several_passes_equals_single_calls_and_the_oracle():
    """5 positions on 2 slots: passes of 2, 2, 1; with two leaves per batch the lane has 4 evaluation items: passes of 4, 1"""
    n, k = 5, 4
    sd = weights_from_fixture(n, "seeded")
    o, onet = orc.Oracle(n, k, 1), orc.Net(n, sd)
    rs = np.random.RandomState(505)
    pos = []
    for stones in (0, 1, 4, 7, 12):
        b = np.zeros(n * n, np.uint8)
        cells = [int(c) for c in rs.permutation(n * n)[:stones]]
        for j, c in enumerate(cells):
            b[c] = 1 + j % 2
        pos.append((b, 1 + stones % 2, cells[-1] if cells else -1))
    boards, players, lasts = _stack(pos)
    oracle = [onet.eval(o.encode(b, int(p), int(l))) for b, p, l in pos]
    e = az.Engine(n, k, 4, 2, engines=1, model="plain")
    e.load_weights(sd, 0)
    try:
        for what in ("2 slots", "2 slots x 2 leaves per batch"):
            got = e.net_eval(boards, players, lasts)
            for i in range(len(pos)):
                one = e.net_eval(boards[i:i + 1], players[i:i + 1], lasts[i:i + 1])
                _assert_rows((got[0][i:i + 1], got[1][i:i + 1], got[2][i:i + 1]), one, f"{what}, position {i} against its own call")
            _assert_oracle(got, oracle, what)
            e.set_virtual_loss(2)
            assert e.ext_capacity() == 4
    finally:
        e.close()


def test_net_eval_delta_in_several_passes_and_the_lane_afterwards():
    """5 leaves of a three-stone root on 2 slots of the plain 15x15 net: passes of 2, 2, 1 (the delta tests' own calls fit into
    one pass).  Rows as net_eval's and the oracle's, the reported path per leaf, and the episode that follows is the one a
    fresh engine plays: the slots were left idle and empty."""
    sd = synthetic_state_dict(N)
    o, onet = orc.Oracle(N, K, 1), orc.Net(N, sd)
    root = _root([7 * N + 7, 7 * N + 8, 3 * N + 2])
    cells = [[6 * N + 6], [0], [N * N - 1, 7 * N + 6], [8 * N + 8, 14 * N], [11 * N + 12]]
    leaves = [_leaf(root, cs) for cs in cells]
    boards, players, lasts = _stack(leaves)
    G, S, seed0, cut = 2, 4, 9150, 3
    e = az.Engine(N, K, S, 2, engines=1, model="plain", log_table=orc.numpy_log_table(S))
    fresh = az.Engine(N, K, S, 2, engines=1, model="plain", log_table=orc.numpy_log_table(S))
    try:
        e.load_weights(sd, 0)
        fresh.load_weights(sd, 0)
        got = e.net_eval_delta(root[0], root[1], boards, players, lasts)
        _assert_rows(got, e.net_eval(boards, players, lasts), "against net_eval")
        _assert_oracle(got, _oracle_rows(onet, o, leaves), "net_eval_delta")
        assert got[3].tolist() == [_tiles(cs) for cs in cells], "path taken"
        e.net_eval_delta(root[0], root[1], boards, players, lasts)          # the last call before the episode is the delta one
        _assert_same_episode(_episode(e, G, seed0, cut), _episode(fresh, G, seed0, cut), "self-play after the evaluation calls")
    finally:
        e.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# options.CONFLICTS against the engine's table
# ---------------------------------------------------------------------------------------------------------------------
# the seams' option names -> how tests/test_engine_edge_gpu.py switches the engine's setting on
ENGINE_SETTING = {"subtree_reuse": "reuse", "virtual_loss": "virtual loss", "leaf_symmetry": "leaf symmetry", "evaluator": "external evaluator",
                  "playout_cap": "playout cap", "forced_playouts": "forced playouts", "gumbel": "gumbel", "solver": "solver"}


def _option_engine():
    S = 8
    return az.Engine(5, 4, S, 2, log_table=orc.numpy_log_table(S))      # no weights: no setter asks for them


def test_the_python_table_names_exactly_the_pairs_the_engine_refuses():
    pairs = {frozenset((a, b)) for a, b, _ in options.CONFLICTS}
    assert len(pairs) == len(options.CONFLICTS) == 15 and all(len(p) == 2 and p <= set(ENGINE_SETTING) for p in pairs)
    for a, b in itertools.combinations(ENGINE_SETTING, 2):
        refused = frozenset((a, b)) in pairs
        for first, second in ((a, b), (b, a)):
            e = _option_engine()
            try:
                SETTINGS[ENGINE_SETTING[first]][0](e)
                if refused:
                    with pytest.raises(az.AzError, match=re.escape("(-1)")):
                        SETTINGS[ENGINE_SETTING[second]][0](e)
                else:
                    SETTINGS[ENGINE_SETTING[second]][0](e)          # not in the table: the engine takes both
            finally:
                e.close()
    # the one rule of NEEDS
    e = _option_engine()
    try:
        with pytest.raises(az.AzError, match=re.escape("(-1)")):
            e.set_threat_search(4, 64)
        e.set_solver(True)
        e.set_threat_search(4, 64)
        with pytest.raises(az.AzError, match=re.escape("(-1)")):
            e.set_solver(False)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# apply_options on a used engine
# ---------------------------------------------------------------------------------------------------------------------
def test_apply_options_brings_a_used_engine_to_the_state_of_a_fresh_one():
    n, k, S, G, seed0 = 5, 4, 8, 4, 4711
    sd = weights_from_fixture(n, "seeded")
    start = np.zeros((2, n * n), np.uint8)
    start[0, 12], start[0, 6] = 1, 2
    start[1, 0] = 1
    start_positions = (start, np.array([1, 2], np.uint8), np.array([6, 0], np.int16))
    A = dict(win_rule="exact", start_positions=start_positions, first=1, resign={"threshold": 0.5, "min_ply": 2, "playout": 0.25},
             playout_cap=None, forced_playouts=None, gumbel=None, solver=True, threat_search={"max_depth": 4, "node_budget": 64})
    B = dict(win_rule="freestyle", start_positions=None, first=0, resign=None,
             playout_cap={"fast_sims": 4, "full": 0.5, "train_on_fast": False}, forced_playouts=None,
             gumbel={"m": 4, "c_visit": 50.0, "c_scale": 1.0}, solver=False, threat_search=None)

    def engine():
        e = az.Engine(n, k, S, 4, log_table=orc.numpy_log_table(S))
        e.load_weights(sd, 0)
        return e

    def episode(e):
        e.selfplay(G, seed0=seed0)
        return e.records(), e.games(), e.values(), e.proofs(), e.threats()

    used, fresh = engine(), engine()
    try:
        options.apply_options(used, **A)
        first = episode(used)
        options.apply_options(used, **B)
        assert used.gumbel()["m"] == 4 and used.playout_cap()["fast_sims"] == 4 and used.win_rule() == "freestyle"
        assert not used.solver() and used.threat_search()[0] == 0 and used.start_positions() == 0 and used.resign()["threshold"] == 0.0
        used.selfplay(G, seed0=seed0)
        options.apply_options(used, **A)
        assert used.gumbel()["m"] == 0 and used.playout_cap()["fast_sims"] == 0 and used.win_rule() == "exact"
        assert used.solver() and used.threat_search() == (4, 64) and used.start_positions() == 2
        again = episode(used)
        options.apply_options(fresh, **A)
        want = episode(fresh)
        for got, what in ((first, "A on the new engine"), (again, "A after B")):
            _assert_same_episode(got, want, what)
            assert np.array_equal(_bits(got[2]), _bits(want[2])), f"{what}: values"
            assert np.array_equal(got[3], want[3]), f"{what}: proofs"
            assert np.array_equal(got[4], want[4]), f"{what}: threats"
    finally:
        used.close()
        fresh.close()
