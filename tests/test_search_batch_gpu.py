"""az_search_batch on the GPU: every position of every batch against the oracle's restatement of one search (orc_search) and
against a loop of az_search on the same engine, bit for bit (array_equal, no tolerances), plus the call's contract and the
MCTS.run_many shim."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.util import load, weights_from_fixture, build_weights

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi, games, net
from alphazero_piskvorky_amd.controller import NeuralNetworkController, make_policy_value_fn
from alphazero_piskvorky_amd.mcts import MCTS
from alphazero_piskvorky_amd.net import fold_resnet_state_dict
from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict

RES_NONE = 0
TEMPS = [1.0, 0.5, 1e-8, 0.05, 1e-7, 2.0, 0.3]          # per-position temperatures, two of them on the float32 path (<= 1e-7)
KEYS = ("N", "W", "P", "pi")


def _fixture_positions(name):
    z = load(name)
    return [(z["board"][i].astype(np.uint8), int(z["player"][i]), int(z["last"][i])) for i in range(len(z["ply"]))]


def _random_positions(rs, n, k, count, max_stones=None):
    """undecided positions reached by legal play, checked with the oracle's rules: result RES_NONE, at least one empty cell"""
    o = orc.Oracle(n, k, 1)
    nn = n * n
    out = []
    while len(out) < count:
        stones = int(rs.randint(0, (max_stones or nn - 1) + 1))
        acts = [int(a) for a in rs.permutation(nn)[:stones]]
        rc, term, board, pl, res = o.replay(acts)
        if rc == 0 and res == RES_NONE and not term.any() and (board == 0).any():
            out.append((board.copy(), int(pl), acts[-1] if acts else -1))
    return out


def _positions(n, k, count, fixtures, seed):
    """fixture positions first, topped up with random undecided ones"""
    pos = []
    for f in fixtures:
        pos += _fixture_positions(f)
    pos = pos[:count]
    if len(pos) < count:
        pos += _random_positions(np.random.RandomState(seed), n, k, count - len(pos))
    return pos


def _draws(pos, seed, with_noise):
    rs = np.random.RandomState(seed)
    noise = [rs.dirichlet([0.3] * int((b == 0).sum())) for b, _, _ in pos]
    us = [float(rs.random_sample()) for _ in pos]
    Ts = [TEMPS[i % len(TEMPS)] for i in range(len(pos))]
    return (noise if with_noise else None), us, Ts


def _oracle_searches(o, onet, pos, noise, us, Ts, game=0):
    def one(i):
        b, pl, la = pos[i]
        return o.search(onet, b, pl, la, Ts[i], None if noise is None else noise[i], us[i], game=game)
    with ThreadPoolExecutor(max_workers=16) as ex:
        return list(ex.map(one, range(len(pos))))


def _batch(e, pos, noise, us, Ts, lo=0, hi=None, slot=0):
    hi = len(pos) if hi is None else hi
    sel = range(lo, hi)
    return e.search_batch(np.stack([pos[i][0] for i in sel]), [pos[i][1] for i in sel], [pos[i][2] for i in sel],
                          [Ts[i] for i in sel], None if noise is None else [noise[i] for i in sel], [us[i] for i in sel], slot=slot)


def _assert_equal(r, refs, what):
    """every position of the batch, every output"""
    assert len(r["action"]) == len(refs)
    for i, ref in enumerate(refs):
        for key in KEYS:
            assert np.array_equal(r[key][i], ref[key]), f"{what}: position {i}: {key} differs"
        assert int(r["action"][i]) == int(ref["action"]), f"{what}: position {i}: action differs"


def _loop(e, pos, noise, us, Ts, slot=0):
    return [e.search(pos[i][0], pos[i][1], pos[i][2], Ts[i], None if noise is None else noise[i], us[i], slot=slot)
            for i in range(len(pos))]


# ---------------------------------------------------------------------------------------------------------------------
# versus the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [False, True])
def test_5x5_real_checkpoint_every_count_and_lane_number_vs_oracle(with_noise):
    n, k, S, slots = 5, 4, 100, 64
    sd = weights_from_fixture(n, "ckpt_saved")
    pos = _positions(n, k, 2 * slots + 3, ["netgame_5x4.npz", "netgame_confident_5x4.npz"], seed=31)
    noise, us, Ts = _draws(pos, 7, with_noise)
    refs = _oracle_searches(orc.Oracle(n, k, S), orc.Net(n, sd), pos, noise, us, Ts)
    for lanes in (1, 4):
        e = az.Engine(n, k, S, slots, log_table=orc.numpy_log_table(S), engines=lanes)
        assert e.lanes() == lanes
        e.load_weights(sd, 0)
        for count in (1, 7, slots, 2 * slots + 3):
            lo = 0 if count == 2 * slots + 3 else 11            # different windows of the position list
            r = _batch(e, pos, noise, us, Ts, lo, lo + count)
            _assert_equal(r, refs[lo:lo + count], f"lanes {lanes}, count {count}")
            c = e.counters()
            assert c["simulations"] == count * S and c["root_evals"] == count and c["plies"] == count
        assert e.persistent() > 0
        e.close()


@pytest.mark.parametrize("with_noise", [False, True])
def test_9x9_seeded_net_150_positions_on_64_slots_vs_oracle(with_noise):
    n, k, S = 9, 5, 64
    sd = weights_from_fixture(n, "seeded")
    pos = _positions(n, k, 150, ["netgame_9x5.npz", "netgame_full_9x5.npz"], seed=32)
    noise, us, Ts = _draws(pos, 8, with_noise)
    refs = _oracle_searches(orc.Oracle(n, k, S), orc.Net(n, sd), pos, noise, us, Ts)
    e = az.Engine(n, k, S, 64, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    _assert_equal(_batch(e, pos, noise, us, Ts), refs, "9x9")
    assert e.persistent() == 0
    e.close()


@pytest.mark.parametrize("with_noise", [False, True])
def test_15x15_seeded_net_every_ply_of_the_fixture_game_on_16_slots_vs_oracle(with_noise):
    n, k, S = 15, 5, 100
    sd = weights_from_fixture(n, "seeded")
    pos = _fixture_positions("netgame_complete_15x5.npz")
    assert len(pos) == 46
    noise, us, Ts = _draws(pos, 9, with_noise)
    refs = _oracle_searches(orc.Oracle(n, k, S), orc.Net(n, sd), pos, noise, us, Ts)
    e = az.Engine(n, k, S, 16, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    _assert_equal(_batch(e, pos, noise, us, Ts), refs, "15x15")
    e.close()


@pytest.mark.parametrize("with_noise", [False, True])
def test_15x15_synthetic_evaluator_300_positions_on_128_slots_vs_oracle(with_noise):
    n, k, S = 15, 5, 100
    pos = _positions(n, k, 300, ["netgame_complete_15x5.npz", "netgame_full_15x5.npz", "netgame_15x5.npz"], seed=33)
    noise, us, Ts = _draws(pos, 10, with_noise)
    refs = _oracle_searches(orc.Oracle(n, k, S, synthetic=True), None, pos, noise, us, Ts)
    e = az.Engine(n, k, S, 128, synthetic=True, log_table=orc.numpy_log_table(S))
    _assert_equal(_batch(e, pos, noise, us, Ts), refs, "15x15 synthetic")
    c = e.counters()
    assert c["simulations"] == 300 * S and c["root_evals"] == 300 and c["plies"] == 300
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# versus a loop of Engine.search on the same engine
# ---------------------------------------------------------------------------------------------------------------------
SMALL = dict(n=5, k=4, S=60, slots=16, count=37, fixtures=["netgame_5x4.npz"])
LARGE = dict(n=15, k=5, S=40, slots=8, count=19, fixtures=["netgame_complete_15x5.npz"])


def _case(cfg, seed=41):
    pos = _positions(cfg["n"], cfg["k"], cfg["count"], cfg["fixtures"], seed)
    noise, us, Ts = _draws(pos, seed + 1, True)
    return pos, noise, us, Ts


def _plain_engine(cfg, S=None, **kw):
    S = cfg["S"] if S is None else S
    e = az.Engine(cfg["n"], cfg["k"], S, cfg["slots"], log_table=orc.numpy_log_table(S), **kw)
    if not kw.get("synthetic") and kw.get("model", "plain") == "plain":
        e.load_weights(weights_from_fixture(cfg["n"], "ckpt_saved" if cfg["n"] == 5 else "seeded"), 0)
    return e


@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["5x5", "15x15"])
def test_virtual_loss_batching_equals_the_loop_of_search(cfg):
    pos, noise, us, Ts = _case(cfg)
    e = _plain_engine(cfg)
    e.set_virtual_loss(8)
    _assert_equal(_batch(e, pos, noise, us, Ts), _loop(e, pos, noise, us, Ts), "virtual loss 8")
    e.close()


@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["5x5", "15x15"])
def test_subtree_reuse_setting_leaves_batch_and_loop_of_search_equal(cfg):
    """every search starts from a fresh root whatever az_set_subtree_reuse says: with the setting on, the batch still
    returns what the loop of search returns on the same engine, and pi and the action are those of the setting off"""
    pos, noise, us, Ts = _case(cfg)
    e = _plain_engine(cfg)
    off = _batch(e, pos, noise, us, Ts)
    e.set_subtree_reuse(True)
    r = _batch(e, pos, noise, us, Ts)
    _assert_equal(r, _loop(e, pos, noise, us, Ts), "subtree reuse on")
    assert np.array_equal(r["pi"], off["pi"]) and np.array_equal(r["action"], off["action"])
    e.close()


@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["5x5", "15x15"])
def test_evaluation_cache_equals_the_loop_of_search_and_hits_on_a_repeated_position(cfg):
    pos, noise, us, Ts = _case(cfg)
    pos[5] = pos[2]; noise[5] = noise[2]; us[5] = us[2]; Ts[5] = Ts[2]           # a repeated position
    e = _plain_engine(cfg)
    e.set_eval_cache(1 << 14)
    r = _batch(e, pos, noise, us, Ts)
    assert e.counters()["cache_hits"] > 0
    for key in KEYS:
        assert np.array_equal(r[key][5], r[key][2])
    _assert_equal(r, _loop(e, pos, noise, us, Ts), "cache")
    e.set_eval_cache(0)
    _assert_equal(r, _loop(e, pos, noise, us, Ts), "cache on vs off")
    e.close()


@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["5x5", "15x15"])
def test_leaf_symmetry_key_is_zero_for_every_position(cfg):
    pos, noise, us, Ts = _case(cfg)
    last = len(pos) - 1
    pos[last] = pos[1]; noise[last] = noise[1]; us[last] = us[1]; Ts[last] = Ts[1]     # the same position at two indices
    e = _plain_engine(cfg)
    e.set_leaf_symmetry(True)
    r = _batch(e, pos, noise, us, Ts)
    for key in KEYS:
        assert np.array_equal(r[key][last], r[key][1])
    assert int(r["action"][last]) == int(r["action"][1])
    _assert_equal(r, _loop(e, pos, noise, us, Ts), "leaf symmetry")
    sd = weights_from_fixture(cfg["n"], "ckpt_saved" if cfg["n"] == 5 else "seeded")
    refs = _oracle_searches(orc.Oracle(cfg["n"], cfg["k"], cfg["S"], leaf_sym=True), orc.Net(cfg["n"], sd), pos, noise, us, Ts, game=0)
    _assert_equal(r, refs, "leaf symmetry vs Oracle(leaf_sym=True).search(game=0)")
    e.close()


@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["5x5", "15x15"])
def test_slot_1_searches_with_the_baseline_net(cfg):
    pos, noise, us, Ts = _case(cfg)
    e = _plain_engine(cfg)
    e.load_weights(build_weights(cfg["n"], seed=77), 1)
    r0 = _batch(e, pos, noise, us, Ts, slot=0)
    r1 = _batch(e, pos, noise, us, Ts, slot=1)
    assert not np.array_equal(r0["P"], r1["P"])                         # the two slots hold different nets
    _assert_equal(r1, _loop(e, pos, noise, us, Ts, slot=1), "slot 1")
    _assert_equal(_batch(e, pos, noise, us, Ts, slot=0), _loop(e, pos, noise, us, Ts, slot=0), "slot 0 after slot 1")
    e.close()


@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["5x5", "15x15"])
def test_resnet_model_equals_the_loop_of_search(cfg):
    pos, noise, us, Ts = _case(cfg)
    e = _plain_engine(cfg, model="resnet")
    e.load_weights(synthetic_resnet_state_dict(cfg["n"]), 0)
    _assert_equal(_batch(e, pos, noise, us, Ts), _loop(e, pos, noise, us, Ts), "resnet")
    e.close()


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["5x5", "15x15"])
def test_emulated_trunks_equal_the_loop_of_search(cfg, mode):
    pos, noise, us, Ts = _case(cfg)
    e = _plain_engine(cfg)
    e.set_trunk_mode(mode)
    _assert_equal(_batch(e, pos, noise, us, Ts), _loop(e, pos, noise, us, Ts), mode)
    e.close()


@pytest.mark.parametrize("cfg", [dict(SMALL, slots=8, count=11), dict(LARGE, slots=4, count=6)], ids=["5x5", "15x15"])
def test_deep_engine_at_1600_simulations_equals_the_loop_of_search(cfg):
    pos, noise, us, Ts = _case(cfg)
    e = _plain_engine(cfg, S=1600, deep=True)
    r = _batch(e, pos, noise, us, Ts)
    assert int(r["N"].max()) > 0 and (r["N"].sum(axis=1) == 1600).all()
    _assert_equal(r, _loop(e, pos, noise, us, Ts), "deep")
    assert e.persistent() == 0
    e.close()


def test_persistent_kernel_serves_small_boards_only():
    pos, noise, us, Ts = _case(SMALL)
    e = _plain_engine(SMALL)
    r = _batch(e, pos, noise, us, Ts)
    assert e.persistent() > 0
    _assert_equal(r, _loop(e, pos, noise, us, Ts), "persistent")
    e.close()
    cfg = dict(n=9, k=5, S=30, slots=8, count=12, fixtures=["netgame_9x5.npz"])
    pos, noise, us, Ts = _case(cfg)
    e = _plain_engine(cfg)
    r = _batch(e, pos, noise, us, Ts)
    assert e.persistent() == 0
    _assert_equal(r, _loop(e, pos, noise, us, Ts), "9x9 lock-step")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# contract
# ---------------------------------------------------------------------------------------------------------------------
def _raw_call(e, boards, players, lasts, T, u, outs):
    return _capi.lib().az_search_batch(e.h, 0, len(players), _capi._p(boards), _capi._p(players), _capi._p(lasts), _capi._p(T),
                                       None, _capi._p(u), *[_capi._p(o) for o in outs])


@pytest.mark.parametrize("fault", ["last_on_empty_cell", "cell_value_3", "full_board"])
def test_invalid_position_in_the_middle_names_its_index_and_writes_nothing(fault):
    n, nn = 5, 25
    e = az.Engine(n, 4, 16, 8, synthetic=True)
    cnt, bad = 6, 3
    boards = np.zeros((cnt, nn), np.uint8); boards[:, 4] = 1
    players = np.full(cnt, 2, np.uint8); lasts = np.full(cnt, 4, np.int16)
    if fault == "last_on_empty_cell":
        lasts[bad] = 9
    elif fault == "cell_value_3":
        boards[bad, 7] = 3
    else:
        boards[bad] = 1 + (np.arange(nn) & 1)
    T = np.ones(cnt); u = np.full(cnt, 0.5)
    outs = [np.full((cnt, nn), 7, np.float32), np.full(cnt, 7, np.int32), np.full((cnt, nn), 7, np.int32),
            np.full((cnt, nn), 7.0, np.float64), np.full((cnt, nn), 7, np.float32)]
    rc = _raw_call(e, boards, players, lasts, T, u, outs)
    assert rc == -1                                                          # AZ_ERR_INVALID
    assert f"position {bad}" in _capi.lib().az_last_error(e.h).decode()
    assert all((o == 7).all() for o in outs)
    with pytest.raises(az.AzError, match=rf"az_search_batch failed \(-1\).*position {bad}"):
        e.search_batch(boards, players, lasts, T, None, u)
    players[1] = 3
    assert _raw_call(e, boards, players, lasts, T, u, outs) == -1 and "position 1" in _capi.lib().az_last_error(e.h).decode()
    e.close()


def test_argument_and_state_contract():
    n, nn, S = 5, 25, 16
    e = az.Engine(n, 4, S, 8, synthetic=True)
    L = _capi.lib()
    b = np.zeros((2, nn), np.uint8); p = np.ones(2, np.uint8); la = np.full(2, -1, np.int16); T = np.ones(2); u = np.full(2, 0.5)
    P = _capi._p
    assert L.az_search_batch(e.h, 0, 0, None, None, None, None, None, None, None, None, None, None, None) == 0     # count = 0
    assert L.az_search_batch(e.h, 0, -1, P(b), P(p), P(la), P(T), None, P(u), None, None, None, None, None) == -1
    assert L.az_search_batch(e.h, 2, 2, P(b), P(p), P(la), P(T), None, P(u), None, None, None, None, None) == -1
    for hole in range(5):
        args = [P(b), P(p), P(la), P(T), None, P(u)]
        args[hole if hole < 4 else 5] = None
        assert L.az_search_batch(e.h, 0, 2, *args, None, None, None, None, None) == -1
    assert L.az_search_batch(e.h, 0, 2, P(b), P(p), P(la), P(T), None, P(u), None, None, None, None, None) == 0    # all outputs NULL
    # an open episode refuses the call; afterwards a batch forgets the episode
    e.selfplay_begin(4, seed0=5)
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.search_batch(b, p, la, 1.0)
    e.selfplay_end()
    e.records()
    r = e.search_batch(b, p, la, 1.0)
    assert (r["N"].sum(axis=1) == S).all()
    c = e.counters()
    assert c["simulations"] == 2 * S and c["root_evals"] == 2 and c["plies"] == 2
    with pytest.raises(az.AzError, match=r"az_selfplay_records failed \(-6\)"):
        e.records()
    e.close()
    # the net evaluator without weights
    e = az.Engine(n, 4, S, 8)
    with pytest.raises(az.AzError, match=r"\(-5\)"):
        e.search_batch(b, p, la, 1.0)
    e.close()


@pytest.mark.parametrize("n,k,lanes", [(5, 4, 1), (9, 5, 2)])
def test_selfplay_after_a_batch_equals_selfplay_on_a_fresh_engine(n, k, lanes):
    S, G = 24, 6
    sd = weights_from_fixture(n, "seeded")

    def episode(e):
        e.selfplay(G, seed0=60, max_plies=6)
        rec = e.records(); nply, res = e.games()
        return rec, nply, res

    fresh = az.Engine(n, k, S, 8, log_table=orc.numpy_log_table(S), engines=lanes)
    fresh.load_weights(sd, 0); fresh.set_leaf_symmetry(True)
    want = episode(fresh)
    fresh.close()
    e = az.Engine(n, k, S, 8, log_table=orc.numpy_log_table(S), engines=lanes)
    e.load_weights(sd, 0); e.set_leaf_symmetry(True)
    pos = _random_positions(np.random.RandomState(3), n, k, 13)
    noise, us, Ts = _draws(pos, 4, True)
    _batch(e, pos, noise, us, Ts)
    got = episode(e)
    for key in want[0]:
        assert np.array_equal(got[0][key], want[0][key]), key
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    # and a single search after the batch is still the single search
    b, pl, la = pos[0]
    r = e.search(b, pl, la, 0.8, noise[0], 0.4)
    ro = orc.Oracle(n, k, S, leaf_sym=True).search(orc.Net(n, sd), b, pl, la, 0.8, noise[0], 0.4, game=0)
    assert np.array_equal(r["N"], ro["N"]) and np.array_equal(r["pi"], ro["pi"]) and r["action"] == ro["action"]
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# MCTS.run_many
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("add_noise", [False, True])
def test_run_many_equals_the_loop_of_run_after_the_same_seed(add_noise):
    n, k = 5, 4
    m = net.GomokuNet(board_size=n)
    m.load_state_dict({kk: torch.tensor(v) for kk, v in weights_from_fixture(n, "ckpt_saved").items()})
    m.eval()
    pvf = make_policy_value_fn(NeuralNetworkController(m, device="cuda:0"))
    states = []
    for b, pl, la in _fixture_positions("netgame_confident_5x4.npz")[:40]:
        s = games.Gomoku(n, k)
        s.cells = b.copy(); s.current_player = "X" if pl == 1 else "O"
        s.last_action = None if la < 0 else (la // n, la % n)
        states.append(s)
    assert len(states) == 40
    temps = [TEMPS[i % len(TEMPS)] for i in range(40)]
    mc = MCTS(pvf, num_simulations=50, c_puct=2.0)
    np.random.seed(3)
    want, want_visits = [], []
    for s, T in zip(states, temps):
        want.append(mc.run(s, T, add_root_noise=add_noise))
        want_visits.append(mc.last_visits.copy())
    np.random.seed(3)
    got = mc.run_many(states, temps, add_root_noise=add_noise)
    assert len(got) == 40
    for i in range(40):
        assert got[i][1] == want[i][1], f"state {i}: move"
        assert np.array_equal(got[i][0], want[i][0]), f"state {i}: pi"
        assert np.array_equal(mc.last_visits[i], want_visits[i]), f"state {i}: visits"
    assert mc.last_visits.shape == (40, n, n)
    assert mc._batch_engine.slots == 64
    # a scalar temperature, and the engine grows with a larger batch
    np.random.seed(5)
    want = [mc.run(s, 0.6, add_root_noise=add_noise) for s in states]
    np.random.seed(5)
    got = mc.run_many(states * 2, 0.6, add_root_noise=add_noise)[:40]
    assert mc._batch_engine.slots == 128
    for i in range(40):
        assert got[i][1] == want[i][1] and np.array_equal(got[i][0], want[i][0])
