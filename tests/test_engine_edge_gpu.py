"""GPU edge cases and full-size invariants for the HIP engine (C-ABI), against the oracle or by size-independent properties."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.util import weights_from_fixture

import alphazero_piskvorky_amd as az


def _engine(n, k, S, slots=4, synthetic=False, **kw):
    return az.Engine(n, k, S, slots, synthetic=synthetic, log_table=orc.numpy_log_table(S), **kw)


def _random_position(rs, n, k, stones):
    """Random non-terminal position reached by legal play (oracle rules)."""
    o = orc.Oracle(n, k, 1)
    while True:
        acts = list(rs.permutation(n * n)[:stones])
        rc, term, board, pl, res = o.replay(acts)
        if rc == 0 and res == 0 and not term.any():
            return board, pl, (acts[-1] if acts else -1)


@pytest.mark.parametrize("T", [1e-8, 1e-7, 3e-7, 5.0])
def test_temperature_extremes_match_oracle(T):
    """T <= 1e-7 takes numpy's float32 path after the clip (mcts.py:156-157); large T flattens pi."""
    n, k, S = 9, 5, 60
    rs = np.random.RandomState(11)
    e = _engine(n, k, S, synthetic=True)
    o = orc.Oracle(n, k, S, synthetic=True)
    for stones in (0, 7, 30):
        board, pl, last = _random_position(rs, n, k, stones)
        for u in (0.0, 0.37, 0.999999):
            r = e.search(board, pl, last, T, None, u)
            ro = o.search(None, board, pl, last, T, None, u)
            assert np.array_equal(r["N"], ro["N"]) and r["action"] == ro["action"]
            assert np.array_equal(r["pi"], ro["pi"])
            assert abs(float(r["pi"].sum()) - 1.0) < 1e-5
    e.close()


def test_nearly_full_boards_terminal_leaves_and_draws():
    """Searches near the end of 5x5 games walk into terminal leaves (wins and full-board draws, mcts.py:132-134)."""
    n, k, S = 5, 4, 80
    rs = np.random.RandomState(5)
    e = _engine(n, k, S, synthetic=True)
    o = orc.Oracle(n, k, S, synthetic=True)
    seen = 0
    for stones in (18, 20, 22, 23, 24):
        for _ in range(4):
            board, pl, last = _random_position(rs, n, k, stones)
            A = n * n - stones
            noise = rs.dirichlet([0.3] * A)
            r = e.search(board, pl, last, 0.8, noise, 0.5)
            ro = o.search(None, board, pl, last, 0.8, noise, 0.5)
            assert np.array_equal(r["N"], ro["N"]) and np.array_equal(r["W"], ro["W"]) and r["action"] == ro["action"]
            assert r["N"].sum() == S and (r["N"][board != 0] == 0).all()
            seen += 1
    assert seen == 20
    e.close()


@pytest.mark.parametrize("S,slots", [(1, 1), (2, 3), (1024, 2)])
def test_simulation_count_and_slot_extremes(S, slots):
    n, k = 5, 4
    e = _engine(n, k, S, slots=slots, synthetic=True)
    o = orc.Oracle(n, k, S, synthetic=True)
    c = e.selfplay(3, seed0=21, max_plies=3)
    rec = e.records(); nply, _ = e.games()
    off = 0
    for g in range(3):
        noise, us = orc.selfplay_tape(21 + g, n)
        r = o.selfplay_game(None, noise, us, maxply=3)
        L = int(nply[g])
        assert L == r["nply"]
        assert np.array_equal(rec["visits"][off:off + L], r["visits"]) and np.array_equal(rec["actions"][off:off + L], r["actions"])
        assert np.array_equal(rec["pis"][off:off + L], r["pis"])
        off += L
    assert c["simulations"] == S * c["plies"]
    e.close()


def test_invalid_arguments_are_rejected():
    with pytest.raises(az.AzError):
        az.Engine(5, 4, 2000, 4)                 # num_simulations > 1024
    with pytest.raises(az.AzError):
        az.Engine(5, 9, 10, 4)                   # win length > board
    e = _engine(5, 4, 8, synthetic=True)
    with pytest.raises(az.AzError):
        e.search(np.zeros(25, np.uint8), 3, -1, 1.0)            # player must be 1 or 2
    b = np.zeros(25, np.uint8); b[3] = 7
    with pytest.raises(az.AzError):
        e.search(b, 1, -1, 1.0)                                 # bad cell value
    with pytest.raises(ValueError):
        e.search(np.zeros(25, np.uint8), 1, -1, 1.0, noise=np.ones(3))   # noise length != legal cells
    e.close()


def _check_episode_invariants(n, k, S, rec, nply, res, games):
    o = orc.Oracle(n, k, 1)
    nn = n * n
    assert rec["boards"].shape[0] == int(nply.sum())
    assert (rec["visits"].sum(axis=1) == S).all()                              # every simulation passes one root child (Q7)
    assert (rec["visits"][rec["boards"] != 0] == 0).all()                      # occupied cells are never selected
    assert (rec["pis"][rec["boards"] != 0] == 0).all()
    np.testing.assert_allclose(rec["pis"].sum(axis=1), 1.0, atol=2e-5)
    chosen = rec["boards"][np.arange(len(rec["actions"])), rec["actions"]]
    assert (chosen == 0).all()                                                 # moves are legal
    off = 0
    for g in range(games):
        L = int(nply[g])
        acts = rec["actions"][off:off + L]
        rc, term, board, pl, result = o.replay(acts)                           # oracle rules replay
        assert rc == 0 and not term.any()
        assert result == int(res[g]) and result in (1, 2, 3)                   # finished, outcome identical
        want = np.array([0 if result == 3 else (1 if m == result else -1) for m in rec["movers"][off:off + L]])
        assert np.array_equal(rec["z"][off:off + L], want)
        assert rec["movers"][off] == 1 and (np.diff(rec["movers"][off:off + L].astype(int)) != 0).all()
        # the recorded board before ply m is the replay of the first m actions
        for m in (0, L // 2, L - 1):
            _, _, bm, _, _ = o.replay(acts[:m])
            assert np.array_equal(rec["boards"][off + m], bm)
        off += L


def test_full_size_5x5_episode_with_refill_invariants():
    """BASELINE configs[1] shape (5x5/4, 100 sims) with more games than slots: refill, outcomes, z, legality."""
    n, k, S, G = 5, 4, 100, 1536
    e = _engine(n, k, S, slots=1024)
    e.load_weights(weights_from_fixture(n, "ckpt_saved"), 0)
    c = e.selfplay(G, seed0=99)
    rec = e.records(); nply, res = e.games()
    assert c["games"] == G and c["plies"] == int(nply.sum()) and (nply > 0).all()
    _check_episode_invariants(n, k, S, rec, nply, res, G)
    e.close()


def test_full_size_15x15_first_plies_invariants():
    """BASELINE configs[3] per-GPU shard (15x15/5, 1024 games, 400 sims), first 3 plies: properties + oracle spot checks."""
    n, k, S, G, cut = 15, 5, 400, 1024, 3
    sd = weights_from_fixture(n, "seeded")
    eng = az.MultiEngine(n, k, S, G, engines=4, log_table=orc.numpy_log_table(S))
    eng.load_weights(sd, 0)
    c = eng.selfplay(G, seed0=31337, max_plies=cut)
    rec = eng.records(); nply, res = eng.games()
    assert (nply == cut).all() and (res == 0).all() and c["plies"] == G * cut
    assert (rec["visits"].sum(axis=1) == S).all()
    assert (rec["visits"][rec["boards"] != 0] == 0).all()
    np.testing.assert_allclose(rec["pis"].sum(axis=1), 1.0, atol=2e-5)
    assert (rec["z"] == 99).all()                                               # cut games carry no label
    o = orc.Oracle(n, k, S); onet = orc.Net(n, sd)
    for g in (0, 255, 256, 777, 1023):                                          # spans all four engines
        noise, us = orc.selfplay_tape(31337 + g, n, maxply=cut)
        r = o.selfplay_game(onet, noise, us, maxply=cut)
        sl = slice(g * cut, g * cut + cut)
        assert np.array_equal(rec["actions"][sl], r["actions"]) and np.array_equal(rec["visits"][sl], r["visits"])
        assert np.array_equal(rec["pis"][sl], r["pis"]) and np.array_equal(rec["boards"][sl], r["boards"])
    eng.close()


def test_full_size_15x15_400sims_episode_with_refill():
    """The BASELINE headline shape end to end: 15x15/5, 400 sims, 1024 slots (4 engines), 1100 games so that slots are
    refilled; every game is replayed with the oracle's rules and every record is checked."""
    n, k, S, G = 15, 5, 400, 1100
    eng = az.MultiEngine(n, k, S, 1024, engines=4, log_table=orc.numpy_log_table(S))
    eng.load_weights(weights_from_fixture(n, "seeded"), 0)
    c = eng.selfplay(G, seed0=2718)
    rec = eng.records(); nply, res = eng.games()
    assert c["games"] == G and c["plies"] == int(nply.sum()) and (nply >= 9).all()      # a win needs at least 9 plies
    assert c["simulations"] == S * c["plies"] and c["expansions"] + c["terminal_hits"] == c["simulations"]
    _check_episode_invariants(n, k, S, rec, nply, res, G)
    eng.close()


def test_full_size_9x9_4096_slots_200sims_episode_with_refill():
    """BASELINE configs[2] end to end: 9x9 / 5-in-a-row, 4096 concurrent games (4 engines: two boards per trunk workgroup,
    two rounds of workgroups per launch), 200 simulations, 4300 games so that slots are refilled; every game is replayed
    with the oracle's rules, every record is checked, and a few complete games are compared with the oracle bit for bit."""
    n, k, S, G = 9, 5, 200, 4300
    sd = weights_from_fixture(n, "seeded")
    eng = az.MultiEngine(n, k, S, 4096, engines=4, log_table=orc.numpy_log_table(S))
    eng.load_weights(sd, 0)
    c = eng.selfplay(G, seed0=1618)
    rec = eng.records(); nply, res = eng.games()
    eng.close()
    assert c["games"] == G and c["plies"] == int(nply.sum()) and (nply >= 9).all()
    assert c["simulations"] == S * c["plies"] and c["expansions"] + c["terminal_hits"] == c["simulations"]
    _check_episode_invariants(n, k, S, rec, nply, res, G)
    o = orc.Oracle(n, k, S); onet = orc.Net(n, sd)
    starts = np.concatenate([[0], np.cumsum(nply)])
    for g in (0, 1023, 2048, 4095, 4096, 4299):                               # first-round slots of every engine + refilled ones
        noise, us = orc.selfplay_tape(1618 + g, n)
        r = o.selfplay_game(onet, noise, us)
        sl = slice(int(starts[g]), int(starts[g + 1]))
        assert r["nply"] == int(nply[g]) and r["result"] == int(res[g])
        for key in ("actions", "boards", "visits", "pis", "z"):
            assert np.array_equal(rec[key][sl], r[key]), f"game {g}: {key} differs from the oracle"


def test_generate_packed_feeds_the_device_replay_ring():
    import torch
    from alphazero_piskvorky_amd import net
    from alphazero_piskvorky_amd.controller import NeuralNetworkController
    from alphazero_piskvorky_amd.device_replay import DeviceReplayBuffer
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    m = net.GomokuNet(board_size=5)
    m.load_state_dict({kk: torch.tensor(v) for kk, v in weights_from_fixture(5, "ckpt_saved").items()})
    ctrl = NeuralNetworkController(m, device="cuda:0")
    mgr = SelfPlayManager(ctrl, "cuda:0", mcts_params={"num_simulations": 30}, concurrent_games=16, seed=5)
    packed, total, eng, dev, n = mgr.generate_packed(20)
    assert total == mgr.last_counters["records"] and packed.numel() >= total * eng.record_bytes
    buf = DeviceReplayBuffer(eng, capacity=10_000, device="cuda:0", seed=0)
    buf.extend_packed(packed, total)
    s, p, z = buf.sample_batch(128)
    assert s.shape == (128, 4, 5, 5) and p.shape == (128, 5, 5) and z.shape == (128,)
    assert torch.allclose(p.sum(dim=(1, 2)), torch.ones(128, device=p.device), atol=1e-5)
    assert np.isfinite(ctrl.train_step(s, p, z)["loss"])


def test_explicit_tapes_equal_seeded_tapes():
    """az_selfplay_args.noise_tape / u_tape (host-provided tapes) give the same episode as seed0-generated ones."""
    n, k, S, G = 5, 4, 30, 4
    e = _engine(n, k, S, slots=3, synthetic=True)
    e.selfplay(G, seed0=4000)
    a = e.records()
    nn = n * n
    tapelen = sum(nn - m for m in range(nn))
    noise = np.zeros((G, tapelen)); us = np.zeros((G, nn))
    for g in range(G):
        nz, u = orc.selfplay_tape(4000 + g, n)
        noise[g], us[g] = nz, u
    e.selfplay(G, seed0=0, noise_tape=noise, u_tape=us)
    b = e.records()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    e.close()


@pytest.mark.parametrize("c_puct,alpha,w", [(1.0, 0.3, 0.25), (4.5, 0.6, 0.4), (2.0, 1.0, 0.1), (0.25, 2.5, 0.9)])
def test_non_default_search_parameters(c_puct, alpha, w):
    """mcts.py:87-97 parameters other than the defaults: PUCT constant, Dirichlet alpha (incl. the >= 1 gamma sampler)
    and mixing weight, engine vs oracle bit for bit, with the engine's own host RNG producing the tape."""
    n, k, S, G = 9, 5, 50, 3
    sd = weights_from_fixture(n, "seeded")
    e = az.Engine(n, k, S, 2, c_puct=c_puct, dirichlet_alpha=alpha, dirichlet_weight=w, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    e.selfplay(G, seed0=555, max_plies=5)
    rec = e.records(); nply, _ = e.games()
    o = orc.Oracle(n, k, S, c_puct=c_puct, alpha=alpha, w=w)
    onet = orc.Net(n, sd)
    off = 0
    for g in range(G):
        rs = np.random.RandomState(555 + g)
        nz, us = [], []
        for m in range(5):
            nz.append(rs.dirichlet([alpha] * (n * n - m))); us.append(rs.random_sample())
        r = o.selfplay_game(onet, np.concatenate(nz), np.array(us), maxply=5)
        L = int(nply[g]); sl = slice(off, off + L)
        for key in ("actions", "visits", "pis"):
            assert np.array_equal(rec[key][sl], r[key]), f"{key} differs (c_puct={c_puct}, alpha={alpha}, w={w})"
        off += L
    e.close()


def test_streamed_tapes_equal_bulk_tapes_with_refill_and_restart(monkeypatch):
    """The tape producer (waves of two plies streamed ahead of the games) against AZ_TAPE_STREAM=0 (every tape generated
    before the first move): many more games than slots, so refilled slots start late at ply 0 while the waves are far
    ahead; also an episode ended mid-way (its producer must stop) and a max_plies cap shorter than one wave."""
    n, k, S, G = 5, 4, 12, 37
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("AZ_TAPE_STREAM", mode)
        e = _engine(n, k, S, slots=5, synthetic=True)
        e.selfplay_begin(G, seed0=31337)
        e.selfplay_step(3)
        e.selfplay_end()                        # abandoned after 3 plies: its producer must stop before the next episode
        e.selfplay(G, seed0=31337)
        full = e.records(); nply, res = e.games()
        e.selfplay(G, seed0=31337, max_plies=1)
        capped = e.records()
        out[mode] = (full, nply, res, capped)
        e.close()
    for a, b in zip(out["1"][0].values(), out["0"][0].values()):
        assert np.array_equal(a, b)
    assert np.array_equal(out["1"][1], out["0"][1]) and np.array_equal(out["1"][2], out["0"][2])
    for key in out["1"][3]:
        assert np.array_equal(out["1"][3][key], out["0"][3][key]), key
    assert len(out["1"][3]["actions"]) == G


def test_calls_that_would_clobber_an_open_episode_are_rejected():
    """az_search / az_net_eval / az_arena / a nested az_selfplay_begin between begin and end would overwrite the slot and
    record state of the running episode: AZ_ERR_STATE, and the episode continues undisturbed."""
    n, k, S, G = 5, 4, 20, 6
    ref = _engine(n, k, S, slots=4, synthetic=True)
    ref.selfplay(G, seed0=808)
    want = ref.records()
    ref.close()
    e = _engine(n, k, S, slots=4, synthetic=True)
    e.selfplay_begin(G, seed0=808)
    e.selfplay_step(2)
    board = np.zeros(n * n, np.uint8)
    for call in (lambda: e.search(board, 1, -1, 1.0), lambda: e.arena(2, seed0=1), lambda: e.selfplay_begin(G, seed0=1),
                 lambda: e.selfplay(G, seed0=1)):
        with pytest.raises(az.AzError, match="-6"):
            call()
    active = 1
    while active > 0:
        active, _ = e.selfplay_step(64)
    e.selfplay_end()
    got = e.records()
    for key in want:
        assert np.array_equal(want[key], got[key]), key
    e.close()


def test_explicit_tape_shorter_than_the_plies_is_rejected():
    n, k, S, G = 5, 4, 8, 2
    nn = n * n
    e = _engine(n, k, S, slots=2, synthetic=True)
    full = sum(nn - m for m in range(nn))
    three = sum(nn - m for m in range(3))
    us = np.full((G, nn), 0.5)
    with pytest.raises(az.AzError):
        e.selfplay(G, noise_tape=np.full((G, full - 1), 0.1), u_tape=us)             # whole games need the whole tape
    with pytest.raises(az.AzError):
        e.selfplay(G, max_plies=3, noise_tape=np.full((G, three - 1), 0.1), u_tape=us)
    c = e.selfplay(G, max_plies=3, noise_tape=np.full((G, three), 1.0 / nn), u_tape=us)   # exactly 3 plies of tape: accepted
    assert c["plies"] == 3 * G
    e.close()


@pytest.mark.parametrize("synthetic", [True, False])
def test_lanes_inside_the_library_give_the_single_lane_episode(synthetic):
    """az_config.engines: the slots split over K streams + K host threads inside ONE az_selfplay call, all lanes claiming
    game ids from one shared device queue.  Games are seeded per id and recorded per id, so records, outcomes and the
    work counters are identical for every K -- also with far more games than slots (refill through the shared queue),
    for the arena, and for a single-position search on a multi-lane engine."""
    n, k, S, G = 9, 5, 24, 45
    sd = weights_from_fixture(n, "seeded")
    out = {}
    for K in (1, 3, 4):
        e = az.Engine(n, k, S, 12, engines=K, synthetic=synthetic, log_table=orc.numpy_log_table(S))
        assert e.lanes() == K
        if not synthetic:
            e.load_weights(sd, 0); e.load_weights(weights_from_fixture(n, "seeded"), 1)
        c = e.selfplay(G, seed0=77, max_plies=0 if synthetic else 4)
        rec = e.records(); nply, res = e.games()
        arena = e.arena(7, seed0=5, temperature_table=orc.arena_T_table(n * n)) if synthetic else None
        board = np.zeros(n * n, np.uint8); board[40] = 1
        srch = e.search(board, 2, 40, 0.7, None, 0.3)
        out[K] = (rec, nply, res, c, arena, srch)
        e.close()
    ref = out[1]
    for K in (3, 4):
        rec, nply, res, c, arena, srch = out[K]
        for key in ref[0]:
            assert np.array_equal(ref[0][key], rec[key]), f"K={K}: {key}"
        assert np.array_equal(ref[1], nply) and np.array_equal(ref[2], res)
        for key in ("games", "plies", "records", "simulations", "expansions", "root_evals", "terminal_hits", "depth_sum"):
            assert ref[3][key] == c[key], f"K={K}: counter {key}"
        if arena is not None:
            for key in ("wins", "losses", "draws", "total"):
                assert ref[4][key] == arena[key]
            assert np.array_equal(ref[4]["actions"], arena["actions"]) and np.array_equal(ref[4]["results"], arena["results"])
        assert np.array_equal(ref[5]["N"], srch["N"]) and ref[5]["action"] == srch["action"]


@pytest.mark.parametrize("lanes", [1, 3])
def test_slot_compaction_between_plies_is_invisible(lanes, monkeypatch):
    """k_refill moves the active slots to the front of a lane after every ply and the next ply is launched over them only
    (AZ_COMPACT=0 keeps every game in the slot it was born in).  Records go by game id, so complete games with refills from
    the shared queue, their outcomes and the work counters are identical either way, also with virtual-loss batching (items
    per slot) and in the arena; and both equal the oracle."""
    n, k, S, G = 9, 5, 20, 37
    out = {}
    for compact in ("1", "0"):
        monkeypatch.setenv("AZ_COMPACT", compact)
        e = az.Engine(n, k, S, 10, engines=lanes, synthetic=True, log_table=orc.numpy_log_table(S))
        c = e.selfplay(G, seed0=913)
        rec = e.records(); nply, res = e.games()
        arena = e.arena(9, seed0=2, temperature_table=orc.arena_T_table(n * n))
        e.set_virtual_loss(3)
        cv = e.selfplay(G, seed0=913)
        recv = e.records()
        out[compact] = (rec, nply, res, c, arena, cv, recv)
        e.close()
    a, b = out["1"], out["0"]
    for key in a[0]:
        assert np.array_equal(a[0][key], b[0][key]), key
        assert np.array_equal(a[6][key], b[6][key]), f"virtual loss: {key}"
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for key in ("games", "plies", "records", "simulations", "expansions", "root_evals", "terminal_hits", "depth_sum"):
        assert a[3][key] == b[3][key] and a[5][key] == b[5][key], key
    assert np.array_equal(a[4]["actions"], b[4]["actions"]) and np.array_equal(a[4]["results"], b[4]["results"])
    assert len(set(a[1].tolist())) > 3           # games of different lengths: slots really emptied at different plies
    o = orc.Oracle(n, k, S, synthetic=True)
    off = 0
    for g in range(G):
        noise, us = orc.selfplay_tape(913 + g, n)
        r = o.selfplay_game(None, noise, us)
        L = int(a[1][g])
        assert L == r["nply"] and np.array_equal(a[0]["visits"][off:off + L], r["visits"]) and np.array_equal(a[0]["actions"][off:off + L], r["actions"])
        off += L


def test_auto_lanes_and_lane_limits():
    e = az.Engine(5, 4, 8, 1024, synthetic=True)
    assert e.lanes() == 1                        # small boards are launch-bound: one lane
    e.close()
    e = az.Engine(9, 5, 8, 1024, synthetic=True)
    assert e.lanes() == 4                        # one lane per 128 slots, at most four
    e.close()
    e = az.Engine(9, 5, 8, 200, synthetic=True)
    assert e.lanes() == 1
    e.close()
    e = az.Engine(9, 5, 8, 3, engines=8, synthetic=True)
    assert e.lanes() == 3                        # never an empty lane
    c = e.selfplay(5, seed0=1, max_plies=2)
    assert c["plies"] == 10
    e.close()
    with pytest.raises(az.AzError):
        az.Engine(9, 5, 8, 64, engines=17, synthetic=True)


@pytest.mark.parametrize("n,k,S,cut,model", [(15, 5, 24, 5, "plain"), (9, 5, 30, 6, "plain"), (15, 5, 16, 3, "resnet")])
def test_every_kernel_shape_gives_the_same_episode(n, k, S, cut, model):
    """The library picks kernel shapes by occupancy (round 3): the fused trunk or the tile-split one (at most 64 active slots of
    a lane), `k_fc<1, 1>` (at most 4 rows of 16 boards) or `k_fc<2, 4>`.  The same 96 games on 96 slots in one lane (fused trunk,
    throughput FC), on 96 slots in three lanes (32 each: tile-split trunk, latency FC) and on 8 slots (everything small, eleven
    refills) must give identical records, and the first games must be the oracle's, bit for bit."""
    if model == "resnet":
        from alphazero_piskvorky_amd.net import fold_resnet_state_dict
        from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict
        sd = synthetic_resnet_state_dict(n)
        onet = orc.Net(n, resnet_tensors=fold_resnet_state_dict(sd))
    else:
        sd = weights_from_fixture(n, "seeded")
        onet = orc.Net(n, sd)
    G, seed0 = 96, 5150
    out = []
    for slots, lanes in ((96, 1), (96, 3), (8, 1)):
        e = az.Engine(n, k, S, slots, engines=lanes, log_table=orc.numpy_log_table(S), model=model)
        e.load_weights(sd, 0)
        e.selfplay(G, seed0=seed0, max_plies=cut)
        out.append((e.records(), e.games()))
        e.close()
    for rec, games in out[1:]:
        for key in out[0][0]:
            assert np.array_equal(rec[key], out[0][0][key]), key
        assert np.array_equal(games[0], out[0][1][0]) and np.array_equal(games[1], out[0][1][1])
    rec, (nply, _) = out[0]
    o = orc.Oracle(n, k, S)
    off = 0
    for g in range(3):
        noise, us = orc.selfplay_tape(seed0 + g, n, maxply=cut)
        r = o.selfplay_game(onet, noise, us, maxply=cut)
        L = int(nply[g])
        assert L == r["nply"]
        for key in ("actions", "visits", "pis"):
            assert np.array_equal(rec[key][off:off + L], r[key]), f"game {g}: {key}"
        off += L


# ---------------------------------------------------------------------------------------------------------------------
# settings that cannot be combined: every pair, whichever is switched on first
# ---------------------------------------------------------------------------------------------------------------------
# how each setting is switched on, and how it reads back as off where the API can say (subtree reuse and leaf symmetry have
# no getter: for them, as for all, the episode after the refusal must be the one before it)
def _ext_on(e):
    from tests.test_external_eval_gpu import CpuEvaluator, net_eval
    CpuEvaluator(e, net_eval(orc.Net(e.n, weights_from_fixture(e.n, "ckpt_saved"))))


SETTINGS = {
    "reuse": (lambda e: e.set_subtree_reuse(True), None),
    "virtual loss": (lambda e: e.set_virtual_loss(2), lambda e: e.ext_capacity() == 4),
    "leaf symmetry": (lambda e: e.set_leaf_symmetry(True), None),
    "external evaluator": (_ext_on, lambda e: not e.external_evaluator()),
    "playout cap": (lambda e: e.set_playout_cap(4), lambda e: e.playout_cap()["fast_sims"] == 0),
    "forced playouts": (lambda e: e.set_forced_playouts(2.0), lambda e: e.forced_playouts()["k"] == 0.0),
    "gumbel": (lambda e: e.set_gumbel(4), lambda e: e.gumbel()["m"] == 0),
    "solver": (lambda e: e.set_solver(True), lambda e: not e.solver()),
}
CONFLICTS = [
    ("reuse", "virtual loss", "subtree reuse and virtual-loss batching cannot be combined"),
    ("reuse", "external evaluator", "subtree reuse and the external evaluator cannot be combined"),
    ("playout cap", "reuse", "the playout cap and subtree reuse cannot be combined"),
    ("forced playouts", "reuse", "forced playouts and subtree reuse cannot be combined"),
    ("gumbel", "reuse", "the Gumbel root search and subtree reuse cannot be combined"),
    ("solver", "reuse", "the solver and subtree reuse cannot be combined"),
    ("playout cap", "external evaluator", "the playout cap and the external evaluator cannot be combined"),
    ("leaf symmetry", "external evaluator", "random-symmetry leaf evaluation and the external evaluator cannot be combined"),
    ("gumbel", "virtual loss", "the Gumbel root search and virtual-loss batching cannot be combined"),
    ("forced playouts", "gumbel", "forced playouts and the Gumbel root search cannot be combined"),
    ("gumbel", "external evaluator", "the Gumbel root search and the external evaluator cannot be combined (it returns priors, not logits)"),
    ("solver", "virtual loss", "the solver and virtual-loss batching cannot be combined"),
    ("solver", "forced playouts", "the solver and forced playouts cannot be combined"),
    ("solver", "gumbel", "the solver and the Gumbel root search cannot be combined"),
    ("solver", "external evaluator", "the solver and the external evaluator cannot be combined"),
]


@pytest.mark.parametrize("a,b,message", CONFLICTS, ids=[f"{a} x {b}" for a, b, _ in CONFLICTS])
def test_conflicting_settings_are_refused_in_either_order(a, b, message):
    import re
    n, k, S = 5, 4, 8
    sd = weights_from_fixture(n, "ckpt_saved")

    def episode(e):
        e.selfplay(2, seed0=31, max_plies=2)
        return e.records(), e.games()

    for first, second in ((a, b), (b, a)):
        e = _engine(n, k, S)
        e.load_weights(sd, 0)
        SETTINGS[first][0](e)
        before = episode(e)
        with pytest.raises(az.AzError, match=r"\(-1\).*" + re.escape(message)):
            SETTINGS[second][0](e)
        reads_off = SETTINGS[second][1]
        assert reads_off is None or reads_off(e), f"{first}, then {second}: the refused setting reads back as on"
        rec, games = episode(e)
        assert len(rec["actions"]) == 4
        for key in rec:
            assert np.array_equal(rec[key], before[0][key]), f"{first}, then {second}: {key} changed with the refused setting"
        assert np.array_equal(games[0], before[1][0]) and np.array_equal(games[1], before[1][1])
        e.close()
