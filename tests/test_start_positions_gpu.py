"""az_set_start_positions on the GPU.  The definition under test: a game started from the position that game g reached at
ply m, with game g's seed, continues game g bit for bit -- so the unchanged CPU oracle pins the feature: its free-running
games, cut at ply m_g = (3 g + 1) mod nply_g, are what the engine has to produce from there on (array_equal everywhere, no
tolerances)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import examples_ref as ref
from tests.util import build_weights, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi, games
from alphazero_piskvorky_amd.net import fold_resnet_state_dict
from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict

REC_KEYS = ("boards", "movers", "lasts", "visits", "pis", "actions", "z")
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _weights(n, tag):
    if tag == "resnet":
        return synthetic_resnet_state_dict(n)
    return weights_from_fixture(n, tag)


def _oracle_net(n, tag):
    if tag is None:
        return None
    if tag == "resnet":
        return orc.Net(n, resnet_tensors=fold_resnet_state_dict(synthetic_resnet_state_dict(n)))
    return orc.Net(n, weights_from_fixture(n, tag))


@functools.lru_cache(maxsize=None)
def _oracle_games(n, k, S, G, seed0, tag, cut=0, leaf_sym=False, vl=0, reuse=False):
    """G free-running oracle games, seeds seed0 + g (computed once per configuration, never modified)"""
    o = orc.Oracle(n, k, S, synthetic=tag is None, leaf_sym=leaf_sym, virtual_loss=vl, reuse=reuse)
    net = _oracle_net(n, tag)

    def one(g):
        noise, us = orc.selfplay_tape(seed0 + g, n, maxply=cut or None)
        return o.selfplay_game(net, noise, us, maxply=cut or None, game=seed0 + g)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return tuple(ex.map(one, range(G)))


def _cut_points(gs, k):
    ms = []
    for g, r in enumerate(gs):
        assert r["nply"] >= 2 * k - 1 or r["result"] == 0          # a decided game has at least 2k - 1 plies
        ms.append((3 * g + 1) % r["nply"])
    return ms


def _positions_of(gs, ms):
    return (np.stack([r["boards"][m] for r, m in zip(gs, ms)]), np.array([r["movers"][m] for r, m in zip(gs, ms)], np.uint8),
            np.array([r["lasts"][m] for r, m in zip(gs, ms)], np.int16))


def _engine(n, k, S, slots, tag, **kw):
    e = az.Engine(n, k, S, slots, synthetic=tag is None, log_table=orc.numpy_log_table(S),
                  model="resnet" if tag == "resnet" else "plain", **kw)
    if tag is not None:
        e.load_weights(_weights(n, tag), 0)
    return e


def _assert_continues(e, gs, ms, c, what):
    """engine game g = oracle game g from ply m_g on: lengths, results, every record field, the counters"""
    nply, res = e.games()
    rec = e.records()
    want_len = [r["nply"] - m for r, m in zip(gs, ms)]
    assert nply.tolist() == want_len, f"{what}: plies searched per game"
    assert res.tolist() == [r["result"] for r in gs], f"{what}: results"
    for key in REC_KEYS:
        want = np.concatenate([r[key][m:] for r, m in zip(gs, ms)])
        assert rec[key].shape == want.shape and np.array_equal(rec[key], want), f"{what}: {key} differ"
    assert c["plies"] == c["records"] == sum(want_len) and c["games"] == len(gs)
    return rec


def _continuation(n, k, S, G, slots, seed0, tag, cut=0, leaf_sym=False, vl=0, cache=0, engine_kw=None, what=""):
    gs = _oracle_games(n, k, S, G, seed0, tag, cut, leaf_sym, vl)
    ms = _cut_points(gs, k)
    e = _engine(n, k, S, slots, tag, **(engine_kw or {}))
    if leaf_sym:
        e.set_leaf_symmetry(True)
    if vl:
        e.set_virtual_loss(vl)
    if cache:
        e.set_eval_cache(cache)
    e.set_start_positions(*_positions_of(gs, ms))
    assert e.start_positions() == G
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    _assert_continues(e, gs, ms, c, what or f"{n}x{n}")
    assert c["root_evals"] == c["plies"]
    return e, c, gs, ms


def _has_line(cells, n, k):
    b = np.asarray(cells).reshape(n, n)
    for r in range(n):
        for c in range(n):
            if b[r, c]:
                for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                    rr, cc, ln = r, c, 0
                    while 0 <= rr < n and 0 <= cc < n and b[rr, cc] == b[r, c]:
                        rr, cc, ln = rr + dr, cc + dc, ln + 1
                    if ln >= k:
                        return int(b[r, c])
    return 0


def _swap(cells):
    c = np.asarray(cells, np.uint8)
    return ((3 - c) * (c != 0)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# 1. continuation identity, self-play
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persist", ["1", "0"])
def test_5x5_trained_checkpoint_continues_the_oracle_games(persist, monkeypatch):
    monkeypatch.setenv("AZ_PERSIST", persist)
    e, c, gs, ms = _continuation(5, 4, 48, 9, 4, 4100, "ckpt_saved", what=f"5x5 AZ_PERSIST={persist}")
    assert (e.persistent() > 0) == (persist == "1")
    assert max(ms) >= 3 and 0 < c["plies"] < sum(r["nply"] for r in gs)
    e.close()


@pytest.mark.parametrize("n,k,S,G,slots,tag", [(8, 5, 24, 7, 3, None), (8, 5, 24, 5, 3, "seeded"), (9, 5, 32, 7, 4, "seeded"),
                                               (9, 5, 24, 5, 3, "resnet")],
                         ids=["8x8-synthetic", "8x8-seeded", "9x9-seeded", "9x9-resnet"])
def test_8x8_and_9x9_continue_the_oracle_games(n, k, S, G, slots, tag):
    """8x8: 64 cells, exactly one plane word; 9x9: two"""
    e, c, gs, ms = _continuation(n, k, S, G, slots, 4200 + n, tag)
    assert e.persistent() == 0
    e.close()


@pytest.mark.parametrize("tag,S,G,cut", [(None, 24, 10, 80), ("seeded", 24, 6, 14)], ids=["synthetic", "seeded"])
def test_15x15_with_max_plies_cutting_games(tag, S, G, cut):
    """max_plies counts stones on the board: a game started at ply m is cut after max_plies - m searched plies (the
    synthetic episode has both cut and decided games)"""
    e, c, gs, ms = _continuation(15, 5, S, G, 4, 4300, tag, cut=cut)
    assert any(r["result"] == 0 and r["nply"] == cut and (r["z"] == 99).all() for r in gs), "no game was cut"
    e.close()


@pytest.mark.parametrize("env,lanes", [({}, 1), ({}, 2), ({"AZ_COMPACT": "0"}, 2), ({"AZ_TAPE_STREAM": "0"}, 1), ({"AZ_GRAPH": "0"}, 1)],
                         ids=["default", "2-lanes", "no-compaction", "bulk-tapes", "eager"])
def test_refill_lanes_compaction_and_tape_modes(env, lanes, monkeypatch):
    """more games than slots, so most games get their position from a refill between plies; deep start plies with the
    streamed tapes (the default) need the producer's look-ahead"""
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    n, k, S, G = 9, 5, 24, 23
    e, c, gs, ms = _continuation(n, k, S, G, 6, 4400, None, engine_kw=dict(engines=lanes), what=f"{env} lanes={lanes}")
    assert e.lanes() == lanes and max(ms) >= 12
    e.close()


def test_15x15_streamed_tapes_with_deep_start_plies():
    """every game starts beyond the first two tape waves (ply >= 4): without the look-ahead of the tape producer the first
    plies would read noise and u that are not on the device yet"""
    n, k, S, G, seed0 = 15, 5, 24, 10, 4500
    gs = _oracle_games(n, k, S, G, seed0, None)
    ms = [max(m, r["nply"] - 6) for r, m in zip(gs, _cut_points(gs, k))]       # start 6 plies before the end at the latest
    assert min(ms) >= 4
    e = _engine(n, k, S, 4, None)
    e.set_start_positions(*_positions_of(gs, ms))
    c = e.selfplay(G, seed0=seed0)
    assert c["tape_threads"] > 0
    _assert_continues(e, gs, ms, c, "15x15 deep starts")
    e.close()


def test_lane_wider_than_1024_slots():
    """k_refill walks such a lane in chunks of 1024 slots"""
    n, k, S, G, slots = 5, 4, 8, 1300, 1100
    gs = _oracle_games(n, k, S, G, 4600, None)
    ms = _cut_points(gs, k)
    e = _engine(n, k, S, slots, None, engines=1)
    e.set_start_positions(*_positions_of(gs, ms))
    c = e.selfplay(G, seed0=4600)
    _assert_continues(e, gs, ms, c, "1100 slots")
    e.close()


@pytest.mark.parametrize("n,k,S,tag", [(5, 4, 40, "ckpt_saved"), (9, 5, 24, "seeded")], ids=["5x5", "9x9"])
def test_virtual_loss_cache_and_leaf_symmetry(n, k, S, tag):
    G, seed0 = 6, 4700 + n
    e, c, _, _ = _continuation(n, k, S, G, 4, seed0, tag, vl=4, what="virtual loss 4")
    e.close()
    e, c, _, _ = _continuation(n, k, S, G, 4, seed0, tag, cache=1 << 14, what="cache")
    assert c["cache_lookups"] > 0
    e.close()
    e, c, _, _ = _continuation(n, k, S, G, 4, seed0, tag, leaf_sym=True, what="leaf symmetry")
    e.close()


def test_explicit_tapes_go_by_absolute_ply():
    n, k, S, G, seed0 = 6, 4, 16, 5, 4800
    gs = _oracle_games(n, k, S, G, seed0, None)
    ms = _cut_points(gs, k)
    tapes = [orc.selfplay_tape(seed0 + g, n) for g in range(G)]
    e = _engine(n, k, S, 3, None)
    e.set_start_positions(*_positions_of(gs, ms))
    c = e.selfplay(G, seed0=1, noise_tape=np.stack([t[0] for t in tapes]), u_tape=np.stack([t[1] for t in tapes]))
    _assert_continues(e, gs, ms, c, "explicit tapes")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. arena
# ---------------------------------------------------------------------------------------------------------------------
def _arena_setup(n=5, k=4, S=32):
    sd_a, sd_b = weights_from_fixture(n, "ckpt_saved"), build_weights(n, seed=77)
    e = az.Engine(n, k, S, 8, log_table=orc.numpy_log_table(S))
    e.load_weights(sd_a, 0); e.load_weights(sd_b, 1)
    return e, orc.Oracle(n, k, S), orc.Net(n, sd_a), orc.Net(n, sd_b)


def test_arena_continues_the_oracle_arena_games():
    """Games 2i and 2i+1 share table entry i, so the even games are continued from their own positions in one run and the
    odd ones, colour-exchanged on input (the engine exchanges them back), in a second."""
    n, k, S, G, seed0 = 5, 4, 32, 8, 5100
    e, o, na, nb = _arena_setup(n, k, S)
    T = orc.arena_T_table(n * n)
    ogs = [o.arena_game(na, nb, g, np.random.RandomState(seed0 + g).random_sample(n * n)) for g in range(G)]
    ms = [(3 * g + 1) % r["nply"] for g, r in enumerate(ogs)]
    pos = [games.position_from_actions(r["actions"][:m], n, first_player=2 if g & 1 else 1) for g, (r, m) in enumerate(zip(ogs, ms))]
    for parity in (0, 1):
        sel = range(parity, G, 2)
        boards = np.stack([_swap(pos[g][0]) if parity else pos[g][0] for g in sel])
        players = np.array([3 - pos[g][1] if parity else pos[g][1] for g in sel], np.uint8)
        lasts = np.array([pos[g][2] for g in sel], np.int16)
        e.set_start_positions(boards, players, lasts)
        r = e.arena(G, seed0=seed0, temperature_table=T)
        for g in sel:
            want = ogs[g]["actions"][ms[g]:]
            assert int(r["nply"][g]) == len(want), f"game {g}: plies"
            assert np.array_equal(r["actions"][g][:len(want)], want), f"game {g}: moves after the start position"
            assert (r["actions"][g][len(want):] == -1).all()
            assert int(r["results"][g]) == ogs[g]["result"], f"game {g}: result"
    e.close()


def test_arena_suite_every_position_once_from_either_side():
    """count positions over 2 count + 1 games (the last game wraps to position 0).  Every ply is searched again by
    Oracle.search with the mover's net, T[(ply + 1) >> 1], u[ply] and no noise; on the CPU this per-ply recipe reproduces
    Oracle.arena_game move for move."""
    n, k, S, seed0 = 5, 4, 32, 5200
    nn = n * n
    e, o, na, nb = _arena_setup(n, k, S)
    T = orc.arena_T_table(nn)
    suite = games.positions_from_actions([[12, 6, 7], [0, 24], [11, 12, 13, 7, 17, 2]], n)
    count = len(suite[1])
    G = 2 * count + 1
    e.set_start_positions(*suite)
    r = e.arena(G, seed0=seed0, temperature_table=T)
    tally = [0, 0, 0, 0]
    for g in range(G):
        i = (g >> 1) % count
        board, pl, last = suite[0][i].copy(), int(suite[1][i]), int(suite[2][i])
        if g & 1:
            board, pl = _swap(board), 3 - pl
        us = np.random.RandomState(seed0 + g).random_sample(nn)
        L = int(r["nply"][g])
        assert L > 0
        result = 0
        for j in range(L):
            assert result == 0, f"game {g} was played on after its end"
            ply = int((board != 0).sum())
            ro = o.search(na if pl == 1 else nb, board, pl, last, T[(ply + 1) >> 1], None, us[ply])
            a = int(r["actions"][g][j])
            assert a == ro["action"], f"game {g} ply {ply}: move"
            board[a] = pl
            pl, last = 3 - pl, a
            result = _has_line(board, n, k) or (3 if (board != 0).all() else 0)
        assert result != 0 and int(r["results"][g]) == result, f"game {g}: result"
        tally[result] += 1
    assert (r["wins"], r["losses"], r["draws"]) == (tally[1], tally[2], tally[3])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. identities
# ---------------------------------------------------------------------------------------------------------------------
def _episode(e, G, seed0, **kw):
    c = e.selfplay(G, seed0=seed0, **kw)
    return e.records(), e.games(), c


def _same_episode(a, b, what):
    for key in REC_KEYS:
        assert np.array_equal(a[0][key], b[0][key]), f"{what}: {key}"
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]), what
    assert a[2]["plies"] == b[2]["plies"] and a[2]["root_evals"] == b[2]["root_evals"], what


@pytest.mark.parametrize("reuse", [False, True])
def test_the_empty_board_as_the_only_position_is_the_default_episode(reuse):
    n, k, S, G, seed0 = 5, 4, 40, 6, 5300
    gs = _oracle_games(n, k, S, G, seed0, "ckpt_saved", reuse=reuse)
    e = _engine(n, k, S, 4, "ckpt_saved")
    e.set_subtree_reuse(reuse)
    e.set_start_positions(np.zeros((1, n * n), np.uint8), [1], [-1])
    c = e.selfplay(G, seed0=seed0)
    _assert_continues(e, gs, [0] * G, c, f"empty board, reuse={reuse}")
    with_positions = (e.records(), e.games(), c)
    # count = 0: the engine is a fresh engine again
    e.clear_start_positions()
    assert e.start_positions() == 0
    cleared = _episode(e, G, seed0)
    fresh_e = _engine(n, k, S, 4, "ckpt_saved")
    fresh_e.set_subtree_reuse(reuse)
    fresh = _episode(fresh_e, G, seed0)
    fresh_e.close()
    _same_episode(cleared, fresh, "after count = 0")
    _same_episode(with_positions, fresh, "empty board")
    e.close()


def test_clearing_after_real_positions_gives_a_fresh_engines_episode():
    n, k, S, G, seed0 = 9, 5, 24, 7, 5400
    e, _, _, _ = _continuation(n, k, S, G, 4, seed0, None)
    e.clear_start_positions()
    cleared = _episode(e, G, seed0)
    e.close()
    fresh_e = _engine(n, k, S, 4, None)
    fresh = _episode(fresh_e, G, seed0)
    fresh_e.close()
    _same_episode(cleared, fresh, "cleared")
    gs = _oracle_games(n, k, S, G, seed0, None)
    assert cleared[1][0].tolist() == [r["nply"] for r in gs]


def test_the_empty_board_gives_the_default_arena():
    n, S, G, seed0 = 5, 32, 5, 5500
    e, _, _, _ = _arena_setup(n, 4, S)
    T = orc.arena_T_table(n * n)
    want = e.arena(G, seed0=seed0, temperature_table=T)
    e.set_start_positions(np.zeros((1, n * n), np.uint8), [1], [-1])
    got = e.arena(G, seed0=seed0, temperature_table=T)
    for key in ("results", "actions", "nply"):
        assert np.array_equal(got[key], want[key]), key
    e.close()


def test_search_and_search_batch_ignore_the_setting():
    n, k, S = 5, 4, 40
    gs = _oracle_games(n, k, S, 6, 5300, "ckpt_saved")
    pos = _positions_of(gs, _cut_points(gs, k))
    e = _engine(n, k, S, 4, "ckpt_saved")
    rs = np.random.RandomState(2)
    noise = [rs.dirichlet([0.3] * int((b == 0).sum())) for b in pos[0]]
    us = rs.random_sample(6)
    before_b = e.search_batch(pos[0], pos[1], pos[2], 0.7, noise, us)
    before_s = e.search(pos[0][2], pos[1][2], pos[2][2], 0.7, noise[2], us[2])
    e.set_start_positions(pos[0][::-1].copy(), pos[1][::-1].copy(), pos[2][::-1].copy(), first=3)
    after_b = e.search_batch(pos[0], pos[1], pos[2], 0.7, noise, us)
    after_s = e.search(pos[0][2], pos[1][2], pos[2][2], 0.7, noise[2], us[2])
    for key in ("N", "W", "P", "pi", "action"):
        assert np.array_equal(before_b[key], after_b[key]) and np.array_equal(before_s[key], after_s[key]), key
    assert e.start_positions() == 6                            # and the searches left the setting in force
    e.selfplay(3, seed0=5300)
    rec = e.records()
    assert np.array_equal(rec["boards"][0], pos[0][::-1][3])
    e.close()


@pytest.mark.parametrize("n,k", [(6, 4), (14, 5)])
def test_pack_and_example_kernels_carry_the_searched_plies_only(n, k):
    """even sizes: the packed record has padding bytes; 14x14 uses all four plane words"""
    S, G, seed0, cut = 8, 6, 5600 + n, 0 if n == 6 else 24
    gs = _oracle_games(n, k, S, G, seed0, None, cut)
    ms = _cut_points(gs, k)
    want = ref.expected_records([{key: (r[key][m:] if key in REC_KEYS else r[key]) for key in r} for r, m in zip(gs, ms)])
    e = _engine(n, k, S, 4, None)
    e.set_start_positions(*_positions_of(gs, ms))
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    R = c["records"]
    assert R == len(want["z"]) == sum(r["nply"] - m for r, m in zip(gs, ms))
    rb = e.record_bytes
    buf = torch.full((R * rb + 4096,), 0xEE, dtype=torch.uint8, device=DEV)
    e.pack_into(buf.data_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[R * rb:] == 0xEE).all(), "az_selfplay_pack wrote behind the last record"
    got = ref.unpack(host[:R * rb], n)
    assert not ref.same(got, ref.records_from_host(e.records())), "az_selfplay_pack and az_selfplay_records disagree"
    assert not ref.same(got, want), f"packed records differ from the oracle's in {ref.same(got, want)}"
    nn = n * n
    st = torch.full((R * 8 * 4 * nn,), float("nan"), device=DEV); pi = torch.full((R * 8 * nn,), float("nan"), device=DEV)
    z = torch.full((R * 8,), float("nan"), device=DEV)
    e.examples_from_packed(buf.data_ptr(), R, 8, st.data_ptr(), pi.data_ptr(), z.data_ptr())
    torch.cuda.synchronize()
    ws, wp, wz = ref.expected_examples(want, n, 8)
    assert np.array_equal(ref.bits(st.cpu().numpy().reshape(ws.shape)), ref.bits(ws))
    assert np.array_equal(ref.bits(pi.cpu().numpy().reshape(wp.shape)), ref.bits(wp))
    assert np.array_equal(ref.bits(z.cpu().numpy()), ref.bits(wz))
    rs = np.random.RandomState(n)
    idx, sym = rs.randint(0, R, R + 5), rs.randint(0, 8, R + 5)
    B = len(idx)
    st = torch.full((B * 4 * nn,), float("nan"), device=DEV); pi = torch.full((B * nn,), float("nan"), device=DEV)
    z = torch.full((B,), float("nan"), device=DEV)
    ti = torch.as_tensor(idx, dtype=torch.int64, device=DEV); ts = torch.as_tensor(sym, dtype=torch.int32, device=DEV)
    e.examples_gather(buf.data_ptr(), ti.data_ptr(), ts.data_ptr(), B, 0, st.data_ptr(), pi.data_ptr(), z.data_ptr())
    torch.cuda.synchronize()
    ws, wp, wz = ref.expected_gather(want, n, idx, sym, 0)
    assert np.array_equal(ref.bits(st.cpu().numpy().reshape(ws.shape)), ref.bits(ws))
    assert np.array_equal(ref.bits(pi.cpu().numpy().reshape(wp.shape)), ref.bits(wp))
    assert np.array_equal(ref.bits(z.cpu().numpy()), ref.bits(wz))
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. subtree reuse from non-empty positions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,S,tag", [(5, 4, 40, "ckpt_saved"), (9, 5, 24, None)], ids=["5x5-persistent", "9x9-lock-step"])
def test_subtree_reuse_from_given_positions(n, k, S, tag):
    """Only part of this can be pinned: the oracle cannot start a reuse game midway, so there is no reference for the plies
    after the first.  Checked: the first record of every game is Oracle.search at the start position (a claimed slot has a
    fresh root) with the game's noise, temperature and u of that ABSOLUTE ply; every ply's visits sum to S; the moves are
    legal and the game ends exactly where the rules say, with that result."""
    nn, G, seed0 = n * n, 7, 5700 + n
    gs = _oracle_games(n, k, S, G, seed0, tag)
    ms = _cut_points(gs, k)
    pos = _positions_of(gs, ms)
    o, onet = orc.Oracle(n, k, S, synthetic=tag is None), _oracle_net(n, tag)
    T = orc.selfplay_T_table(nn)
    e = _engine(n, k, S, 3, tag)
    e.set_subtree_reuse(True)
    e.set_start_positions(*pos)
    c = e.selfplay(G, seed0=seed0)
    nply, res = e.games()
    rec = e.records()
    assert c["plies"] == c["records"] == int(nply.sum()) and c["root_evals"] <= c["plies"]
    assert (rec["visits"].sum(axis=1) == S).all()
    off = 0
    for g in range(G):
        m, L = ms[g], int(nply[g])
        noise, us = orc.selfplay_tape(seed0 + g, n)
        noff = sum(nn - j for j in range(m))
        ro = o.search(onet, pos[0][g], int(pos[1][g]), int(pos[2][g]), T[m], noise[noff:noff + nn - m], us[m])
        assert np.array_equal(rec["boards"][off], pos[0][g]) and int(rec["lasts"][off]) == int(pos[2][g])
        assert np.array_equal(rec["visits"][off], ro["N"]) and np.array_equal(rec["pis"][off], ro["pi"])
        assert int(rec["actions"][off]) == ro["action"]
        board, pl, result = pos[0][g].copy(), int(pos[1][g]), 0
        for j in range(L):
            assert result == 0, f"game {g} was played on after its end"
            a = int(rec["actions"][off + j])
            assert np.array_equal(rec["boards"][off + j], board) and int(rec["movers"][off + j]) == pl and board[a] == 0
            board[a] = pl
            pl = 3 - pl
            result = _has_line(board, n, k) or (3 if (board != 0).all() else 0)
        assert result != 0 and int(res[g]) == result
        off += L
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. validation and errors
# ---------------------------------------------------------------------------------------------------------------------
def _raw_set(e, boards, players, lasts, first=0):
    return _capi.lib().az_set_start_positions(e.h, len(players), _capi._p(boards), _capi._p(players), _capi._p(lasts), first)


@pytest.mark.parametrize("fault", ["five_not_through_last", "full_board", "cell_value_3", "last_on_empty_cell", "player_3"])
def test_an_invalid_position_names_its_index_and_keeps_the_previous_setting(fault):
    n, k, nn = 7, 5, 49
    e = az.Engine(n, k, 16, 4, synthetic=True)
    good = games.positions_from_actions([[24], [24, 10, 3]], n)
    e.set_start_positions(*good)
    cnt, bad = 5, 3
    boards = np.zeros((cnt, nn), np.uint8); boards[:, 4] = 1
    players = np.full(cnt, 2, np.uint8); lasts = np.full(cnt, 4, np.int16)
    if fault == "five_not_through_last":
        boards[bad, [14, 15, 16, 17, 18]] = 2            # a row of five O; `last` is the X stone on cell 4
        boards[bad, [30, 31, 33, 40]] = 1
    elif fault == "full_board":
        boards[bad] = 1 + ((np.arange(nn) // 2 + np.arange(nn) // n) & 1)
        lasts[bad] = 0
    elif fault == "cell_value_3":
        boards[bad, 9] = 3
    elif fault == "last_on_empty_cell":
        lasts[bad] = 9
    else:
        players[bad] = 3
    assert _raw_set(e, boards, players, lasts) == -1                         # AZ_ERR_INVALID
    assert f"position {bad}" in _capi.lib().az_last_error(e.h).decode()
    with pytest.raises(az.AzError, match=rf"az_set_start_positions failed \(-1\).*position {bad}"):
        e.set_start_positions(boards, players, lasts)
    assert e.start_positions() == 2                                          # the previous setting is in force
    e.selfplay(2, seed0=1, max_plies=6)
    rec = e.records(); nply, _ = e.games()
    assert np.array_equal(rec["boards"][0], good[0][0]) and np.array_equal(rec["boards"][int(nply[0])], good[0][1])
    e.close()


def test_a_diagonal_line_of_win_length_is_refused_and_a_shorter_one_is_not():
    n, k = 6, 4
    e = az.Engine(n, k, 16, 4, synthetic=True)
    b = np.zeros((1, n * n), np.uint8)
    b[0, [3, 8, 13]] = 1; b[0, [0, 1, 2]] = 2                  # three on the anti-diagonal: fine
    e.set_start_positions(b, [1], [2])
    b[0, 18] = 1; b[0, 35] = 2                                 # the fourth
    with pytest.raises(az.AzError, match=r"\(-1\).*position 0.*already won"):
        e.set_start_positions(b, [1], [35])
    assert _raw_set(e, b, np.ones(1, np.uint8), np.full(1, 35, np.int16), first=-1) == -1
    e.close()


def test_max_plies_open_episodes_first_and_wrap():
    n, k, S, nn = 5, 4, 16, 25
    e = az.Engine(n, k, S, 4, synthetic=True)
    pos = games.positions_from_actions([[12], [12, 6, 7], [0, 24, 4, 20, 13]], n)
    e.set_start_positions(*pos, first=2)
    # a position at or beyond max_plies
    for cut in (5, 3):
        with pytest.raises(az.AzError, match=r"az_selfplay failed \(-1\).*max_plies"):
            e.selfplay(4, seed0=3, max_plies=cut)
        with pytest.raises(az.AzError, match=r"az_selfplay_begin failed \(-1\)"):
            e.selfplay_begin(4, seed0=3, max_plies=cut)
    # first and the modulo wrap with more games than positions: game g starts from position (2 + g) % 3
    G = 7
    c = e.selfplay(G, seed0=3, max_plies=6)
    nply, res = e.games()
    rec = e.records()
    off = 0
    for g in range(G):
        i = (2 + g) % 3
        stones = int((pos[0][i] != 0).sum())
        assert np.array_equal(rec["boards"][off], pos[0][i]) and int(rec["movers"][off]) == int(pos[1][i])
        assert int(rec["lasts"][off]) == int(pos[2][i])
        assert 1 <= int(nply[g]) <= 6 - stones and (int(nply[g]) == 6 - stones or int(res[g]) != 0)
        off += int(nply[g])
    assert off == c["records"] == c["plies"] == c["root_evals"]
    # while an episode is open the setting cannot change
    e.selfplay_begin(3, seed0=4)
    with pytest.raises(az.AzError, match=r"az_set_start_positions failed \(-6\)"):
        e.set_start_positions(*pos)
    with pytest.raises(az.AzError, match=r"az_set_start_positions failed \(-6\)"):
        e.clear_start_positions()
    e.selfplay_step(1)
    c = e.selfplay_end()
    # stopped early: every begun game reports the plies searched so far, the others none
    nply, _ = e.games()
    assert nply.tolist() == [1, 1, 1] and c["records"] == 3
    rec = e.records()
    assert [int((b != 0).sum()) for b in rec["boards"]] == [5, 1, 3]
    assert e.start_positions() == 3
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the Python seams (single process: first = 0)
# ---------------------------------------------------------------------------------------------------------------------
def _controller(tag, n=5):
    from alphazero_piskvorky_amd import net
    from alphazero_piskvorky_amd.controller import NeuralNetworkController
    m = net.GomokuNet(board_size=n)
    m.load_state_dict({kk: torch.tensor(v) for kk, v in weights_from_fixture(n, tag).items()})
    m.eval()
    return NeuralNetworkController(m, device=DEV)


def test_selfplay_manager_and_evaluator_take_start_positions():
    from alphazero_piskvorky_amd import constants
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    n, nn = 5, 25
    suite = games.positions_from_actions([[12, 6, 7], [0, 24], [11, 12, 13, 7, 17, 2]], n)
    stones = [3, 2, 6]
    params = {"num_simulations": 40, "c_puct": 2.0}
    mgr = SelfPlayManager(_controller("ckpt_saved"), DEV, mcts_params=params, concurrent_games=4, seed=91, start_positions=suite)
    packed, total, eng, _, _ = mgr.generate_packed(7)
    nply, _ = eng.games()
    rec = eng.records()
    assert total == mgr.last_counters["records"] == int(nply.sum())
    off = 0
    for g in range(7):
        i = g % 3
        assert np.array_equal(rec["boards"][off], suite[0][i]) and int(rec["lasts"][off]) == int(suite[2][i])
        assert int(nply[g]) <= nn - stones[i]
        off += int(nply[g])
    # the option taken away again: the same manager (and engine) plays the default episode
    mgr.start_positions = None
    mgr.generate_packed(7)
    plain = SelfPlayManager(_controller("ckpt_saved"), DEV, mcts_params=params, concurrent_games=4, seed=91)
    plain.generate_packed(7)
    a, b = mgr._engine.records(), plain._engine.records()
    assert all(np.array_equal(a[key], b[key]) for key in REC_KEYS) and not a["boards"][0].any()
    # arena: games 2i and 2i+1 start from position i mod 3, the second with the colours exchanged
    constants.NUM_EVAL_SIMULATIONS = 32
    try:
        ev = ModelEvaluator(device=DEV, seed=92, start_positions=suite)
        cand, base = _controller("ckpt_saved"), _controller("ckpt_0802")
        _, metrics = ev.evaluate(cand, base, num_games=7)
        r = ev.last_result
        assert metrics["total"] == 7
        for g in range(7):
            i = (g >> 1) % 3
            L = int(r["nply"][g])
            acts = r["actions"][g][:L]
            assert 0 < L <= nn - stones[i] and len(set(acts.tolist())) == L and not suite[0][i][acts].any()
        ev.start_positions = None
        ev.evaluate(cand, base, num_games=7)
        want = ModelEvaluator(device=DEV, seed=92)
        want.evaluate(cand, base, num_games=7)
        assert np.array_equal(ev.last_result["actions"], want.last_result["actions"])
    finally:
        constants.NUM_EVAL_SIMULATIONS = 200
