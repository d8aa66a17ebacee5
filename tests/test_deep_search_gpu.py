"""Deep searches (az_create_deep): more than 1024 simulations per move, held bit for bit to the oracle at the same S.
Above 1024 simulations the engine runs the DEEP tree kernels (sqrt table from HBM, in-flight counts of virtual-loss
batching beside the tree), launches each ply kernel by kernel and never picks the persistent search kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.util import load, synth_eval_codes, weights_from_fixture

import alphazero_piskvorky_amd as az


def _deep(n, k, S, slots=1, synthetic=False, tag=None, **kw):
    e = az.Engine(n, k, S, slots, synthetic=synthetic, log_table=orc.numpy_log_table(S), deep=True, **kw)
    sd = None
    if tag is not None:
        sd = weights_from_fixture(n, tag)
        e.load_weights(sd, 0)
    return e, sd


def _positions(n):
    """the empty board and two mid-game positions of the fixture game of this size"""
    z = load(f"netgame_{n}x{4 if n == 5 else 5}.npz")
    out = [(np.zeros(n * n, np.uint8), 1, -1)]
    for i in (1, len(z["ply"]) // 2):
        out.append((z["board"][i].astype(np.uint8), int(z["player"][i]), int(z["last"][i])))
    return out


def _same_search(r, ro, what):
    assert np.array_equal(r["N"], ro["N"]), f"{what}: visit counts"
    assert np.array_equal(r["W"], ro["W"]) and np.array_equal(r["P"], ro["P"]), what
    assert np.array_equal(r["pi"], ro["pi"]) and r["action"] == ro["action"], what


@pytest.mark.parametrize("n,k,S,tag", [(5, 4, 1025, "ckpt_saved"), (5, 4, 4096, "ckpt_saved"), (9, 5, 1600, "seeded"),
                                       (15, 5, 1600, "seeded"), (15, 5, 10_000, None)])
def test_deep_single_search_bit_exact_vs_oracle(n, k, S, tag):
    synth = tag is None
    e, sd = _deep(n, k, S, synthetic=synth, tag=tag)
    o = orc.Oracle(n, k, S, synthetic=synth)
    onet = None if synth else orc.Net(n, sd)
    rs = np.random.RandomState(S + n)
    for i, (board, pl, last) in enumerate(_positions(n)):
        for noisy in (False, True):
            noise = rs.dirichlet([0.3] * int((board == 0).sum())) if noisy else None
            r = e.search(board, pl, last, 1.0, noise, 0.43)
            ro = o.search(onet, board, pl, last, 1.0, noise, 0.43)
            _same_search(r, ro, f"{n}x{n} S={S} position {i} noise={noisy}")
            assert int(r["N"].sum()) == S
    e.close()


@pytest.mark.parametrize("n,k,S,Ls", [(5, 4, 4096, (2, 8, 32)), (15, 5, 10_000, (2, 8, 32))])
def test_deep_virtual_loss_bit_exact_vs_oracle(n, k, S, Ls):
    rs = np.random.RandomState(7)
    board = np.zeros(n * n, np.uint8)
    if n == 5:
        for a in (12, 6, 18):
            board[a] = 1 if a != 6 else 2
    pl = 2 if n == 5 else 1
    for L in Ls:
        e, _ = _deep(n, k, S, synthetic=True)
        e.set_virtual_loss(L)
        o = orc.Oracle(n, k, S, synthetic=True, virtual_loss=L)
        noise = rs.dirichlet([0.3] * int((board == 0).sum()))
        r = e.search(board, pl, 18 if n == 5 else -1, 1.0, noise, 0.61)
        ro = o.search(None, board, pl, 18 if n == 5 else -1, 1.0, noise, 0.61)
        _same_search(r, ro, f"{n}x{n} S={S} L={L}")
        assert int(r["N"].sum()) == S
        e.close()


@pytest.mark.parametrize("n,k,S", [(5, 4, 4096), (15, 5, 10_000)])
@pytest.mark.parametrize("L", [2, 8, 32])
def test_deep_virtual_loss_first_search_counters_vs_oracle(n, k, S, L):
    """The first search of a game (one ply) from the empty board: the records and the work counters, duplicate leaves
    (simulations that met a leaf already pending in their batch) included, equal the oracle's."""
    G = 2
    e, _ = _deep(n, k, S, slots=G, synthetic=True)
    e.set_virtual_loss(L)
    o = orc.Oracle(n, k, S, synthetic=True, virtual_loss=L)
    c, _, tot = _selfplay_vs_oracle(e, o, None, n, G, 60 + L, cut=1)
    assert (c["expansions"], c["terminal_hits"], c["depth_sum"], c["duplicate_leaves"], c["simulations"]) == \
        (tot["expansions"], tot["terminal_hits"], tot["depth_sum"], tot["dup_sims"], tot["sims"])
    assert c["simulations"] == S * G
    e.close()


def _selfplay_vs_oracle(e, o, onet, n, G, seed0, cut=0):
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    rec = e.records(); nply, res = e.games()
    off, tot = 0, dict(expansions=0, terminal_hits=0, depth_sum=0, dup_sims=0, sims=0)
    for g in range(G):
        noise, us = orc.selfplay_tape(seed0 + g, n)
        r = o.selfplay_game(onet, noise, us, maxply=cut if cut else None, game=seed0 + g)
        Lg = int(nply[g]); sl = slice(off, off + Lg)
        assert Lg == r["nply"] and int(res[g]) == r["result"], f"game {g}"
        for key in ("actions", "boards", "visits", "pis", "z"):
            assert np.array_equal(rec[key][sl], r[key]), f"game {g}: {key} differs from the oracle"
        for key in tot:
            tot[key] += r["counters"][key]
        off += Lg
    return c, rec, tot


def test_deep_selfplay_games_with_refills_and_virtual_loss():
    n, k, S = 5, 4, 1600
    e, sd = _deep(n, k, S, slots=4, tag="ckpt_saved")
    c, _, _ = _selfplay_vs_oracle(e, orc.Oracle(n, k, S), orc.Net(n, sd), n, 6, 900)
    assert c["simulations"] == S * c["plies"]
    e.set_virtual_loss(8)
    c, _, tot = _selfplay_vs_oracle(e, orc.Oracle(n, k, S, virtual_loss=8), orc.Net(n, sd), n, 6, 900)
    assert c["duplicate_leaves"] == tot["dup_sims"]
    e.close()


def test_deep_selfplay_9x9_cut_leaf_symmetry_and_cache():
    n, k, S, G, cut = 9, 5, 1600, 2, 4
    e, sd = _deep(n, k, S, slots=2, tag="seeded")
    _, rec0, _ = _selfplay_vs_oracle(e, orc.Oracle(n, k, S), orc.Net(n, sd), n, G, 40, cut)
    e.set_eval_cache(1 << 14)
    e.selfplay(G, seed0=40, max_plies=cut)
    rec1 = e.records()
    for key in rec0:
        assert np.array_equal(rec0[key], rec1[key]), f"evaluation cache changed {key}"
    e.set_eval_cache(0)
    e.set_leaf_symmetry(True)
    _selfplay_vs_oracle(e, orc.Oracle(n, k, S, leaf_sym=True), orc.Net(n, sd), n, G, 40, cut)
    e.close()


def test_deep_arena_game_by_game():
    n, k, S, G, seed0 = 5, 4, 1600, 6, 77
    e, cand = _deep(n, k, S, slots=4, tag="ckpt_saved")
    base = weights_from_fixture(n, "ckpt_0802")
    e.load_weights(base, 1)
    r = e.arena(G, seed0=seed0, temperature_table=orc.arena_T_table(n * n))
    o = orc.Oracle(n, k, S); oc, ob = orc.Net(n, cand), orc.Net(n, base)
    for g in range(G):
        us = np.random.RandomState(seed0 + g).random_sample(n * n)
        ro = o.arena_game(oc, ob, g, us)
        assert int(r["nply"][g]) == ro["nply"] and int(r["results"][g]) == ro["result"], f"game {g}"
        assert np.array_equal(r["actions"][g][:ro["nply"]], ro["actions"])
    e.close()


def test_deep_search_callback_vs_oracle():
    n, k, S = 5, 4, 2000
    e, _ = _deep(n, k, S)

    def fn(cells, player, last):
        codes = np.where(cells == 0, 0, np.where(cells == player, 1, 2)).astype(np.uint8)
        return synth_eval_codes(codes, last, n)

    o = orc.Oracle(n, k, S, synthetic=True)
    rs = np.random.RandomState(3)
    board = np.zeros(n * n, np.uint8)
    noise = rs.dirichlet([0.3] * (n * n))
    r = e.search_callback(board, 1, -1, 1.0, fn, noise, 0.52)
    ro = o.search(None, board, 1, -1, 1.0, noise, 0.52)
    assert np.array_equal(r["N"], ro["N"]) and np.array_equal(r["pi"], ro["pi"]) and r["action"] == ro["action"]
    e.close()


def test_deep_tiny_board_never_takes_the_persistent_kernel():
    """3x3 at S = 1030: records equal the oracle's on the lock-step pipeline.  search_prepare refuses S > 1024 explicitly
    (k_search's static sqrt table holds 1026 entries); the guard is defensive -- the LDS-size check alone already refuses
    the persistent kernel on every board above about S = 940 (at 3x3: 28 KiB static + 1031 rows x 144 B > 160 KiB)."""
    n, k, S, G = 3, 3, 1030, 3
    e, _ = _deep(n, k, S, slots=2, synthetic=True)
    _selfplay_vs_oracle(e, orc.Oracle(n, k, S, synthetic=True), None, n, G, 5)
    assert az._capi.lib().az_get_persistent(e.h) == 0
    e.close()


def test_deep_refusals():
    e, _ = _deep(5, 4, 2000, synthetic=True)
    with pytest.raises(az.AzError, match="subtree reuse"):
        e.set_subtree_reuse(True)
    e.close()
    with pytest.raises(az.AzError, match=r"\(-1\): .*needs \d+ bytes"):
        az.Engine(15, 5, 65_534, 65_536, synthetic=True, deep=True)


def test_deep_engine_at_default_depth_is_the_default_engine():
    n, k, S, G = 5, 4, 400, 6
    sd = weights_from_fixture(n, "ckpt_saved")
    recs, pers = [], []
    for deep in (False, True):
        e = az.Engine(n, k, S, 4, log_table=orc.numpy_log_table(S), deep=deep)
        e.load_weights(sd, 0)
        e.selfplay(G, seed0=11)
        recs.append(e.records())
        pers.append(az._capi.lib().az_get_persistent(e.h))
        e.close()
    for key in recs[0]:
        assert np.array_equal(recs[0][key], recs[1][key]), key
    assert pers[0] == pers[1]


def test_deep_shims():
    import torch
    from alphazero_piskvorky_amd import constants as C, games, net
    from alphazero_piskvorky_amd.controller import NeuralNetworkController, make_policy_value_fn
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator
    from alphazero_piskvorky_amd.mcts import MCTS
    from alphazero_piskvorky_amd.self_play import SelfPlayManager

    def ctrl(tag):
        m = net.GomokuNet(board_size=5)
        m.load_state_dict({k: torch.tensor(v) for k, v in weights_from_fixture(5, tag).items()})
        m.eval()
        return NeuralNetworkController(m, device="cuda:0")

    n, k, S = 5, 4, 2000
    cand = ctrl("ckpt_saved")
    m = MCTS(make_policy_value_fn(cand), num_simulations=S, c_puct=2.0)
    o = orc.Oracle(n, k, S)
    onet = orc.Net(n, weights_from_fixture(n, "ckpt_saved"))
    g = games.Gomoku(n, k)
    for ply in range(2):
        np.random.seed(500 + ply)
        pi, action = m.run(g, temperature=1.0, add_root_noise=True)
        np.random.seed(500 + ply)
        noise = np.random.dirichlet([0.3] * int((g.cells == 0).sum())); u = np.random.random_sample()
        ro = o.search(onet, g.cells, g.player_code(), g.last_index(), 1.0, noise, u)
        assert np.array_equal(pi.reshape(-1), ro["pi"]) and action[0] * n + action[1] == ro["action"], f"ply {ply}"
        g = g.apply_action(action)

    spm = SelfPlayManager(cand, "cuda:0", mcts_params={"num_simulations": 1600}, seed=3)
    ex = spm.generate_self_play(2)
    assert len(ex) > 0 and all(s.shape == (4, n, n) and p.shape == (n, n) and z in (-1, 0, 1) for s, p, z in ex)
    with pytest.raises(ValueError, match="subtree_reuse"):
        SelfPlayManager(cand, "cuda:0", mcts_params={"num_simulations": 1600}, seed=3, subtree_reuse=True).generate_self_play(1)

    saved = C.NUM_EVAL_SIMULATIONS
    C.NUM_EVAL_SIMULATIONS = 1600
    try:
        ev = ModelEvaluator(game_class=games.Gomoku, print_games=False, device="cuda:0", seed=21)
        wr, metrics = ev.evaluate(cand, ctrl("ckpt_0802"), num_games=4)
    finally:
        C.NUM_EVAL_SIMULATIONS = saved
    o = orc.Oracle(n, k, 1600)
    ob = orc.Net(n, weights_from_fixture(n, "ckpt_0802"))
    w = l = d = 0
    for gi in range(4):
        us = np.random.RandomState(21 + gi).random_sample(n * n)
        ro = o.arena_game(onet, ob, gi, us)
        w += ro["result"] == 1; l += ro["result"] == 2; d += ro["result"] == 3
    assert (metrics["wins"], metrics["losses"], metrics["draws"]) == (w, l, d)
