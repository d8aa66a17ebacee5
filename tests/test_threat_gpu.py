"""The root threat search on the GPU (az_set_threat_search, az_threat_batch), against az_threat_solve on the host and the numpy
restatement in tests/threat.py (both held to each other and to brute force by tests/test_threat_cpu.py).  The searches are
compared with the solver's restatement started from the premarked root statuses, its evaluator being the engine's own
az_net_eval, so every comparison is exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import threat as th
from tests.test_solver_gpu import C_PUCT, NetEval, _clean_env, _refused, assert_search, engine
from tests.util import build_weights

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

SHAPES = {"3x3": (3, 3, 3), "5x5": (5, 4, 8), "7x7": (7, 4, 14), "9x9": (9, 5, 30), "15x15": (15, 5, 40)}     # n, k, stones
COUNT, SLOTS = 70, 16             # five waves, the last one of 6 positions
KEYS = ("status", "move", "depth", "nodes")


def threat_engine(n, k, S=32, slots=4, depth=8, budget=256, rule="freestyle", **kw):
    e = engine(n, k, S, slots, **kw)
    if rule != "freestyle":
        e.set_win_rule(rule)
    e.set_threat_search(depth, budget)
    assert e.threat_search() == (depth, budget)
    return e


@functools.lru_cache(maxsize=None)
def sample(shape, rule):
    n, k, stones = SHAPES[shape]
    return th.positions(n, k, rule, stones, COUNT, 50 + n)


def host(boards, players, n, k, rule, depth, budget):
    rows = [_capi.threat_solve(b, n, k, rule, int(p), depth, budget) for b, p in zip(boards, players)]
    return {key: np.array([r[key] for r in rows]) for key in KEYS + ("edges",)}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel on its own
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", th.RULES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_threat_batch_equals_the_host_and_the_restatement(shape, rule):
    """70 positions on 16 slots.  Against az_threat_solve at (6, unlimited), (4, 3) and (1, 1); against the restatement at (4, 3)
    and at unlimited budget with depth 6, at 15x15 depth 4 (the restatement's cost grows with the board)."""
    n, k, _ = SHAPES[shape]
    boards, players = sample(shape, rule)
    e = az.Engine(n, k, 8, SLOTS, log_table=orc.numpy_log_table(8))     # no weights, no solver: the kernel needs neither
    e.set_win_rule(rule)
    found = 0
    for depth, budget in ((6, 65535), (4, 3), (1, 1)):
        got = e.threat_batch(boards, players, depth, budget)
        want = host(boards, players, n, k, rule, depth, budget)
        for key in KEYS + ("edges",):
            assert np.array_equal(got[key], want[key]), (shape, rule, depth, budget, key, np.flatnonzero((got[key] != want[key]).reshape(COUNT, -1).any(1)))
        assert got["edges"].dtype == np.int8 and not got["edges"][boards != 0].any()
        found += int((got["depth"] >= 2).sum())
    assert found > 0 or n == 3
    for depth, budget in ((4 if n == 15 else 6, 65535), (4, 3)):
        got = e.threat_batch(boards, players, depth, budget)
        for i, (b, p) in enumerate(zip(boards, players)):
            want = th.solve(b, n, k, rule, int(p), depth, budget)
            assert all(got[key][i] == want[key] for key in KEYS) and np.array_equal(got["edges"][i], want["edges"]), (shape, rule, depth, budget, i)
    e.close()


def test_threat_batch_null_outputs_empty_batch_and_refusals():
    n, k, _ = SHAPES["9x9"]
    boards, players = sample("9x9", "freestyle")
    e = az.Engine(n, k, 8, SLOTS, log_table=orc.numpy_log_table(8), engines=2)     # two lanes share the waves
    assert e.lanes() == 2
    full = e.threat_batch(boards, players, 6, 300)
    want = host(boards, players, n, k, "freestyle", 6, 300)
    for key in KEYS + ("edges",):
        assert np.array_equal(full[key], want[key]), key
        assert np.array_equal(e.threat_batch(boards, players, 6, 300, outputs=(key,))[key], full[key]), key      # every other output NULL
    assert e.threat_batch(boards, players, 6, 300, outputs=()) == {}
    assert len(e.threat_batch(np.zeros((0, n * n), np.uint8), np.zeros(0, np.uint8))["status"]) == 0
    # a position that is already won: refused with its index, nothing is searched
    bad = boards[:6].copy()
    bad[3] = 0
    bad[3, :5] = 1
    bad[3, 9:13] = 2
    with pytest.raises(_capi.AzError) as ex:
        e.threat_batch(bad, players[:6])
    assert "(-1)" in str(ex.value) and "position 3" in str(ex.value) and "already won" in str(ex.value)
    e.set_win_rule("exact")
    six = bad.copy()
    six[3, 5] = 1                                                 # a run of six: no winner under the exact rule
    six[3, 13:15] = 2
    assert e.threat_batch(six, players[:6])["status"][3] == th.UNKNOWN
    e.set_win_rule("freestyle")
    for kw in (dict(max_depth=0), dict(max_depth=17), dict(node_budget=0), dict(node_budget=65536)):
        _refused(lambda: e.threat_batch(boards[:2], players[:2], **kw))
    cells = boards[:2].copy()
    cells[1, 0] = 3
    _refused(lambda: e.threat_batch(cells, players[:2]))
    _refused(lambda: e.threat_batch(boards[:2], np.array([1, 0], np.uint8)))
    _refused(lambda: e.threat_batch(np.ones((1, n * n), np.uint8), np.array([1], np.uint8)))      # no legal action
    assert np.array_equal(e.threat_batch(boards, players, 6, 300)["nodes"], full["nodes"])         # the engine still works
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. az_search and az_search_batch with the option on
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def search_positions(case):
    """crafted: the depth-3 win.  Random: the first position of the sample with a win of depth >= 2, the first with LOSS marks
    around a single block, the first lost one and the first without any mark (whichever of them the sample holds)."""
    n, k = {"crafted-9x9": (9, 5), "crafted-15x15": (15, 5), "5x5": (5, 4), "9x9": (9, 5), "15x15": (15, 5)}[case]
    if case.startswith("crafted"):
        board, player, _ = th.crafted_depth3(n)
        picked = [(board, player)] * 2                           # at T = 1 and at T -> 0
    else:
        boards, players = sample(case, "freestyle")
        res = host(boards, players, n, k, "freestyle", 8, 256)
        kinds = (res["depth"] >= 2, (res["status"] == th.UNKNOWN) & (res["edges"] == th.LOSS).any(1), res["status"] == th.LOSS,
                 ~res["edges"].any(1))
        picked = [(boards[int(np.flatnonzero(m)[0])], int(players[int(np.flatnonzero(m)[0])])) for m in kinds if m.any()]
        assert len(picked) >= 3
    out = []
    for i, (board, player) in enumerate(picked):
        rs = np.random.RandomState(2000 * n + i)
        out.append(dict(board=board, player=int(player), last=th.last_of(board, player), noise=rs.dirichlet([0.3] * int((board == 0).sum())),
                        u=float(rs.random_sample()), T=(1.0, 1e-9)[i % 2]))
    return n, k, tuple(out)


@pytest.mark.parametrize("noised", [True, False], ids=["noise", "no-noise"])
@pytest.mark.parametrize("case", ["crafted-9x9", "crafted-15x15", "5x5", "9x9", "15x15"])
def test_searches_equal_the_restatement(case, noised, monkeypatch):
    _clean_env(monkeypatch)
    n, k, ps = search_positions(case)
    S = 48
    ev = NetEval(n, k, "seeded")
    e = threat_engine(n, k, S, 4)
    rb = e.search_batch(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps],
                        np.array([p["T"] for p in ps]), [p["noise"] for p in ps] if noised else None, [p["u"] for p in ps])
    assert e.persistent() == 0                                    # lock-step, 5x5 included
    eb, rootb = e.last_proof()
    stops_b, stats_b = e.solver_stops(), e.threat_stats()
    stops = 0
    marked = 0
    for i, p in enumerate(ps):
        info = {}
        want = th.threat_search(ev, n, k, S, p["board"], p["player"], p["last"], p["noise"] if noised else None, "freestyle", 8, 256, info)
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"] if noised else None, p["u"])
        assert e.persistent() == 0
        assert_search(r, e.last_proof(), want, p, S, f"{case} position {i} az_search")
        assert_search({key: val[i] for key, val in rb.items()}, (eb[i], rootb[i]), want, p, S, f"{case} position {i} az_search_batch")
        assert e.solver_stops() == info["stops"]
        t, st = want["threat"], e.threat_stats()
        assert st == dict(win_roots=int(t["status"] == th.WIN), lost_roots=int(t["status"] == th.LOSS),
                          block_roots=int(t["depth"] == 0 and len(t["Wd"]) == 1), exhausted=int(t["nodes"] > 256), nodes=t["nodes"])
        stops += info["stops"]
        marked += int(t["edges"].any())
        if case.startswith("crafted"):
            move = t["move"]
            assert t["depth"] == 3 and r["N"][move] == S and r["N"].sum() == S and r["W"][move] == float(S)
            assert e.last_proof()[1] == th.WIN and r["action"] == move
            # T -> 0: exactly one-hot; T = 1: the unchanged temperature path leaves every emptied cell log(0 + 1e-8)
            assert (r["pi"][move] == 1.0 and np.count_nonzero(r["pi"]) == 1) if p["T"] < 1e-7 else (np.delete(r["pi"], move).max() < 1e-8)
            assert e.solver_stops() == S and info["evals"] == 1
            c = e.counters()
            assert c["expansions"] == 0 and c["trunk_boards"] == 1 and c["root_evals"] == 1     # the root's evaluation and nothing else
    assert stops_b == stops and marked >= len(ps) - 1
    assert stats_b["nodes"] > 0
    e.close(); ev.close()


def test_the_crafted_win_records_value_one():
    """one ply of self-play from the crafted position: value exactly +1, proof WIN, depth 3, pi one-hot on the move"""
    n, k, S = 9, 5, 32
    board, player, move = th.crafted_depth3(n)
    e = threat_engine(n, k, S, 2)
    e.set_start_positions(board[None], [player], [th.last_of(board, player)])
    e.selfplay(1, seed0=5, max_plies=int((board != 0).sum()) + 1)
    rec = e.records()
    assert len(rec["actions"]) == 1 and int(rec["actions"][0]) == move and rec["pis"][0][move] == 1.0 and rec["visits"][0][move] == S
    assert e.values()[0] == 1.0 and e.proofs()[0] == th.WIN and e.threats().tolist() == [3]
    assert e.threat_stats()["win_roots"] == 1 and e.solver_stops() == S
    e.close()


def test_deep_engine():
    n, k, S = 9, 5, 1100
    _, _, ps = search_positions("9x9")
    board, player, move = th.crafted_depth3(n)
    ev = NetEval(n, k, "seeded")
    e = threat_engine(n, k, S, 1, deep=True)
    p = dict(board=board, player=player, last=th.last_of(board, player), T=1e-9, u=0.5)
    want = th.threat_search(ev, n, k, S, board, player, p["last"], None, "freestyle", 8, 256)
    r = e.search(board, player, p["last"], p["T"], None, p["u"])
    assert_search(r, e.last_proof(), want, p, S, "deep crafted")
    assert r["N"][move] == S and e.solver_stops() == S
    p = ps[1]                                                     # LOSS marks around a single block: every simulation goes through it
    want = th.threat_search(ev, n, k, 1100, p["board"], p["player"], p["last"], None, "freestyle", 8, 256)
    r = e.search(p["board"], p["player"], p["last"], p["T"], None, p["u"])
    assert_search(r, e.last_proof(), want, p, S, "deep block")
    e.close(); ev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. whole games
# ---------------------------------------------------------------------------------------------------------------------
# Carry-through -- the side that once holds a threat-proven WIN root wins the game -- needs every later root search of that side
# to find a win again.  A search of depth d + 1 finds a win wherever one of depth d does (each candidate's sub-search only gets
# deeper), so the follow-up search at max_depth succeeds where the first search's recursion at max_depth - 1 did, PROVIDED its
# node budget lasts: it looks one level deeper than the recursion did and can need more nodes (on the host: 1 of 282 wins of
# depth >= 3 on random 9x9 / 30-stone positions is lost that way at max_depth 8, node_budget 256; tests/test_threat_cpu.py has the
# property without the budget).  So the whole games run with a budget that these boards do not reach, and say so: no search of
# the episode may be exhausted.
GAME_DEPTH, GAME_BUDGET = 6, 65535


def check_games(e, n, k, rule, depth=GAME_DEPTH, budget=GAME_BUDGET):
    rec, (nply, res), threats, proofs, values = e.records(), e.games(), e.threats(), e.proofs(), e.values()
    assert len(threats) == len(proofs) == len(values) == int(nply.sum()) and threats.dtype == np.int8
    seen = dict(win=0, deep=0, block=0, lost=0)
    off = 0
    for g, L in enumerate(nply):
        holder = 0                                                # the side that held a threat-proven WIN root
        for i in range(off, off + int(L)):
            board, mover, a = rec["boards"][i], int(rec["movers"][i]), int(rec["actions"][i])
            t = _capi.threat_solve(board, n, k, rule, mover, depth, budget)
            assert threats[i] == t["depth"], (g, i)
            if t["status"] != th.UNKNOWN:
                assert proofs[i] == t["status"] and values[i] == (1.0 if t["status"] == th.WIN else -1.0), (g, i)
            if t["status"] == th.WIN:
                assert t["edges"][a] == th.WIN, (g, i)            # every move of a WIN root is a WIN cell
                holder = holder or mover
                seen["win"] += 1
                seen["deep"] += t["depth"] >= 2
            Wa = th.win_set(board, n, k, rule, mover)
            Wd = th.win_set(board, n, k, rule, 3 - mover)
            if Wa:
                assert a in Wa, (g, i)                            # nobody passes a completion by
            elif len(Wd) == 1:
                assert a == Wd[0], (g, i)                         # ... or leaves a single opposing completion open
                seen["block"] += 1
            elif len(Wd) >= 2:
                assert proofs[i] == th.LOSS and values[i] == -1.0
                seen["lost"] += 1
        if holder:
            assert int(res[g]) == holder, (g, holder, int(res[g]))      # carry-through: the holder of a proven WIN root wins
        off += int(L)
    return seen


@pytest.mark.parametrize("rule", th.RULES)
@pytest.mark.parametrize("n,k,S", [(5, 4, 64), (9, 5, 32)])
def test_whole_games(n, k, S, rule):
    e = threat_engine(n, k, S, 8, GAME_DEPTH, GAME_BUDGET, rule=rule)
    c = e.selfplay(8, seed0=700)
    assert e.persistent() == 0 and c["simulations"] == S * c["plies"]
    seen = check_games(e, n, k, rule)
    st = e.threat_stats()
    assert seen["win"] == st["win_roots"] > 0 and seen["lost"] == st["lost_roots"] and st["exhausted"] == 0
    e.close()


def test_whole_games_under_the_playout_cap():
    n, k, S = 9, 5, 32
    e = threat_engine(n, k, S, 4, GAME_DEPTH, GAME_BUDGET)
    e.set_playout_cap(8, 0.4, export_full_only=False)
    e.selfplay(6, seed0=710)
    sims = e.sims()
    assert (sims == 8).any() and (sims == S).any()
    seen = check_games(e, n, k, "freestyle")                      # FAST and FULL plies alike
    assert seen["win"] > 0 and e.threat_stats()["exhausted"] == 0
    e.close()


def test_arena_games():
    n, k, S, G = 9, 5, 32, 6
    e = threat_engine(n, k, S, 4, GAME_DEPTH, GAME_BUDGET)
    e.load_weights(build_weights(n, seed=4321), 1)
    a = e.arena(G, seed0=21)
    assert int(a["nply"].sum()) == len(e.threats())
    seen = check_games(e, n, k, "freestyle")
    assert seen["win"] > 0 and e.threat_stats()["exhausted"] == 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the option off again, and the launch paths
# ---------------------------------------------------------------------------------------------------------------------
def test_option_off_after_on_is_the_solver_alone():
    n, k, S, G = 5, 4, 32, 6
    outs = []
    for toggle in (False, True):
        e = engine(n, k, S, 4)
        if toggle:
            e.set_threat_search(6, 100)
            e.selfplay(2, seed0=1)
            assert e.persistent() == 0 and len(e.threats()) == e.last_records
            e.set_threat_search(0)
            assert e.threat_search() == (0, 0)
        c = e.selfplay(G, seed0=77)
        outs.append((e.records(), e.values(), e.proofs(), e.games(), e.persistent(), e.solver_stops(),
                     {key: c[key] for key in ("simulations", "expansions", "terminal_hits")}))
        with pytest.raises(_capi.AzError) as ex:
            e.threats()
        assert "(-6)" in str(ex.value)                            # AZ_ERR_STATE: the episode ran without the option
        assert e.threat_stats() == dict(win_roots=0, lost_roots=0, block_roots=0, exhausted=0, nodes=0)
        e.close()
    a, b = outs
    assert a[4] == b[4] > 0 and a[5] == b[5] and a[6] == b[6]    # the persistent kernel is back
    for key in a[0]:
        assert a[0][key].tobytes() == b[0][key].tobytes(), key
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


def _episode(n, k, S, G):
    e = threat_engine(n, k, S, 4)
    e.selfplay(G, seed0=1234)
    out = (e.records(), e.values(), e.proofs(), e.threats(), e.games(), e.solver_stops(), e.threat_stats())
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def default_episode(n, k, S, G):
    return _episode(n, k, S, G)


@pytest.mark.parametrize("switch", ["AZ_GRAPH", "AZ_COMPACT"])
def test_launch_paths_give_identical_episodes(switch, monkeypatch):
    n, k, S, G = 9, 5, 24, 6
    _clean_env(monkeypatch)
    want = default_episode(n, k, S, G)
    monkeypatch.setenv(switch, "0")
    got = _episode(n, k, S, G)
    for key in want[0]:
        assert np.array_equal(got[0][key], want[0][key]), (switch, key)
    assert all(np.array_equal(got[i], want[i]) for i in (1, 2, 3)) and all(np.array_equal(x, y) for x, y in zip(got[4], want[4]))
    assert got[5] == want[5] and got[6] == want[6] and want[6]["nodes"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    n, k, S = 5, 4, 16
    e = engine(n, k, S, 2, solver=False)
    _refused(e.set_threat_search, 8, 256)                         # it needs the solver
    e.set_threat_search(0)                                        # switching off is always fine
    e.set_solver(True)
    e.set_threat_search(8, 256)
    _refused(e.set_solver, False)                                 # ... and the solver stays while it is on
    assert e.solver() and e.threat_search() == (8, 256)
    for args in ((-1, 256), (17, 256), (8, 0), (8, 65536), (8, -5)):
        _refused(e.set_threat_search, *args)
        assert e.threat_search() == (8, 256)                      # the previous setting is kept
    others = (("subtree reuse", lambda: e.set_subtree_reuse(True), lambda: e.set_subtree_reuse(False)),
              ("virtual loss", lambda: e.set_virtual_loss(4), lambda: e.set_virtual_loss(1)),
              ("forced playouts", lambda: e.set_forced_playouts(2.0), lambda: e.set_forced_playouts(0.0)),
              ("gumbel", lambda: e.set_gumbel(8), lambda: e.set_gumbel(0)))
    for name, on, off in others:
        _refused(on)                                              # the solver's refused pairs are its own: threat search first
        e.set_threat_search(0)
        e.set_solver(False)
        on()
        _refused(e.set_solver, True)                              # the other option first: no solver,
        _refused(e.set_threat_search, 8, 256)                     # ... so no threat search
        off()
        e.set_solver(True)
        e.set_threat_search(8, 256)
    # an open episode
    e.selfplay_begin(2, seed0=3)
    for fn, args in ((e.set_threat_search, (4, 10)), (e.set_threat_search, (0, 0)),
                     (lambda: e.threat_batch(np.zeros((1, n * n), np.uint8), np.array([1], np.uint8)), ())):
        with pytest.raises(_capi.AzError) as ex:
            fn(*args)
        assert "(-6)" in str(ex.value), str(ex.value)             # AZ_ERR_STATE
    e.selfplay_step(2)
    mid = e.threat_stats()
    e.selfplay_step(1 << 20)
    e.selfplay_end()
    end = e.threat_stats()
    assert all(mid[key] <= end[key] for key in end) and len(e.threats()) == e.last_records
    e.close()
    s = az.Engine(n, k, S, 2, synthetic=True, log_table=orc.numpy_log_table(S))
    _refused(s.set_solver, True)
    _refused(s.set_threat_search, 8, 256)
    s.close()


def test_the_batched_external_evaluator_is_refused_in_both_orders():
    import torch
    n, k, S = 5, 4, 16
    e = threat_engine(n, k, S, 2)
    planes = torch.zeros((2, 4, n, n), dtype=torch.float32, device="cuda")
    policy = torch.zeros((2, n * n), dtype=torch.float32, device="cuda")
    value = torch.zeros(2, dtype=torch.float32, device="cuda")
    args = (planes.data_ptr(), policy.data_ptr(), value.data_ptr(), 2, lambda net, count: None)
    _refused(e.set_external_evaluator, *args)
    e.set_threat_search(0)
    e.set_solver(False)
    e.set_external_evaluator(*args)
    _refused(e.set_solver, True)
    _refused(e.set_threat_search, 8, 256)
    e.clear_external_evaluator()
    e.close()


def test_the_python_seams_take_the_option():
    from alphazero_piskvorky_amd.mcts import MCTS
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    with pytest.raises(ValueError):
        MCTS(lambda s: None, 16, 2.0, threat_search={"max_depth": 4})          # without solver=True
    with pytest.raises(ValueError):
        SelfPlayManager(None, "cuda", threat_search=True)
    m = SelfPlayManager(None, "cuda", solver=True, threat_search={"max_depth": 4, "node_budget": 64})
    assert m.threat_search == dict(max_depth=4, node_budget=64)
