"""az_set_candidates on the GPU, against the numpy restatement in tests/candidates.py (which with radius 0 is the oracle's search,
tests/test_candidates_cpu.py).  Every comparison is exact: array_equal on visits, the float64 W, the float32 priors and pi, == on
actions and values.  tests/test_candidates_cpu.py shows that the compared cases are not vacuous.

Shapes: 5x5 has one cell per lane, 9x9 two, 15x15 four cells per lane and four words of the candidate plane.  The nets are the
seeded weights of tests/util.build_weights through the oracle's net; c_puct = 2."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import candidates as cd
from tests import forced
from tests.test_playout_cap_cpu import np_full
from tests.util import build_weights, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

S1 = 32
REC_KEYS = ("boards", "movers", "lasts", "actions", "pis", "visits", "z")
INVALID, STATE = r"\(-1\)", r"\(-6\)"


# ---------------------------------------------------------------------------------------------------------------------
# references (computed once, never modified)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net(n, k):
    sd = build_weights(n)
    return sd, cd.net_evaluator(n, k, orc.Net(n, sd))


@functools.lru_cache(maxsize=None)
def synth(n, k):
    return cd.synth_evaluator(n, k)


@functools.lru_cache(maxsize=None)
def tree(n, k, S, i, noised, radius, L=1, fk=0.0, ev="net"):
    p = cd.positions(n, k)[i]
    evaluate = synth(n, k) if ev == "synth" else net(n, k)[1]
    return cd.search(evaluate, n, k, S, p["board"], p["player"], p["last"], p["noise"] if noised else None, fk, L=L, radius=radius)


def engine(n, k, S, slots, real=True, **kw):
    e = az.Engine(n, k, S, slots, synthetic=not real, log_table=orc.numpy_log_table(S), c_puct=cd.C_PUCT, **kw)
    if real:
        e.load_weights(net(n, k)[0], 0)
    return e


def assert_search(r, want, p, S, what, fk=0.0):
    assert np.array_equal(r["N"], want["N"]), f"{what}: visits"
    assert np.array_equal(r["W"], want["W"]), f"{what}: W"
    assert np.array_equal(r["P"], want["P"]), f"{what}: priors"
    legal = np.flatnonzero(p["board"] == 0)
    counts = r["N"][legal]
    if fk > 0:
        counts, _ = _capi.forced_prune(fk, cd.C_PUCT, counts, r["W"][legal], r["P"][legal])
    pi, a = forced.pi_action(counts, p["board"], p["T"], p["u"], orc.numpy_log_table(S))
    assert r["pi"].dtype == np.float32 and np.array_equal(r["pi"], pi), f"{what}: pi"
    assert int(r["action"]) == a, f"{what}: action"


def batch(e, ps, noised=True):
    rb = e.search_batch(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps],
                        np.array([p["T"] for p in ps]), [p["noise"] for p in ps] if noised else None, [p["u"] for p in ps])
    return [{key: val[i] for key, val in rb.items()} for i in range(len(ps))]


def search(e, p, noised=True):
    return e.search(p["board"], p["player"], p["last"], p["T"], p["noise"] if noised else None, p["u"])


def episode(e, G, seed0, **kw):
    c = e.selfplay(G, seed0=seed0, **kw)
    nply, res = e.games()
    return dict(rec=e.records(), nply=nply.copy(), res=res.copy(), values=e.values(), c=c)


def same_episode(a, b):
    return (all(a["rec"][key].tobytes() == b["rec"][key].tobytes() for key in a["rec"]) and a["nply"].tobytes() == b["nply"].tobytes()
            and a["res"].tobytes() == b["res"].tobytes() and a["values"].tobytes() == b["values"].tobytes())


def assert_games(ep, games, what):
    assert ep["nply"].tolist() == [g["nply"] for g in games], f"{what}: plies per game"
    assert ep["res"].tolist() == [g["result"] for g in games], f"{what}: results"
    for key in REC_KEYS:
        exp = np.concatenate([g[key] for g in games])
        assert ep["rec"][key].shape == exp.shape and np.array_equal(ep["rec"][key], exp), f"{what}: {key}"
    assert np.array_equal(ep["values"], np.concatenate([g["values"] for g in games])), f"{what}: values"


# ---------------------------------------------------------------------------------------------------------------------
# 1. off is off
# ---------------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    """never set, and set then 0: an episode of 6 games at 5x5 byte for byte a fresh engine's, and the persistent kernel is back"""
    def run(touch):
        e = engine(5, 4, 24, 4)
        assert e.candidates() == 0
        if touch:
            e.set_candidates(2)
            assert e.candidates() == 2
            search(e, cd.positions(5, 4)[2])
            assert e.persistent() == 0
            e.set_candidates(0)
            assert e.candidates() == 0
        out = [search(e, p) for p in cd.positions(5, 4)]
        ep = episode(e, 6, 6100)
        pers = e.persistent()
        e.close()
        return out, ep, pers
    a, b = run(False), run(True)
    for x, y in zip(a[0], b[0]):
        assert x.keys() == y.keys() and all(np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes() for key in x)
    assert same_episode(a[1], b[1])
    assert a[2] == b[2] and a[2] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. single searches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", ["1", "2", "n-1"])
@pytest.mark.parametrize("n,k", cd.SIZES)
def test_single_searches_equal_the_restatement(n, k, radius):
    """the empty board, a 1-, a 6- and an 11-stone position, with and without noise, through az_search and az_search_batch (the
    four positions of the size in one batch).  The lock-step kernels on every size."""
    r_ = n - 1 if radius == "n-1" else int(radius)
    e = engine(n, k, S1, 4)
    e.set_candidates(r_)
    ps = cd.positions(n, k)
    for noised in (True, False):
        rbs = batch(e, ps, noised)
        assert e.persistent() == 0
        for i, (p, rb) in enumerate(zip(ps, rbs)):
            r = search(e, p, noised)
            assert e.persistent() == 0
            want = tree(n, k, S1, i, noised, r_)
            for got, what in ((r, "az_search"), (rb, "az_search_batch")):
                assert_search(got, want, p, S1, f"{n}x{n} radius {r_} position {i} noise {noised} {what}")
            C = cd.candidate_mask(p["board"], n, r_)
            assert not r["N"][~C].any() and not r["P"][~C].any()
    e.close()


@pytest.mark.parametrize("radius", [1, 2])
def test_wrap_and_word_boundaries(radius):
    """15x15, one stone at a corner, a row end, either side of a plane word's end, the last row's start and the last cell"""
    n, k, S = 15, 5, 16
    e = engine(n, k, S, 8)
    e.set_candidates(radius)
    cells = (0, 14, 63, 64, 128, 210, 224)
    ps = [cd.one_stone(n, c) for c in cells]
    for c, p, rb in zip(cells, ps, batch(e, ps, noised=False)):
        want = cd.search(net(n, k)[1], n, k, S, p["board"], p["player"], p["last"], None, radius=radius)
        assert_search(rb, want, p, S, f"stone at {c}, radius {radius}")
        C = cd.candidate_mask(p["board"], n, radius)
        assert int((rb["P"] > 0).sum()) == int(C.sum()) and not rb["P"][~C].any()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. virtual loss, deep engines, the other nets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", cd.SIZES)
def test_virtual_loss_batches(n, k):
    """L = 4 at S = 32.  Radius 1, at 15x15 radius 2: there the batches change the 6- and the 11-stone search, as they do at radius
    1 on the smaller boards (on an almost empty board 32 simulations in batches of 4 build the tree the sequential search builds)"""
    radius = 2 if n == 15 else 1
    e = engine(n, k, S1, 4)
    e.set_virtual_loss(4)
    e.set_candidates(radius)
    ps = cd.positions(n, k)
    differ = 0
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        want, seq = tree(n, k, S1, i, True, radius, L=4), tree(n, k, S1, i, True, radius)
        differ += not (np.array_equal(want["N"], seq["N"]) and np.array_equal(want["W"], seq["W"]))
        r = search(e, p) if i == 2 else rb
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, want, p, S1, f"virtual loss 4, {n}x{n} position {i} {what}")
    assert differ >= 2
    e.close()


@pytest.mark.parametrize("n,k,L", [(5, 4, 1), (15, 5, 1), (5, 4, 4)])
def test_deep_engines(n, k, L):
    """az_create_deep at S = 1100, the synthetic evaluator (candidates keep their prior, the rest is 0); with L = 4 the in-flight
    counts live beside the tree"""
    S = 1100 if L == 1 else 64
    p = cd.positions(n, k)[2]
    want = cd.search(synth(n, k), n, k, S, p["board"], p["player"], p["last"], p["noise"], L=L, radius=1)
    plain = cd.search(synth(n, k), n, k, S, p["board"], p["player"], p["last"], p["noise"], L=L)
    assert not np.array_equal(want["N"], plain["N"])
    e = engine(n, k, S, 1, real=False, deep=True)
    e.set_virtual_loss(L)
    e.set_candidates(1)
    r = search(e, p)
    assert e.persistent() == 0
    assert_search(r, want, p, S, f"deep {n}x{n} S = {S} L = {L}")
    e.close()


def test_the_5x5_checkpoint():
    n, k = 5, 4
    sd = weights_from_fixture(5, "ckpt_saved")
    ev = cd.net_evaluator(n, k, orc.Net(n, sd))
    e = az.Engine(n, k, S1, 4, log_table=orc.numpy_log_table(S1), c_puct=cd.C_PUCT)
    e.load_weights(sd, 0)
    e.set_candidates(1)
    ps = cd.positions(n, k)
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        want = cd.search(ev, n, k, S1, p["board"], p["player"], p["last"], p["noise"], radius=1)
        assert_search(rb, want, p, S1, f"5x5 checkpoint, position {i}")
    e.close()


def test_residual_block_net_5x5():
    from alphazero_piskvorky_amd.net import fold_resnet_state_dict
    from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict
    n, k = 5, 4
    sd = synthetic_resnet_state_dict(n)
    ev = cd.net_evaluator(n, k, orc.Net(n, resnet_tensors=fold_resnet_state_dict(sd)))
    p = cd.positions(n, k)[2]
    want = cd.search(ev, n, k, S1, p["board"], p["player"], p["last"], p["noise"], radius=1)
    e = az.Engine(n, k, S1, 2, log_table=orc.numpy_log_table(S1), c_puct=cd.C_PUCT, model="resnet")
    e.load_weights(sd, 0)
    e.set_candidates(1)
    assert_search(search(e, p), want, p, S1, "ResidualBlock net")
    assert e.persistent() == 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. whole games
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_games(n, k, S, G, seed0, radius, max_plies=0, cap=None, fk=0.0):
    return tuple(cd.selfplay_game(net(n, k)[1], n, k, S, seed0 + g, radius, fk, True, cap, np_full, max_plies=max_plies) for g in range(G))


def test_whole_games_5x5():
    """6 games on 4 slots in 2 lanes (refill happens), S = 24, radius 1"""
    n, k, S, G, seed0 = 5, 4, 24, 6, 6200
    games = ref_games(n, k, S, G, seed0, 1)
    e = engine(n, k, S, 4, engines=2)
    e.set_candidates(1)
    ep = episode(e, G, seed0)
    assert e.persistent() == 0
    assert_games(ep, games, "5x5")
    assert all(cd.moves_lie_in_candidates(g["boards"], g["actions"], n, 1) for g in games)
    e.close()


def test_whole_games_9x9():
    n, k, S, G, seed0 = 9, 5, 16, 3, 6300
    games = ref_games(n, k, S, G, seed0, 2, max_plies=8)
    e = engine(n, k, S, 4)
    e.set_candidates(2)
    assert_games(episode(e, G, seed0, max_plies=8), games, "9x9")
    e.close()


@pytest.mark.parametrize("delta", [True, False], ids=["delta", "full"])
def test_whole_games_15x15(delta):
    n, k, S, G, seed0 = 15, 5, 12, 2, 6400
    games = ref_games(n, k, S, G, seed0, 1, max_plies=6)
    e = engine(n, k, S, 2)
    e.set_delta_eval(delta)
    e.set_candidates(1)
    assert_games(episode(e, G, seed0, max_plies=6), games, f"15x15 delta {delta}")
    if delta:
        assert e.delta_stats()["delta"] > 0
    e.close()


@pytest.mark.parametrize("cap,fk", [((8, 500), 0.0), (None, 2.0)], ids=["cap", "forced"])
def test_games_with_options(cap, fk):
    """under the playout cap (F = 8, 500 permille: the FAST plies search an un-noised root); with forced playouts k = 2 and
    pruning (a child with P = 0 is never forced, and the pruning leaves the edges without a visit alone)"""
    n, k, S, G, seed0 = 5, 4, 24, 4, 6500
    games = ref_games(n, k, S, G, seed0, 1, cap=cap, fk=fk)
    e = engine(n, k, S, 4)
    e.set_candidates(1)
    if cap:
        e.set_playout_cap(cap[0], cap[1] / 1000)
        full = np.concatenate([np_full(seed0 + i, np.arange(g["nply"]), cap[1]) for i, g in enumerate(games)])
        assert full.any() and not full.all()
    if fk:
        e.set_forced_playouts(fk, True)
    assert_games(episode(e, G, seed0), games, f"cap {cap} forced {fk}")
    e.close()


def test_the_evaluation_cache_changes_nothing_and_leaf_symmetry_does():
    n, k, S, G, seed0 = 5, 4, 24, 6, 6200

    def run(cache, symmetry):
        e = engine(n, k, S, 4)
        e.set_candidates(1)
        e.set_eval_cache(1 << 12 if cache else 0)
        e.set_leaf_symmetry(symmetry)
        ep = episode(e, G, seed0)
        hits = ep["c"]["cache_hits"]
        e.close()
        return ep, hits
    (plain, _), (cached, hits), (sym, _) = run(False, False), run(True, False), run(False, True)
    assert hits > 0 and same_episode(plain, cached)
    assert not same_episode(plain, sym) and int(sym["nply"].sum()) > 0
    assert cd.moves_lie_in_candidates(sym["rec"]["boards"], sym["rec"]["actions"], n, 1)
    assert_games(plain, ref_games(n, k, S, G, seed0, 1), "one lane")


def test_a_cache_filled_without_the_option_serves_it():
    """entries hold logits: a search whose evaluations are all cache hits from a run with the option off equals the restatement"""
    n, k = 5, 4
    e = engine(n, k, S1, 1)
    e.set_eval_cache(1 << 12)
    p = cd.positions(n, k)[2]
    search(e, p)
    e.set_candidates(n - 1)                           # the same leaves are reachable: every legal cell is a candidate
    r = search(e, p)
    assert e.counters()["cache_hits"] > 0
    assert_search(r, tree(n, k, S1, 2, True, n - 1), p, S1, "cache carried over")
    e.close()


def test_a_game_continued_from_ply_m_a_resigned_game_and_the_exact_rule(monkeypatch):
    from tests import win_rule
    from tests.test_resign_gpu import choose_threshold, first_cross
    n, k, S, G, seed0, m = 5, 4, 24, 6, 6200, 3
    e = engine(n, k, S, 4)
    e.set_candidates(1)
    full = episode(e, G, seed0)
    offs = np.concatenate([[0], np.cumsum(full["nply"])[:-1]])
    assert (full["nply"] > m).all()
    rec = full["rec"]
    e.set_start_positions(rec["boards"][offs + m], rec["movers"][offs + m], rec["lasts"][offs + m])
    cont = episode(e, G, seed0)
    assert np.array_equal(cont["nply"], full["nply"] - m) and np.array_equal(cont["res"], full["res"])
    keep = np.concatenate([np.arange(o + m, o + L) for o, L in zip(offs, full["nply"])])
    for key in REC_KEYS:
        assert np.array_equal(cont["rec"][key], rec[key][keep]), key
    e.clear_start_positions()
    vals = np.split(full["values"].astype(np.float64), np.cumsum(full["nply"])[:-1])
    thr, crossing = choose_threshold(vals)
    e.set_resign(thr)
    res = episode(e, G, seed0)
    assert crossing
    for g in range(G):
        c = first_cross(vals[g], thr)
        natural = c < 0 or c == full["nply"][g] - 1
        assert res["nply"][g] == (full["nply"][g] if natural else c + 1), g
    e.set_resign(0.0)
    win_rule.use_rule(monkeypatch, "exact")
    games = tuple(cd.selfplay_game(net(n, k)[1], n, k, S, seed0 + g, 1) for g in range(4))
    e.set_win_rule("exact")
    assert_games(episode(e, 4, seed0), games, "exact win rule")
    e.close()


def test_arena_moves_lie_in_the_candidates_on_every_engine_shape():
    n, k, S, G, seed0, radius = 5, 4, 24, 8, 6600, 1
    cand, base = weights_from_fixture(n, "ckpt_saved"), weights_from_fixture(n, "ckpt_0802")
    out = []
    for slots, lanes in ((8, 1), (8, 2), (3, 1)):
        e = az.Engine(n, k, S, slots, log_table=orc.numpy_log_table(S), c_puct=cd.C_PUCT, engines=lanes)
        e.load_weights(cand, 0); e.load_weights(base, 1)
        e.set_candidates(radius)
        tally = e.arena(G, seed0=seed0, temperature_table=orc.arena_T_table(n * n))
        rec = e.records()
        assert cd.moves_lie_in_candidates(rec["boards"], rec["actions"], n, radius)
        assert not any(v[~cd.candidate_mask(b, n, radius)].any() for b, v in zip(rec["boards"], rec["visits"]))
        out.append((tally["wins"], tally["losses"], tally["draws"], {key: rec[key].tobytes() for key in ("boards", "actions", "visits", "pis")}))
        e.close()
    assert out[0] == out[1] == out[2]


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals, ranges and state
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_pairs_in_both_orders():
    e = engine(5, 4, 16, 2)
    want = episode(e, 2, 77)
    from tests.test_external_eval_gpu import CpuEvaluator, net_eval
    partners = ((lambda: e.set_subtree_reuse(True), lambda: e.set_subtree_reuse(False), "subtree reuse"),
                (lambda: e.set_gumbel(4, 50.0, 1.0), lambda: e.set_gumbel(0), "Gumbel"),
                (lambda: e.set_solver(True), lambda: e.set_solver(False), "solver"),
                (lambda: e.set_selection(fpu=0.2), lambda: e.set_selection(on=False), "selection rule"))
    for on, off, word in partners:
        e.set_candidates(1)
        with pytest.raises(az.AzError, match=INVALID) as ei:
            on()
        assert word in str(ei.value) and "candidate moves" in str(ei.value)
        e.set_candidates(0)                              # switching off is always allowed
        on()
        with pytest.raises(az.AzError, match=INVALID) as ei:
            e.set_candidates(1)
        assert word in str(ei.value) and e.candidates() == 0
        off()
    e.set_candidates(1)
    with pytest.raises(az.AzError, match=INVALID):
        e.set_threat_search(4, 64)                       # stays refused without the solver, and the solver with the option
    p = cd.positions(5, 4)[1]
    with pytest.raises(az.AzError, match=INVALID) as ei:
        e.search_callback(p["board"], p["player"], p["last"], 1.0, lambda cells, pl, la: (np.full(25, 0.04, np.float32), 0.0), None, 0.5)
    assert "candidate moves" in str(ei.value)
    e.set_candidates(0)
    assert same_episode(episode(e, 2, 77), want)         # the engine afterwards plays the episode it played before
    e.close()
    # the external evaluator, in both orders
    e = az.Engine(5, 4, 16, 2, log_table=orc.numpy_log_table(16), c_puct=cd.C_PUCT)
    e.set_candidates(1)
    with pytest.raises(az.AzError, match=INVALID) as ei:
        CpuEvaluator(e, net_eval(orc.Net(5, net(5, 4)[0])))
    assert "candidate moves" in str(ei.value) and "external evaluator" in str(ei.value)
    e.set_candidates(0)
    CpuEvaluator(e, net_eval(orc.Net(5, net(5, 4)[0])))
    with pytest.raises(az.AzError, match=INVALID) as ei:
        e.set_candidates(1)
    assert "external evaluator" in str(ei.value) and e.candidates() == 0
    e.close()


def test_ranges_and_an_open_episode():
    L = _capi.lib()
    e = engine(5, 4, 16, 2, real=False)
    e.set_candidates(2)
    for bad in (-1, 5, 14, 1 << 20):
        assert L.az_set_candidates(e.h, bad) == -1, bad
        assert e.candidates() == 2                       # the previous setting is kept
    with pytest.raises(az.AzError, match=INVALID):
        e.set_candidates(5)
    for good in (1, 4, 0, 3):
        assert L.az_set_candidates(e.h, good) == 0 and e.candidates() == good
    assert L.az_get_candidates(e.h, None) == 0
    e.selfplay_begin(2, seed0=1)
    assert e.persistent() == 0
    with pytest.raises(az.AzError, match=STATE):
        e.set_candidates(1)
    with pytest.raises(az.AzError, match=STATE):
        e.set_candidates(0)
    e.selfplay_step(1 << 20)
    e.selfplay_end()
    assert e.candidates() == 3
    e.close()


def test_a_captured_ply_graph_does_not_outlive_the_setting():
    e = engine(9, 5, 16, 2, real=False)

    def run():
        e.selfplay(2, seed0=9, max_plies=6)
        return e.records()["visits"].copy()
    e.set_candidates(1)
    a = run()
    e.set_candidates(0)
    b = run()
    e.set_candidates(2)
    c = run()
    e.set_candidates(1)
    d = run()
    assert np.array_equal(a, d)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    assert np.array_equal(b, np.concatenate([orc.Oracle(9, 5, 16, c_puct=cd.C_PUCT, synthetic=True).selfplay_game(
        None, *orc.selfplay_tape(9 + g, 9, maxply=6), maxply=6)["visits"] for g in range(2)]))
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the seams
# ---------------------------------------------------------------------------------------------------------------------
def _controller():
    from tests.test_external_eval_gpu import _controller as fixture_controller
    return fixture_controller("ckpt_saved")


def test_mcts_run_and_run_many():
    from alphazero_piskvorky_amd import constants as consts
    from alphazero_piskvorky_amd.controller import make_policy_value_fn
    from alphazero_piskvorky_amd.games import Gomoku
    from alphazero_piskvorky_amd.mcts import MCTS
    n, k, S = 5, 4, S1
    ctrl = _controller()
    states = []
    for p in cd.positions(n, k):
        g = Gomoku(n, k)
        g.cells = p["board"].reshape(n, n).copy()
        g.current_player = consts.X if p["player"] == 1 else consts.O
        g.last_action = None if p["last"] < 0 else (p["last"] // n, p["last"] % n)
        states.append(g)
    e = az.Engine(n, k, S, 1, log_table=orc.numpy_log_table(S), c_puct=cd.C_PUCT)
    e.load_weights(weights_from_fixture(5, "ckpt_saved"), 0)
    e.set_candidates(1)

    def engine_level(seed, noised):
        np.random.seed(seed)
        out = []
        for p in cd.positions(n, k):
            noise = np.random.dirichlet([0.3] * int((p["board"] == 0).sum())) if noised else None
            u = np.random.random_sample()
            out.append(e.search(p["board"], p["player"], p["last"], 1.0, noise, u))
        return out
    m = MCTS(make_policy_value_fn(ctrl), S, cd.C_PUCT, candidates={"radius": 1})
    plain = MCTS(make_policy_value_fn(ctrl), S, cd.C_PUCT)
    for noised in (False, True):
        want = engine_level(7, noised)
        np.random.seed(7)
        got = [m.run(g, 1.0, add_root_noise=noised) for g in states]
        np.random.seed(7)
        many = m.run_many(states, 1.0, add_root_noise=noised)
        np.random.seed(7)
        off = [plain.run(g, 1.0, add_root_noise=noised) for g in states]
        for w, a, b in zip(want, got, many):
            assert np.array_equal(a[0].reshape(-1), w["pi"]) and a[1] == (int(w["action"]) // n, int(w["action"]) % n)
            assert np.array_equal(b[0].reshape(-1), w["pi"]) and b[1] == a[1]
        assert any(not np.array_equal(a[0], o[0]) for a, o in zip(got, off))
    assert m._engine.candidates() == 1 and m._batch_engine.candidates() == 1 and plain._engine.candidates() == 0
    e.close()


def test_self_play_manager_and_a_cached_engine_brought_back_to_off():
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    n, k, S, G, seed0 = 5, 4, S1, 4, 6700
    ctrl = _controller()
    e = az.Engine(n, k, S, 4, log_table=orc.numpy_log_table(S), c_puct=cd.C_PUCT)
    e.load_weights(weights_from_fixture(5, "ckpt_saved"), 0)
    e.set_candidates(1)
    e.selfplay(G, seed0=seed0)
    want_on = e.records()
    e.set_candidates(0)
    e.selfplay(G, seed0=seed0)
    want_off = e.records()
    e.close()
    m = SelfPlayManager(ctrl, "cuda:0", mcts_params={"num_simulations": S, "c_puct": cd.C_PUCT}, concurrent_games=4, seed=seed0,
                        candidates={"radius": 1})
    _, total, eng, _, _ = m.generate_packed(G)
    assert eng.candidates() == 1 and eng.persistent() == 0
    got = eng.records()
    for key in REC_KEYS:
        assert np.array_equal(got[key], want_on[key]), key
    assert total == len(want_on["actions"])
    m.candidates = None                                 # the cached engine that played with the option goes back to off
    _, _, eng2, _, _ = m.generate_packed(G)
    assert eng2 is eng and eng.candidates() == 0 and eng.persistent() > 0
    got = eng.records()
    for key in REC_KEYS:
        assert np.array_equal(got[key], want_off[key]), key
    m.candidates = {"radius": 1}
    m.selection = {"fpu": 0.2}                          # a cached engine never meets both: the seam refuses first
    with pytest.raises(ValueError, match="selection rule"):
        m.generate_packed(G)
    m.candidates = None                                 # ... and from candidates to the selection rule on the same engine
    _, _, eng3, _, _ = m.generate_packed(G)
    assert eng3 is eng and eng.candidates() == 0 and eng.selection()["on"]
    m.selection, m.candidates = None, {"radius": 2}
    _, _, eng4, _, _ = m.generate_packed(G)
    assert eng4 is eng and eng.candidates() == 2 and not eng.selection()["on"]


def test_model_evaluator_arena(monkeypatch):
    from alphazero_piskvorky_amd import constants as consts
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator, temperature_schedule
    n, k, G, seed0, S = 5, 4, 4, 6800, S1
    ctrl = _controller()
    sd = weights_from_fixture(5, "ckpt_saved")
    e = az.Engine(n, k, S, G, c_puct=consts.EVAL_EXPLORATION_CONSTANT, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    e.load_weights(sd, 1)
    T = np.array([float(temperature_schedule(m)) for m in range(n * n + 2)], dtype=np.float64)
    e.set_candidates(1)
    want = e.arena(G, seed0=seed0, temperature_table=T)
    want_rec = e.records()
    e.close()
    monkeypatch.setattr(consts, "NUM_EVAL_SIMULATIONS", S)
    ev = ModelEvaluator(device="cuda:0", seed=seed0, candidates={"radius": 1})
    _, metrics = ev.evaluate(ctrl, ctrl, num_games=G)
    assert (metrics["wins"], metrics["losses"], metrics["draws"]) == (want["wins"], want["losses"], want["draws"])
    got = ev._engine.records()
    for key in ("actions", "visits", "pis"):
        assert np.array_equal(got[key], want_rec[key]), key
    assert ev._engine.candidates() == 1
    ev.candidates = None
    ev.evaluate(ctrl, ctrl, num_games=G)
    assert ev._engine.candidates() == 0


def test_train_loop_runs_with_the_option():
    from alphazero_piskvorky_amd import constants, train
    saved = (constants.BATCHES_PER_EPISODE, constants.NUM_EPOCHS, constants.BATCH_SIZE)
    constants.BATCHES_PER_EPISODE, constants.NUM_EPOCHS, constants.BATCH_SIZE = 2, 1, 256
    try:
        hist = train.run(episodes=1, games=8, sims=12, eval_games=4, device="cuda:0", seed=3, log=lambda *_: None, candidates={"radius": 1})
    finally:
        constants.BATCHES_PER_EPISODE, constants.NUM_EPOCHS, constants.BATCH_SIZE = saved
    assert len(hist) == 1 and hist[0]["examples"] > 0 and np.isfinite(hist[0]["loss"])
    assert hist[0]["total"] == 4
