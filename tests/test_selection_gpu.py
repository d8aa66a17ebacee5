"""az_set_selection on the GPU, against the numpy restatement in tests/selection.py (which with the rule off is the oracle's search,
tests/test_selection_cpu.py).  Every comparison is exact: array_equal on visits, the float64 W, the float32 priors and pi, ==
on actions.  tests/test_selection_cpu.py shows that none of the compared cases is vacuous: in every single search the rule
changes the root visits and picks another child than the plain rule both at the root and below it.

Parameter sets (tests/selection.py SETS): (a) fpu 0.2, root 0; (b) factor 1, base 50; (c) both, fpu_root 0.1; (d) on with all four
zero-valued parameters, the parent-value urgency alone.  c_puct = 3 throughout (selection.C_PUCT says why)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import forced
from tests import selection as sel
from tests.test_playout_cap_cpu import np_full
from tests.util import weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

C_PUCT = sel.C_PUCT
S1 = 64
REC_KEYS = ("boards", "movers", "lasts", "actions", "pis", "visits", "z")
INVALID, STATE = r"\(-1\)", r"\(-6\)"


# ---------------------------------------------------------------------------------------------------------------------
# references (computed once, never modified)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synth(n, k):
    return orc.Oracle(n, k, 1, synthetic=True).synth_eval


def oracle_net_eval(n, k, onet):
    o = orc.Oracle(n, k, 1)

    def evaluate(board, player, last):
        _, P, v = onet.eval(o.encode(board, player, last))
        return P, v
    return evaluate


@functools.lru_cache(maxsize=None)
def net5():
    sd = weights_from_fixture(5, "ckpt_saved")
    return sd, oracle_net_eval(5, 4, orc.Net(5, sd))


@functools.lru_cache(maxsize=None)
def tree(n, k, S, i, noised, name, L=1, fk=0.0, ev="synth"):
    p = sel.positions(n, k)[i]
    evaluate = net5()[1] if ev == "net5" else synth(n, k)
    return sel.search(evaluate, n, k, S, p["board"], p["player"], p["last"], p["noise"] if noised else None, fk, C_PUCT, L=L,
                      sel=sel.SETS[name] if name else None)


def engine(n, k, S, slots, real=False, **kw):
    e = az.Engine(n, k, S, slots, synthetic=not real, log_table=orc.numpy_log_table(S), c_puct=C_PUCT, **kw)
    if real:
        e.load_weights(net5()[0], 0)
    return e


def expect_pi(r, p, S, name, fk=0.0):
    """pi and the action the rule asks for, from the ENGINE's root statistics; under forced playouts from az_forced_prune's counts
    given c(count)"""
    legal = np.flatnonzero(p["board"] == 0)
    counts = r["N"][legal]
    if fk > 0:
        c = sel.prune_c(C_PUCT, sel.SETS[name] if name else None, S, counts.sum())
        counts, removed = _capi.forced_prune(fk, c, counts, r["W"][legal], r["P"][legal])
        assert removed == int(r["N"].sum() - counts.sum())
    return forced.pi_action(counts, p["board"], p["T"], p["u"], orc.numpy_log_table(S)), counts


def assert_search(r, want, p, S, name, what, fk=0.0):
    assert np.array_equal(r["N"], want["N"]), f"{what}: visits"
    assert np.array_equal(r["W"], want["W"]), f"{what}: W"
    assert np.array_equal(r["P"], want["P"]), f"{what}: priors"
    (pi, a), _ = expect_pi(r, p, S, name, fk)
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
@pytest.mark.parametrize("n,k", [(5, 4), (15, 5)])
def test_off_is_off(n, k):
    """an engine on which the option was set and cleared searches and plays byte for byte like one never touched, and at 5x5 the
    persistent kernel is back"""
    def run(touch):
        e = engine(n, k, S1 if n == 5 else 32, 4)
        assert e.selection() == dict(on=False, fpu=0.0, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0)
        if touch:
            e.set_selection(**sel.SETS["c"])
            assert e.selection() == dict(sel.SETS["c"], on=True)
            search(e, sel.positions(n, k)[1])
            assert e.persistent() == 0
            e.set_selection(on=False)
            assert e.selection() == dict(sel.SETS["c"], on=False)         # the parameters stay as last set
        out = [search(e, p) for p in sel.positions(n, k)] + batch(e, sel.positions(n, k), noised=False)
        pers = e.persistent()
        ep = episode(e, 6, 5100, max_plies=0 if n == 5 else 4)
        pers = (pers, e.persistent())
        e.close()
        return out, ep, pers
    a, b = run(False), run(True)
    for x, y in zip(a[0], b[0]):
        assert x.keys() == y.keys() and all(np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes() for key in x)
    assert same_episode(a[1], b[1])
    assert a[2] == b[2] and (a[2][1] > 0) == (n == 5)


# ---------------------------------------------------------------------------------------------------------------------
# 2. single searches, the synthetic evaluator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sel.SETS))
@pytest.mark.parametrize("n,k", sel.SIZES)
def test_single_searches_equal_the_restatement(n, k, name):
    """the empty board, a 6-stone and an 11-stone position, with and without noise, through az_search and az_search_batch.  5x5: one
    cell per lane; 9x9: two; 15x15: four.  The lock-step kernels on every size."""
    e = engine(n, k, S1, 4)
    e.set_selection(**sel.SETS[name])
    ps = sel.positions(n, k)
    for noised in (True, False):
        rbs = batch(e, ps, noised)
        assert e.persistent() == 0
        for i, (p, rb) in enumerate(zip(ps, rbs)):
            r = search(e, p, noised)
            assert e.persistent() == 0
            for got, what in ((r, "az_search"), (rb, "az_search_batch")):
                assert_search(got, tree(n, k, S1, i, noised, name), p, S1, name, f"{n}x{n} set {name} position {i} noise {noised} {what}")
            assert not np.array_equal(r["N"], tree(n, k, S1, i, noised, None)["N"])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the real nets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", [False, True], ids=["plain", "eval-cache"])
def test_real_net_5x5(cache):
    """the 5x5 fixture checkpoint through the oracle's net; with the evaluation cache the later searches take the root's value
    from a cache hit"""
    n, k = 5, 4
    e = engine(n, k, S1, 4, real=True)
    e.set_selection(**sel.SETS["c"])
    if cache:
        e.set_eval_cache(1 << 10)
    ps = sel.positions(n, k)
    for rep in range(2 if cache else 1):
        for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
            r = search(e, p)
            for got, what in ((r, "az_search"), (rb, "az_search_batch")):
                assert_search(got, tree(n, k, S1, i, True, "c", ev="net5"), p, S1, "c", f"real net, position {i} {what} round {rep}")
    if cache:
        assert e.counters()["cache_hits"] > 0
    e.close()


def test_native_net_15x15_with_and_without_delta_evaluation():
    """one 15x15 position, the plain net: delta evaluation on and off agree with each other and with the restatement"""
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    n, k, S = 15, 5, 48
    sd = synthetic_state_dict(n)
    p = sel.positions(n, k)[2]
    info = {}
    want = sel.search(oracle_net_eval(n, k, orc.Net(n, sd)), n, k, S, p["board"], p["player"], p["last"], p["noise"], 0.0, C_PUCT,
                      sel=sel.SETS["c"], info=info)
    assert info["root_diff"] > 0 and info["below_diff"] > 0
    got = {}
    for delta in (True, False):
        e = az.Engine(n, k, S, 4, log_table=orc.numpy_log_table(S), c_puct=C_PUCT)
        e.load_weights(sd, 0)
        e.set_delta_eval(delta)
        e.set_selection(**sel.SETS["c"])
        got[delta] = search(e, p)
        if delta:
            assert e.delta_stats()["delta"] > 0
        assert_search(got[delta], want, p, S, "c", f"15x15 native net, delta {delta}")
        e.close()
    assert all(np.asarray(got[True][key]).tobytes() == np.asarray(got[False][key]).tobytes() for key in got[True])


def test_residual_block_net_5x5():
    from alphazero_piskvorky_amd.net import fold_resnet_state_dict
    from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict
    n, k, S = 5, 4, 48
    sd = synthetic_resnet_state_dict(n)
    p = sel.positions(n, k)[1]
    info = {}
    want = sel.search(oracle_net_eval(n, k, orc.Net(n, resnet_tensors=fold_resnet_state_dict(sd))), n, k, S, p["board"], p["player"],
                      p["last"], p["noise"], 0.0, C_PUCT, sel=sel.SETS["c"], info=info)
    assert info["root_diff"] + info["below_diff"] > 0
    e = az.Engine(n, k, S, 2, log_table=orc.numpy_log_table(S), c_puct=C_PUCT, model="resnet")
    e.load_weights(sd, 0)
    e.set_selection(**sel.SETS["c"])
    assert_search(search(e, p), want, p, S, "c", "ResidualBlock net")
    assert e.persistent() == 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. virtual-loss batching, 5. deep engines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 8])
def test_virtual_loss_batches(L):
    """9x9: the rule on N + in-flight and W - in-flight; a child with an in-flight visit only counts as visited"""
    n, k = 9, 5
    e = engine(n, k, S1, 4)
    e.set_virtual_loss(L)
    e.set_selection(**sel.SETS["c"])
    ps = sel.positions(n, k)
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        r = search(e, p)
        want = tree(n, k, S1, i, True, "c", L=L)
        assert not (np.array_equal(want["N"], tree(n, k, S1, i, True, "c")["N"]) and np.array_equal(want["W"], tree(n, k, S1, i, True, "c")["W"]))
        assert not np.array_equal(want["N"], tree(n, k, S1, i, True, None, L=L)["N"])
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, want, p, S1, "c", f"virtual loss {L}, position {i} {what}")
    e.close()


@pytest.mark.parametrize("S,L", [(64, 1), (1100, 1), (64, 4)])
def test_deep_engines(S, L):
    """az_create_deep: the DEEP kernels read sqrt and c(count) from the global tables; 16-bit counts at S = 1100; with L = 4 the
    in-flight counts live beside the tree"""
    n, k = 5, 4
    p = sel.positions(n, k)[1]
    info = {}
    want = sel.search(synth(n, k), n, k, S, p["board"], p["player"], p["last"], p["noise"], 0.0, C_PUCT, L=L, sel=sel.SETS["c"], info=info)
    assert info["root_diff"] > 0 and info["below_diff"] > 0
    e = engine(n, k, S, 1, deep=True)
    e.set_virtual_loss(L)
    e.set_selection(**sel.SETS["c"])
    r = search(e, p)
    assert e.persistent() == 0
    assert_search(r, want, p, S, "c", f"deep S = {S} L = {L}")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. forced playouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", sel.SIZES)
def test_forced_playouts_prune_at_c_of_the_count(n, k):
    """k = 2 with pruning, set (c): the engine's pruned counts are az_forced_prune's given c(count), and the restatement's by the
    rule's definition"""
    e = engine(n, k, S1, 4)
    e.set_forced_playouts(2.0, True)
    e.set_selection(**sel.SETS["c"])
    ps = sel.positions(n, k)
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        r = search(e, p)
        want = tree(n, k, S1, i, True, "c", fk=2.0)
        legal = np.flatnonzero(p["board"] == 0)
        c = sel.prune_c(C_PUCT, sel.SETS["c"], S1, S1)
        assert c > C_PUCT
        by_rule = forced.prune(2.0, c, want["N"][legal], want["W"][legal], want["P"][legal])
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, want, p, S1, "c", f"forced, {n}x{n} position {i} {what}", fk=2.0)
            _, counts = expect_pi(got, p, S1, "c", 2.0)
            assert np.array_equal(counts, by_rule)
        assert (by_rule < want["N"][legal]).any()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. whole self-play games
# ---------------------------------------------------------------------------------------------------------------------
FK = 4.0
GAME_CASES = [pytest.param(5, 4, 6, 5300, None, 0.0, id="5x5"), pytest.param(9, 5, 3, 5400, None, 0.0, id="9x9"),
              pytest.param(5, 4, 6, 5300, (8, 500), 0.0, id="5x5-cap"), pytest.param(9, 5, 3, 5400, (8, 500), 0.0, id="9x9-cap"),
              pytest.param(5, 4, 6, 5300, None, FK, id="5x5-forced"), pytest.param(9, 5, 3, 5400, None, FK, id="9x9-forced")]


@functools.lru_cache(maxsize=None)
def ref_games(n, k, S, G, seed0, cap=None, fk=0.0, name="c"):
    return tuple(sel.selfplay_game(synth(n, k), n, k, S, seed0 + g, sel.SETS[name], fk, True, cap, np_full) for g in range(G))


@pytest.mark.parametrize("n,k,G,seed0,cap,fk", GAME_CASES)
def test_self_play_games_equal_the_restatement_ply_by_ply(n, k, G, seed0, cap, fk):
    """S = 32, set (c), four slots (refill happens at 5x5).  Under the playout cap (F = 8, 500 permille) the FAST plies search an
    un-noised root with fpu_root; with forced playouts (k = 4) pi comes from the counts pruned at c(count)."""
    S = 32
    games = ref_games(n, k, S, G, seed0, cap, fk)
    if fk:          # forcing decides most root selections at 5x5, and at 9x9 all 32 of a ply: there only the pruning at c(count) is the rule's
        assert n != 5 or (sum(g["root_diff"] for g in games) > 0 and all(g["below_diff"] > 0 for g in games))
    else:
        assert all(g["root_diff"] > 0 and g["below_diff"] > 0 for g in games)
    e = engine(n, k, S, 4)
    e.set_selection(**sel.SETS["c"])
    if cap:
        e.set_playout_cap(cap[0], cap[1] / 1000)
        full = np.concatenate([np_full(seed0 + i, np.arange(g["nply"]), cap[1]) for i, g in enumerate(games)])
        assert full.any() and not full.all()
    if fk:
        e.set_forced_playouts(fk, True)
    ep = episode(e, G, seed0)
    assert e.persistent() == 0
    assert_games(ep, games, f"{n}x{n} cap {cap} forced {fk}")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. properties
# ---------------------------------------------------------------------------------------------------------------------
def test_the_evaluation_cache_changes_nothing_and_leaf_symmetry_does():
    n, k, S, G, seed0 = 5, 4, 32, 6, 5500

    def run(cache, symmetry):
        e = engine(n, k, S, 4, real=True)
        e.set_selection(**sel.SETS["c"])
        e.set_eval_cache(1 << 12 if cache else 0)
        e.set_leaf_symmetry(symmetry)
        ep = episode(e, G, seed0)
        hits = ep["c"]["cache_hits"]
        e.close()
        return ep, hits
    (plain, _), (cached, hits), (sym, _) = run(False, False), run(True, False), run(False, True)
    assert hits > 0 and same_episode(plain, cached)
    assert not same_episode(plain, sym) and int(sym["nply"].sum()) > 0
    games = tuple(sel.selfplay_game(net5()[1], n, k, S, seed0 + g, sel.SETS["c"]) for g in range(G))
    assert_games(plain, games, "real net, six games")


def test_a_game_continued_from_ply_m_and_a_resigned_game():
    """start positions: game g restarted from its ply m with its own seed continues bit for bit; resignation: a resigned game is the
    same-seed game cut at its first crossing ply"""
    from tests.test_resign_gpu import choose_threshold, first_cross
    n, k, S, G, seed0, m = 5, 4, 32, 6, 5600, 3
    e = engine(n, k, S, 4)
    e.set_selection(**sel.SETS["c"])
    full = episode(e, G, seed0)
    offs = np.concatenate([[0], np.cumsum(full["nply"])[:-1]])
    assert (full["nply"] > m).all()
    rec = full["rec"]
    e.set_start_positions(rec["boards"][offs + m], rec["movers"][offs + m], rec["lasts"][offs + m])
    cont = episode(e, G, seed0)
    assert np.array_equal(cont["nply"], full["nply"] - m) and np.array_equal(cont["res"], full["res"])      # the plies played from there
    keep = np.concatenate([np.arange(o + m, o + L) for o, L in zip(offs, full["nply"])])
    for key in REC_KEYS:
        assert np.array_equal(cont["rec"][key], rec[key][keep]), key
    assert np.array_equal(cont["values"], full["values"][keep])
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
    keep = np.concatenate([np.arange(o, o + L) for o, L in zip(offs, res["nply"])])
    for key in ("boards", "actions", "pis", "visits"):
        assert np.array_equal(res["rec"][key], rec[key][keep]), key
    e.close()


@pytest.mark.parametrize("rule", ["freestyle", "exact"])
def test_the_win_rule(rule, monkeypatch):
    """tests/win_rule.py turns the restatement to the exact rule in one line"""
    from tests import win_rule
    n, k, S, G, seed0 = 5, 4, 32, 4, 5700
    win_rule.use_rule(monkeypatch, rule)
    games = tuple(sel.selfplay_game(synth(n, k), n, k, S, seed0 + g, sel.SETS["c"]) for g in range(G))
    e = engine(n, k, S, 4)
    e.set_win_rule(rule)
    e.set_selection(**sel.SETS["c"])
    assert_games(episode(e, G, seed0), games, f"win rule {rule}")
    e.close()


def test_behind_the_external_evaluator_seam():
    """the oracle's net behind az_set_external_evaluator (the evaluator with which tests/test_external_eval_gpu.py reproduces the
    native records): the same records as the native run under the same option, and the restatement's"""
    from tests.test_external_eval_gpu import CpuEvaluator, net_eval
    n, k, S, G, seed0 = 5, 4, 32, 4, 5800
    nat = engine(n, k, S, 4, real=True)
    nat.set_selection(**sel.SETS["c"])
    want = episode(nat, G, seed0)
    nat.close()
    e = az.Engine(n, k, S, 4, log_table=orc.numpy_log_table(S), c_puct=C_PUCT)
    CpuEvaluator(e, net_eval(orc.Net(n, net5()[0])))
    e.set_selection(**sel.SETS["c"])
    got = episode(e, G, seed0)
    assert same_episode(got, want)
    for key in ("plies", "simulations", "expansions", "root_evals", "terminal_hits", "depth_sum"):
        assert got["c"][key] == want["c"][key], key
    assert_games(got, tuple(sel.selfplay_game(net5()[1], n, k, S, seed0 + g, sel.SETS["c"]) for g in range(G)), "external evaluator")
    e.close()


def test_search_callback_with_a_host_evaluator():
    n, k, S = 5, 4, 32
    e = engine(n, k, S, 1)
    e.set_selection(**sel.SETS["c"])
    p = sel.positions(n, k)[1]
    ev = synth(n, k)
    r = e.search_callback(p["board"], p["player"], p["last"], p["T"], lambda cells, pl, la: ev(cells, pl, la), p["noise"], p["u"])
    assert_search(r, tree(n, k, S, 1, True, "c"), p, S, "c", "az_search_callback")
    e.close()


@pytest.mark.parametrize("n,k", [(5, 4), (9, 5)])
def test_a_captured_ply_graph_does_not_outlive_the_setting(n, k):
    """the same engine, the same games: on, off, on again with other parameters, on as at first"""
    e = engine(n, k, 16, 2)

    def run():
        c = e.selfplay(2, seed0=9, max_plies=6)
        return c["expansions"], e.records()["visits"].copy()
    e.set_selection(**sel.SETS["a"])
    a = run()
    e.set_selection(on=False)
    b = run()
    e.set_selection(**sel.SETS["b"])
    c = run()
    e.set_selection(**sel.SETS["a"])
    d = run()
    assert np.array_equal(a[1], d[1]) and a[0] == d[0]
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1]) and not np.array_equal(b[1], c[1])
    assert np.array_equal(b[1], np.concatenate([orc.Oracle(n, k, 16, c_puct=C_PUCT, synthetic=True).selfplay_game(
        None, *orc.selfplay_tape(9 + g, n, maxply=6), maxply=6)["visits"] for g in range(2)]))
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals and arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_pairs_in_both_orders():
    e = engine(5, 4, 16, 2, real=True)
    partners = ((lambda: e.set_subtree_reuse(True), lambda: e.set_subtree_reuse(False), "subtree reuse"),
                (lambda: e.set_solver(True), lambda: e.set_solver(False), "solver"),
                (lambda: e.set_gumbel(4, 50.0, 1.0), lambda: e.set_gumbel(0), "Gumbel"))
    for on, off, word in partners:
        e.set_selection(**sel.SETS["a"])
        with pytest.raises(az.AzError, match=INVALID) as ei:
            on()
        assert word in str(ei.value) and "selection rule" in str(ei.value)
        e.set_selection(on=False)                      # switching off is always allowed
        on()
        with pytest.raises(az.AzError, match=INVALID) as ei:
            e.set_selection(**sel.SETS["a"])
        assert word in str(ei.value) and not e.selection()["on"]
        e.set_selection(on=False)
        off()
    # the threat search stays refused without the solver, and the solver with the option
    e.set_selection(**sel.SETS["a"])
    with pytest.raises(az.AzError, match=INVALID):
        e.set_threat_search(4, 64)
    assert e.threat_search() == (0, 0) and e.selection()["on"]
    e.close()


def test_arguments_and_an_open_episode():
    L = _capi.lib()
    e = engine(5, 4, 16, 2)
    e.set_selection(**sel.SETS["c"])
    nan, inf = float("nan"), float("inf")
    for bad in ((1, -0.1, 0, 50, 1), (1, 2.1, 0, 50, 1), (1, nan, 0, 50, 1), (1, 0.2, -0.1, 50, 1), (1, 0.2, 2.5, 50, 1), (1, 0.2, inf, 50, 1),
                (1, 0.2, 0, 0.5, 1), (1, 0.2, 0, nan, 1), (1, 0.2, 0, inf, 1), (1, 0.2, 0, 50, -1), (1, 0.2, 0, 50, 16.5), (1, 0.2, 0, 50, nan),
                (2, 0.2, 0, 50, 1), (-1, 0.2, 0, 50, 1)):
        assert L.az_set_selection(e.h, *bad) == -1, bad
        assert e.selection() == dict(sel.SETS["c"], on=True)           # the previous setting is kept
    with pytest.raises(az.AzError, match=INVALID):
        e.set_selection(fpu=3.0)
    for good in ((1, 0.0, 0.0, 1.0, 0.0), (1, 2.0, 2.0, 1e9, 16.0)):
        assert L.az_set_selection(e.h, *good) == 0
    assert L.az_get_selection(e.h, None, None, None, None, None) == 0 and L.az_get_selection(None, None, None, None, None, None) == -1
    assert L.az_set_selection(e.h, 0, nan, -5.0, 0.0, 99.0) == 0 and not e.selection()["on"]      # off: the rest is ignored
    e.set_selection(**sel.SETS["a"])
    e.selfplay_begin(2, seed0=1)
    with pytest.raises(az.AzError, match=STATE):
        e.set_selection(**sel.SETS["c"])
    with pytest.raises(az.AzError, match=STATE):
        e.set_selection(on=False)
    e.selfplay_step(1 << 20)
    e.selfplay_end()
    assert e.selection() == dict(sel.SETS["a"], on=True)
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. the seams
# ---------------------------------------------------------------------------------------------------------------------
def _controller():
    from tests.test_external_eval_gpu import _controller as fixture_controller
    return fixture_controller("ckpt_saved")


def test_mcts_run_and_run_many():
    from alphazero_piskvorky_amd import constants as consts
    from alphazero_piskvorky_amd.controller import make_policy_value_fn
    from alphazero_piskvorky_amd.games import Gomoku
    from alphazero_piskvorky_amd.mcts import MCTS
    n, k, S = 5, 4, 32
    ctrl = _controller()
    states = []
    for p in sel.positions(n, k):
        g = Gomoku(n, k)
        g.cells = p["board"].reshape(n, n).copy()
        g.current_player = consts.X if p["player"] == 1 else consts.O
        g.last_action = None if p["last"] < 0 else (p["last"] // n, p["last"] % n)
        states.append(g)
    e = engine(n, k, S, 1, real=True)
    e.set_selection(**sel.SETS["c"])

    def engine_level(seed, noised):
        np.random.seed(seed)
        out = []
        for g, p in zip(states, sel.positions(n, k)):
            noise = np.random.dirichlet([0.3] * int((p["board"] == 0).sum())) if noised else None
            u = np.random.random_sample()
            out.append(e.search(p["board"], p["player"], p["last"], 1.0, noise, u))
        return out
    m = MCTS(make_policy_value_fn(ctrl), S, C_PUCT, selection=dict(sel.SETS["c"]))
    plain = MCTS(make_policy_value_fn(ctrl), S, C_PUCT)
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
    assert m._engine.selection() == dict(sel.SETS["c"], on=True) and m._batch_engine.selection()["on"]
    assert not plain._engine.selection()["on"]
    e.close()


def test_self_play_manager_and_a_cached_engine_brought_back_to_off():
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    n, k, S, G, seed0 = 5, 4, 32, 4, 5900
    ctrl = _controller()
    e = engine(n, k, S, 4, real=True)
    e.set_selection(**sel.SETS["c"])
    e.selfplay(G, seed0=seed0)
    want_on = e.records()
    e.set_selection(on=False)
    e.selfplay(G, seed0=seed0)
    want_off = e.records()
    e.close()
    m = SelfPlayManager(ctrl, "cuda:0", mcts_params={"num_simulations": S, "c_puct": C_PUCT}, concurrent_games=4, seed=seed0,
                        selection=dict(sel.SETS["c"]))
    _, total, eng, _, _ = m.generate_packed(G)
    assert eng.selection() == dict(sel.SETS["c"], on=True) and eng.persistent() == 0
    got = eng.records()
    for key in REC_KEYS:
        assert np.array_equal(got[key], want_on[key]), key
    assert total == len(want_on["actions"])
    m.selection = None                                  # the cached engine that played with the option goes back to off
    _, _, eng2, _, _ = m.generate_packed(G)
    assert eng2 is eng and not eng.selection()["on"] and eng.persistent() > 0
    got = eng.records()
    for key in REC_KEYS:
        assert np.array_equal(got[key], want_off[key]), key
    assert not np.array_equal(want_on["visits"][0], want_off["visits"][0]) or len(want_on["actions"]) != len(want_off["actions"])
    m.selection = dict(sel.SETS["a"])
    m.solver = False
    m.subtree_reuse = True
    with pytest.raises(ValueError, match="subtree_reuse"):
        m.generate_packed(G)


def test_model_evaluator_arena(monkeypatch):
    from alphazero_piskvorky_amd import constants as consts
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator, temperature_schedule
    n, k, G, seed0, S = 5, 4, 4, 6000, 32
    ctrl = _controller()
    e = az.Engine(n, k, S, G, c_puct=consts.EVAL_EXPLORATION_CONSTANT, log_table=orc.numpy_log_table(S), deep=S > _capi.AZ_MAX_SIMULATIONS)
    e.load_weights(net5()[0], 0)
    e.load_weights(net5()[0], 1)
    T = np.array([float(temperature_schedule(m)) for m in range(n * n + 2)], dtype=np.float64)
    e.set_selection(**sel.SETS["c"])
    want = e.arena(G, seed0=seed0, temperature_table=T)
    want_rec = e.records()
    e.set_selection(on=False)
    off_rec = (e.arena(G, seed0=seed0, temperature_table=T), e.records())[1]
    e.close()
    monkeypatch.setattr(consts, "NUM_EVAL_SIMULATIONS", S)
    ev = ModelEvaluator(device="cuda:0", seed=seed0, selection=dict(sel.SETS["c"]))
    rate, metrics = ev.evaluate(ctrl, ctrl, num_games=G)
    assert (metrics["wins"], metrics["losses"], metrics["draws"]) == (want["wins"], want["losses"], want["draws"])
    got = ev._engine.records()
    for key in ("actions", "visits", "pis"):
        assert np.array_equal(got[key], want_rec[key]), key
    assert ev._engine.selection() == dict(sel.SETS["c"], on=True)
    assert got["visits"].shape != off_rec["visits"].shape or not np.array_equal(got["visits"], off_rec["visits"])
    ev.selection = None
    ev.evaluate(ctrl, ctrl, num_games=G)
    assert not ev._engine.selection()["on"]
    got = ev._engine.records()
    for key in ("actions", "visits", "pis"):
        assert np.array_equal(got[key], off_rec[key]), key
