"""az_set_forced_playouts on the GPU, against the numpy restatement in tests/forced.py (which with the rule off is the oracle's
search, tests/test_forced_playouts_cpu.py).  Every comparison is exact: integer equality for visits and actions, == on the
float64 W, == on the float32 priors and pi.  pi and the action are the helper's restatement of mcts.py:144-177 applied to the
counts az_forced_prune returns for the engine's own visits, W and priors, and az_forced_prune in turn equals the rule's
definition on the CPU.

The positions are chosen on the CPU with the helper alone (test_the_cases_are_not_vacuous states what they show): at
S = 64, k = 2 all nine single-search positions give other raw visits than k = 0, every one has children with N' < N (13 to 38
of them, 14 to 41 visits), and 16 children in all are emptied by the single-playout step of the rule (13 of them at 5x5).
The six self-play games prune visits on 71 of 71 plies at 5x5 and on 242 of 244 at 9x9; under the playout cap on 38 of 76 and
116 of 237, all of them FULL plies."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import forced
from tests.test_playout_cap_cpu import np_full
from tests.util import ROOT, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

C_PUCT = 2.0
SIZES = ((5, 4), (9, 5), (15, 5))
S1 = 64
REC_KEYS = ("boards", "movers", "lasts", "actions", "pis", "visits", "z")


# ---------------------------------------------------------------------------------------------------------------------
# positions and references (computed once, never modified)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def positions(n, k):
    """the empty board and two mid-game positions, each with its Dirichlet sample, uniform and temperature"""
    out = []
    for i, (stones, seed) in enumerate(((0, 1), (6, 2), (11, 3))):
        board, player, last = forced.random_position(n, k, stones, seed)
        rs = np.random.RandomState(1000 * n + i)
        noise = rs.dirichlet([0.3] * int((board == 0).sum()))
        out.append(dict(board=board, player=player, last=last, noise=noise, u=float(rs.random_sample()), T=(1.0, 0.5, 1e-9)[i]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def synth(n, k):
    return orc.Oracle(n, k, 1, synthetic=True).synth_eval


@functools.lru_cache(maxsize=None)
def net5():
    """(state dict for the engine, evaluate(board, player, last) through the oracle's net) of the 5x5 fixture"""
    sd = weights_from_fixture(5, "ckpt_saved")
    net, o = orc.Net(5, sd), orc.Oracle(5, 4, 1)

    def evaluate(board, player, last):
        _, P, v = net.eval(o.encode(board, player, last))
        return P, v
    return sd, evaluate


@functools.lru_cache(maxsize=None)
def tree(n, k, S, i, fk, L=1, real=False):
    p = positions(n, k)[i]
    ev = net5()[1] if real else synth(n, k)
    return forced.search(ev, n, k, S, p["board"], p["player"], p["last"], p["noise"], fk, C_PUCT, L=L)


def engine(n, k, S, slots, real=False, **kw):
    e = az.Engine(n, k, S, slots, synthetic=not real, log_table=orc.numpy_log_table(S), c_puct=C_PUCT, **kw)
    if real:
        e.load_weights(net5()[0], 0)
    return e


def expect_pi(r, p, S, fk, prune):
    """pi and action the rule asks for, from the ENGINE's root statistics: az_forced_prune's counts when pruning applies"""
    legal = np.flatnonzero(p["board"] == 0)
    counts = r["N"][legal]
    if fk > 0 and prune:
        counts, removed = _capi.forced_prune(fk, C_PUCT, counts, r["W"][legal], r["P"][legal])
        assert removed == int(r["N"].sum() - counts.sum())
    return forced.pi_action(counts, p["board"], p["T"], p["u"], orc.numpy_log_table(S))


def assert_search(r, want, p, S, fk, prune, what):
    assert np.array_equal(r["N"], want["N"]), f"{what}: visits"
    assert np.array_equal(r["W"], want["W"]), f"{what}: W"
    assert np.array_equal(r["P"], want["P"]), f"{what}: priors"
    pi, a = expect_pi(r, p, S, fk, prune)
    assert r["pi"].dtype == np.float32 and np.array_equal(r["pi"], pi), f"{what}: pi"
    assert int(r["action"]) == a, f"{what}: action"


def batch(e, ps):
    rb = e.search_batch(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps],
                        np.array([p["T"] for p in ps]), [p["noise"] for p in ps], [p["u"] for p in ps])
    return [{key: val[i] for key, val in rb.items()} for i in range(len(ps))]


# ---------------------------------------------------------------------------------------------------------------------
# 1. guard: with the option off the restatement of pi and the action is the engine's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", SIZES)
def test_guard_pi_and_action_restated_from_the_raw_visits(n, k):
    """Holds exactly (largest deviation 0.0 on every position), so the pruned runs below are compared with == as well."""
    e = engine(n, k, S1, 4)
    assert e.forced_playouts() == dict(k=0.0, prune=False)
    ps = positions(n, k)
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, tree(n, k, S1, i, 0.0), p, S1, 0.0, False, f"{n}x{n} position {i} {what}, option off")
    e.close()


def test_guard_self_play_records_restated_from_the_raw_visits():
    n, k, S, G, seed0 = 5, 4, 32, 6, 4100
    e = engine(n, k, S, 4)
    e.selfplay(G, seed0=seed0)
    rec, (nply, _) = e.records(), e.games()
    T, lt, r = orc.selfplay_T_table(n * n), orc.numpy_log_table(S), 0
    for g in range(G):
        _, us = orc.selfplay_tape(seed0 + g, n)
        for m in range(nply[g]):
            board = rec["boards"][r]
            pi, a = forced.pi_action(rec["visits"][r][board == 0], board, T[m], us[m], lt)
            assert np.array_equal(rec["pis"][r], pi) and rec["actions"][r] == a, (g, m)
            r += 1
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. single searches with noise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prune", [True, False], ids=["prune", "no-prune"])
@pytest.mark.parametrize("n,k", SIZES)
def test_single_searches_equal_the_helper(n, k, prune):
    """5x5: one cell per lane and the persistent kernel (az_search one game per workgroup, az_search_batch two); 9x9: two cells
    per lane; 15x15: four.  k = 2, S = 64."""
    e = engine(n, k, S1, 4)
    e.set_forced_playouts(2.0, prune)
    assert e.forced_playouts() == dict(k=2.0, prune=prune)
    ps = positions(n, k)
    rbs = batch(e, ps)
    assert (e.persistent() > 0) == (n == 5)
    for i, (p, rb) in enumerate(zip(ps, rbs)):
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        assert (e.persistent() > 0) == (n == 5)
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, tree(n, k, S1, i, 2.0), p, S1, 2.0, prune, f"{n}x{n} position {i} {what}")
        if prune and p["T"] > 0.1:               # (at T -> 0 pi is the one-hot of the most visited child either way)
            legal = p["board"] == 0
            assert not np.array_equal(r["pi"], forced.pi_action(r["N"][legal], p["board"], p["T"], p["u"], orc.numpy_log_table(S1))[0])
    e.close()


@pytest.mark.parametrize("cache", [False, True], ids=["plain", "eval-cache"])
def test_real_net_5x5(cache):
    """the trained 5x5 net through the oracle's Net.eval; with the evaluation cache the persistent kernel runs its other
    instantiation (tile subsets) and the searches after the first hit the cache"""
    n, k = 5, 4
    e = engine(n, k, S1, 4, real=True)
    e.set_forced_playouts(2.0, True)
    ps = positions(n, k)
    if cache:
        e.set_eval_cache(1 << 10)
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, tree(n, k, S1, i, 2.0, real=True), p, S1, 2.0, True, f"real net, position {i} {what}")
    e.close()


def test_external_evaluator_callback():
    """az_search_callback with noise: the host evaluator's priors as given, the rule on top"""
    n, k, S = 5, 4, 32
    e = engine(n, k, S, 1)
    e.set_forced_playouts(2.0, True)
    p = positions(n, k)[1]
    ev = synth(n, k)
    r = e.search_callback(p["board"], p["player"], p["last"], p["T"], lambda cells, pl, la: ev(cells, pl, la), p["noise"], p["u"])
    want = forced.search(ev, n, k, S, p["board"], p["player"], p["last"], p["noise"], 2.0, C_PUCT)
    assert_search(r, want, p, S, 2.0, True, "az_search_callback")
    off = e.search_callback(p["board"], p["player"], p["last"], p["T"], lambda cells, pl, la: ev(cells, pl, la), None, p["u"])
    want = forced.search(ev, n, k, S, p["board"], p["player"], p["last"], None, 0.0, C_PUCT)
    assert_search(off, want, p, S, 0.0, False, "az_search_callback without noise")
    e.close()


def test_batched_external_evaluator_self_play():
    """az_set_external_evaluator: six 5x5 games whose leaves are evaluated outside the engine, by the oracle's net behind a
    BatchPolicyValueFn (exact answers), against the helper with the same net"""
    import torch
    from alphazero_piskvorky_amd.controller import BatchPolicyValueFn
    n, k, S, seed0 = 5, 4, 32, 4600
    onet = orc.Net(n, net5()[0])

    def fn(planes, net):
        pl = planes.cpu().numpy()
        out = [onet.eval(pl[j]) for j in range(len(pl))]
        return torch.from_numpy(np.stack([o[1] for o in out])), torch.tensor([o[2] for o in out], dtype=torch.float32)
    e = az.Engine(n, k, S, 4, log_table=orc.numpy_log_table(S), c_puct=C_PUCT)
    BatchPolicyValueFn(fn, "cuda:0").attach(e)
    e.set_forced_playouts(FK, True)
    ep = episode(e, seed0)
    games = tuple(forced.selfplay_game(net5()[1], n, k, S, seed0 + g, FK, True) for g in range(GAMES))
    assert sum(int((g["pruned"] > 0).sum()) for g in games) > 0
    assert_games(ep, games, "external evaluator")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the cases above show something
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_not_vacuous():
    emptied = 0
    for n, k in SIZES:
        fired = pruned = 0
        for i, p in enumerate(positions(n, k)):
            on, off = tree(n, k, S1, i, 2.0), tree(n, k, S1, i, 0.0)
            assert on["N"].sum() == off["N"].sum() == S1
            fired += not np.array_equal(on["N"], off["N"])
            legal = np.flatnonzero(p["board"] == 0)
            info = {}
            Np = forced.prune(2.0, C_PUCT, on["N"][legal], on["W"][legal], on["P"][legal], info)
            pruned += int((Np < on["N"][legal]).any())
            emptied += info["single"]
        assert fired >= 1 and pruned >= 1, (n, fired, pruned)
    assert emptied >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 4. no noise, no rule
# ---------------------------------------------------------------------------------------------------------------------
def test_searches_without_noise_the_arena_and_fast_plies_are_untouched():
    n, k, S = 5, 4, 32
    p = positions(n, k)[1]

    def run(fk):
        e = engine(n, k, S, 4)
        if fk:
            e.set_forced_playouts(fk, True)
        s = e.search(p["board"], p["player"], p["last"], p["T"], None, p["u"])
        sb = e.search_batch(p["board"][None], [p["player"]], [p["last"]], p["T"], None, [p["u"]])
        ar = e.arena(4, seed0=77, temperature_table=orc.arena_T_table(n * n))
        ar_rec = e.records()
        e.set_playout_cap(8, 0.0)                  # every ply FAST: no noise anywhere
        e.selfplay(4, seed0=4200)
        fast = dict(e.records(), values=e.values(), nply=e.games()[0])
        e.close()
        return s, sb, ar, ar_rec, fast
    a, b = run(0.0), run(2.0)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key in x:
            assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), key


# ---------------------------------------------------------------------------------------------------------------------
# 5. whole self-play games
# ---------------------------------------------------------------------------------------------------------------------
GAMES = 6
FK = 4.0


@functools.lru_cache(maxsize=None)
def ref_games(n, k, S, seed0, cap=None):
    return tuple(forced.selfplay_game(synth(n, k), n, k, S, seed0 + g, FK, True, cap, lambda s, m, pm: np_full(s, m, pm))
                 for g in range(GAMES))


def episode(e, seed0):
    c = e.selfplay(GAMES, seed0=seed0)
    nply, res = e.games()
    return dict(rec=e.records(), nply=nply, res=res, values=e.values(), c=c)


def assert_games(ep, games, what):
    assert ep["nply"].tolist() == [g["nply"] for g in games], f"{what}: plies per game"
    assert ep["res"].tolist() == [g["result"] for g in games], f"{what}: results"
    for key in REC_KEYS:
        exp = np.concatenate([g[key] for g in games])
        assert ep["rec"][key].shape == exp.shape and np.array_equal(ep["rec"][key], exp), f"{what}: {key}"
    assert np.array_equal(ep["values"], np.concatenate([g["values"] for g in games])), f"{what}: values"


GAME_CASES = [pytest.param(5, 4, 4300, None, id="5x5"), pytest.param(9, 5, 4400, None, id="9x9"),
              pytest.param(5, 4, 4300, (8, 500), id="5x5-cap"), pytest.param(9, 5, 4400, (8, 500), id="9x9-cap")]


@pytest.mark.parametrize("n,k,seed0,cap", GAME_CASES)
def test_self_play_games_equal_the_helper_ply_by_ply(n, k, seed0, cap):
    """k = 4, S = 32, six games on four slots (refill happens), the engine's own tapes = oracle.selfplay_tape.  With the playout
    cap (F = 8, 500 permille) the FULL plies only get the rule."""
    S = 32
    games = ref_games(n, k, S, seed0, cap)
    assert sum(int((g["pruned"] > 0).sum()) for g in games) > 0
    e = engine(n, k, S, 4)
    e.set_forced_playouts(FK, True)
    if cap:
        e.set_playout_cap(cap[0], cap[1] / 1000)
        full = np.concatenate([np_full(seed0 + i, np.arange(g["nply"]), cap[1]) for i, g in enumerate(games)])
        assert full.any() and not full.all()
        assert not np.concatenate([g["pruned"] for g in games])[~full].any()
    ep = episode(e, seed0)
    assert (e.persistent() > 0) == (n == 5 and not cap)
    assert_games(ep, games, f"{n}x{n} cap {cap}")
    e.close()


@pytest.mark.parametrize("trunk", ["f32", "bf16x3"])
def test_options_the_helper_cannot_restate_do_not_depend_on_slots_and_lanes(trunk):
    """Leaf symmetry (its hash names game and ply, which a single restated search cannot) and an emulated trunk (not bit-exact
    by design), together with the real net, start positions, resignation and max_plies: the episode is the same on 6 slots
    in 2 lanes and on 4 slots in 1 lane, and it is not the episode with the option off."""
    n, k, S, G, seed0 = 5, 4, 32, 8, 4500
    ps = positions(n, k)[1:]

    def run(slots, lanes, fk):
        e = engine(n, k, S, slots, real=True, engines=lanes)
        e.set_leaf_symmetry(True)
        e.set_trunk_mode(trunk)
        e.set_resign(0.9, 2, 0.25)
        e.set_start_positions(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps])
        if fk:
            e.set_forced_playouts(fk, True)
        e.selfplay(G, seed0=seed0, max_plies=18)
        nply, res = e.games()
        out = dict(e.records(), values=e.values(), nply=nply, res=res)
        e.close()
        return out
    a, b, off = run(6, 2, 2.0), run(4, 1, 2.0), run(4, 1, 0.0)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert len(set(a["nply"].tolist())) > 1 and a["visits"].tobytes() != off["visits"].tobytes()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import test_forced_playouts_gpu as t
e = t.engine(5, 4, 32, 4)
e.set_forced_playouts(t.FK, True)
ep = t.episode(e, 4300)
assert e.persistent() == 0
e.close()
np.savez(sys.argv[2], nply=ep["nply"], res=ep["res"], values=ep["values"], **ep["rec"])
"""


def test_self_play_games_on_the_lock_step_path_in_a_fresh_process(tmp_path):
    """AZ_PERSIST=0: the 5x5 games through k_step instead of the persistent kernel"""
    path = str(tmp_path / "child.npz")
    env = {key: v for key, v in os.environ.items() if key not in ("AZ_COMPACT", "AZ_GRAPH", "AZ_PROFILE_EVENTS")}
    env["AZ_PERSIST"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(path)
    ep = dict(rec={key: z[key] for key in REC_KEYS}, nply=z["nply"], res=z["res"], values=z["values"])
    assert_games(ep, ref_games(5, 4, 32, 4300), "AZ_PERSIST=0")


# ---------------------------------------------------------------------------------------------------------------------
# 6. virtual-loss batching, 7. deep engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [128, 126])
def test_virtual_loss_batches_of_four(S):
    """9x9, L = 4: n = N + in-flight, total = simulations done + the item's index in its batch, duplicates back up the value of
    the item they repeat.  S = 126 ends on a batch of two.  (At S = 64 the batches change nothing on these positions: nearly
    every selection at the root is a forced one.)"""
    n, k = 9, 5
    e = engine(n, k, S, 4)
    e.set_virtual_loss(4)
    e.set_forced_playouts(2.0, True)
    ps = positions(n, k)
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        want = tree(n, k, S, i, 2.0, L=4)
        seq = tree(n, k, S, i, 2.0)
        assert not (np.array_equal(want["N"], seq["N"]) and np.array_equal(want["W"], seq["W"])), "the batches change nothing"
        assert not np.array_equal(want["N"], tree(n, k, S, i, 0.0, L=4)["N"]), "forcing changes nothing"
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, want, p, S, 2.0, True, f"virtual loss, S = {S}, position {i} {what}")
    e.close()


def test_deep_engine_1100_simulations():
    """16-bit counts: n * n of a child with more than 181 visits no longer fits a 16-bit product, nor 46341 a 32-bit one"""
    n, k, S = 5, 4, 1100
    p = positions(n, k)[1]
    want = forced.search(synth(n, k), n, k, S, p["board"], p["player"], p["last"], p["noise"], 2.0, C_PUCT)
    assert want["N"].max() > 256 and not np.array_equal(want["N"], forced.search(synth(n, k), n, k, S, p["board"], p["player"], p["last"],
                                                                                   p["noise"], 0.0, C_PUCT)["N"])
    e = engine(n, k, S, 1, deep=True)
    e.set_forced_playouts(2.0, True)
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    assert e.persistent() == 0
    assert_search(r, want, p, S, 2.0, True, "deep")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the setters
# ---------------------------------------------------------------------------------------------------------------------
def test_setters():
    L = _capi.lib()
    e = engine(5, 4, 16, 2)
    assert e.forced_playouts() == dict(k=0.0, prune=False)
    e.set_forced_playouts(2.0)
    assert e.forced_playouts() == dict(k=2.0, prune=True)
    for bad in ((-1.0, 1), (16.5, 1), (float("nan"), 1), (float("inf"), 0), (2.0, 2), (2.0, -1)):
        assert L.az_set_forced_playouts(e.h, *bad) == -1, bad
        assert e.forced_playouts() == dict(k=2.0, prune=True)
    with pytest.raises(az.AzError, match=r"\(-1\)"):
        e.set_forced_playouts(17.0)
    e.set_forced_playouts(16.0, False)
    assert e.forced_playouts() == dict(k=16.0, prune=False)
    assert L.az_get_forced_playouts(e.h, None, None) == 0
    # refused with subtree reuse, whichever comes first
    with pytest.raises(az.AzError, match=r"\(-1\)"):
        e.set_subtree_reuse(True)
    assert L.az_set_forced_playouts(e.h, 0.0, 7) == 0 and e.forced_playouts() == dict(k=0.0, prune=False)     # off: the rest is ignored
    e.set_subtree_reuse(True)
    with pytest.raises(az.AzError, match=r"\(-1\)"):
        e.set_forced_playouts(2.0)
    assert e.forced_playouts()["k"] == 0.0
    e.set_forced_playouts(0.0)                   # switching off is always allowed
    e.set_subtree_reuse(False)
    e.set_forced_playouts(2.0)
    # an open episode
    e.selfplay_begin(2, seed0=1)
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.set_forced_playouts(4.0)
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.set_forced_playouts(0.0)
    e.selfplay_step(1 << 20)
    e.selfplay_end()
    assert e.forced_playouts() == dict(k=2.0, prune=True)
    e.close()


@pytest.mark.parametrize("n,k", [(5, 4), (9, 5)], ids=["persistent", "lock-step"])
def test_a_captured_ply_graph_does_not_outlive_the_setting(n, k):
    """the same engine, the same games: on, off, on again.  Both paths replay a captured graph of the ply."""
    e = engine(n, k, 16, 2)

    def run():
        c = e.selfplay(2, seed0=9, max_plies=6)
        return c["expansions"], e.records()["visits"].copy()
    e.set_forced_playouts(2.0)
    a = run()
    e.set_forced_playouts(0.0)
    b = run()
    e.set_forced_playouts(2.0)
    c = run()
    assert (e.persistent() > 0) == (n == 5)
    assert np.array_equal(a[1], c[1]) and a[0] == c[0] and not np.array_equal(a[1], b[1])
    assert np.array_equal(b[1], np.concatenate([orc.Oracle(n, k, 16, synthetic=True).selfplay_game(None, *orc.selfplay_tape(9 + g, n, maxply=6),
                                                                                                    maxply=6)["visits"] for g in range(2)]))
    e.close()
