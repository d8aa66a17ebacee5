"""az_set_external_evaluator on the GPU: self-play, the arena and batched search with the evaluator outside the engine.

The evaluators of these tests run on the CPU on purpose: the oracle's own net (orc.Net.eval) applied to the planes the engine
hands out, or the oracle's synthetic evaluator on the cells decoded from those planes.  With them the expected result is
exact: every record, game and tree counter must equal the oracle's bit for bit (np.array_equal, no tolerances), and where
the oracle has no such notion (search values, resignation) the same engine with the same weights loaded natively.
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_all_sizes_gpu import SIZES
from tests.test_options_all_sizes_gpu import _assert_games, _assert_work, _oracle_games, _totals
from tests.test_resign_gpu import choose_threshold
from tests.test_search_batch_gpu import _assert_equal, _batch, _draws, _fixture_positions, _oracle_searches, _positions
from tests.util import weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import games as az_games
from alphazero_piskvorky_amd import net as az_net
from alphazero_piskvorky_amd.controller import BatchPolicyValueFn, NeuralNetworkController, make_batch_policy_value_fn
from alphazero_piskvorky_amd.evaluator import ModelEvaluator
from alphazero_piskvorky_amd.mcts import MCTS
from alphazero_piskvorky_amd.net import fold_resnet_state_dict
from alphazero_piskvorky_amd.self_play import SelfPlayManager
from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict, synthetic_state_dict

ALL_SIZES = sorted(SIZES + [(5, 4), (9, 5), (15, 5)])        # n = 3 .. 15
DEV = "cuda:0"
_POOL = ThreadPoolExecutor(max_workers=16)                   # the oracle's scratch is per thread: one net serves many


class CpuEvaluator:
    """The test's evaluator behind Engine.set_external_evaluator: owns the three device buffers, reads the planes back,
    evaluates every item on the CPU with evalfn(planes [4, n, n], net) -> (P [n*n], v) and uploads the answers.  Keeps what
    the lifecycle tests look at: the thread of every call, (net, count) of every request, the planes of the first one."""

    def __init__(self, e, evalfn, capacity=None, pool=True):
        self.n, self.nn, self.evalfn, self.pool = e.n, e.nn, evalfn, pool
        cap = e.ext_capacity() if capacity is None else capacity
        self.planes = torch.full((cap, 4, e.n, e.n), 7.0, dtype=torch.float32, device=DEV)      # 7: a float the engine never writes
        self.policy = torch.zeros((cap, e.nn), dtype=torch.float32, device=DEV)
        self.value = torch.zeros(cap, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        self.threads, self.requests, self.first_planes = [], [], None
        self.fail_after = None                # raise in the request with this index
        e.set_external_evaluator(self.planes.data_ptr(), self.policy.data_ptr(), self.value.data_ptr(), cap, self)

    def __call__(self, net, count):
        self.threads.append(threading.get_ident())
        self.requests.append((net, count))
        if self.fail_after is not None and len(self.requests) > self.fail_after:
            raise KeyError("the evaluator gave up")
        host = self.planes.cpu().numpy()
        assert (host[count:] == 7.0).all(), "the engine wrote behind the last item of the request"
        pl = host[:count]
        assert np.isin(pl, (0.0, 1.0)).all() and (pl[:, 3] == 0.0).all(), "every float of every handed-out plane is written"
        if self.first_planes is None:
            self.first_planes = pl.copy()
        self.planes.fill_(7.0)                # the next request is checked against a clean buffer again
        out = list(_POOL.map(lambda j: self.evalfn(pl[j], net), range(count))) if self.pool else [self.evalfn(pl[j], net) for j in range(count)]
        P = np.stack([np.asarray(o[0], np.float32).reshape(self.nn) for o in out])
        v = np.array([o[1] for o in out], np.float32)
        self.policy[:count].copy_(torch.from_numpy(P))
        self.value[:count].copy_(torch.from_numpy(v))
        torch.cuda.synchronize()


def net_eval(onet):
    """the oracle's own net on the planes the engine hands out -> its P and v"""
    def f(planes, net):
        _, P, v = onet.eval(planes)
        return P, v
    return f


def nets_eval(onets):
    """the arena's: the oracle net named by the request's net id"""
    def f(planes, net):
        _, P, v = onets[net].eval(planes)
        return P, v
    return f


def synth_eval(n):
    """the oracle's synthetic evaluator on the cells decoded from planes 0 / 1 with player 1 and last from plane 2 (its hash
    is mover-relative)"""
    o = orc.Oracle(n, min(n, 3), 1)

    def f(planes, net):
        cells = (planes[0] + 2 * planes[1]).astype(np.uint8).reshape(-1)
        last = int(planes[2].argmax()) if planes[2].any() else -1
        return o.synth_eval(cells, 1, last)
    return f


def _engine(n, k, S, slots, **kw):
    return az.Engine(n, k, S, slots, log_table=orc.numpy_log_table(S), **kw)


def _play_vs_oracle(e, ev, o, onet, n, G, seed0, cut, what):
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    gs = _oracle_games(o, onet, n, G, seed0, cut=cut)
    _assert_games(e, gs, what, cut=cut)
    tot = _totals(gs)
    _assert_work(c, tot, what)
    st = e.ext_stats()
    assert st["items"] == c["expansions"] + c["root_evals"] == sum(cnt for _, cnt in ev.requests), f"{what}: every evaluation is handed out exactly once"
    assert st["requests"] == len(ev.requests)
    assert (c["trunk_launches"], c["trunk_boards"], c["nn_seconds"], c["trunk_seconds"]) == (0, 0, 0.0, 0.0)
    assert e.persistent() == 0
    return c, gs


# ---------------------------------------------------------------------------------------------------------------------
# 1. every board size, the synthetic evaluator through the seam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", ALL_SIZES)
def test_all_sizes_synthetic_through_the_seam(n, k):
    S, G, slots = 24, 5, 3                       # 5 complete games on 3 slots: refills happen
    e = _engine(n, k, S, slots)                  # a net engine without weights: none are needed
    ev = CpuEvaluator(e, synth_eval(n), pool=False)
    assert e.external_evaluator() and e.ext_capacity() == slots
    _play_vs_oracle(e, ev, orc.Oracle(n, k, S, synthetic=True), None, n, G, 100 + n, 0, f"{n}x{n} synthetic")
    assert all(net == 0 and 1 <= cnt <= slots for net, cnt in ev.requests)
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the oracle's net through the seam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,S,G,slots,cut,tag,kw", [
    (5, 4, 32, 6, 4, 0, "ckpt_saved", {}),
    (9, 5, 16, 4, 3, 6, "seeded", dict(engines=2)),
    (8, 5, 12, 3, 3, 4, "synthetic", {}),
    (15, 5, 8, 3, 2, 3, "seeded", {}),
])
def test_oracle_net_through_the_seam(n, k, S, G, slots, cut, tag, kw):
    sd = synthetic_state_dict(n) if tag == "synthetic" else weights_from_fixture(n, tag)
    onet = orc.Net(n, sd)
    e = _engine(n, k, S, slots, **kw)
    ev = CpuEvaluator(e, net_eval(onet))
    _play_vs_oracle(e, ev, orc.Oracle(n, k, S), onet, n, G, 7, cut, f"{n}x{n} {tag}")
    assert len(set(ev.threads)) == 1 and ev.threads[0] == threading.get_ident()
    e.close()


def test_the_engines_own_model_does_not_matter():
    """the evaluator is the oracle's ResidualBlock net, the engine was created for the plain model"""
    n, k, S, G = 5, 4, 24, 4
    onet = orc.Net(n, resnet_tensors=fold_resnet_state_dict(synthetic_resnet_state_dict(n)))
    e = _engine(n, k, S, 3, model="plain")
    ev = CpuEvaluator(e, net_eval(onet))
    _play_vs_oracle(e, ev, orc.Oracle(n, k, S), onet, n, G, 21, 0, "resnet evaluator on a plain engine")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. virtual-loss batching: L leaves per game and request
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,S,L,G,slots,tag", [
    (5, 4, 48, 4, 4, 4, "ckpt_saved"),
    (5, 4, 48, 32, 4, 3, "ckpt_saved"),          # late plies have fewer legal cells than L: duplicates are forced
    (9, 5, 40, 8, 3, 2, None),
])
def test_virtual_loss_through_the_seam(n, k, S, L, G, slots, tag):
    onet = orc.Net(n, weights_from_fixture(n, tag)) if tag else None
    e = _engine(n, k, S, slots)
    e.set_virtual_loss(L)
    assert e.ext_capacity() == slots * L
    ev = CpuEvaluator(e, net_eval(onet) if tag else synth_eval(n))
    o = orc.Oracle(n, k, S, synthetic=tag is None, virtual_loss=L)
    c, gs = _play_vs_oracle(e, ev, o, onet, n, G, 55, 0, f"{n}x{n} L = {L}")
    tot = _totals(gs)
    assert c["duplicate_leaves"] == tot["dup_sims"]
    if L == 32:
        assert tot["dup_sims"] > 0
    # one lane: az_counters.steps = lock-step plies x (1 + ceil(S / L)) evaluation steps, each at most one request
    nb = 1 + -(-S // L)
    assert e.lanes() == 1 and c["steps"] % nb == 0
    plies_steps = c["steps"] // nb
    assert e.ext_stats()["requests"] <= plies_steps * nb
    assert max(cnt for _, cnt in ev.requests) <= slots * L
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. arena: two nets, at most two homogeneous requests per step
# ---------------------------------------------------------------------------------------------------------------------
def test_arena_through_the_seam():
    n, k, S, G, seed0 = 5, 4, 16, 6, 900
    cand, base = weights_from_fixture(n, "ckpt_saved"), weights_from_fixture(n, "ckpt_0802")
    oc, ob = orc.Net(n, cand), orc.Net(n, base)
    e = _engine(n, k, S, 4)
    ev = CpuEvaluator(e, nets_eval((oc, ob)))
    r = e.arena(G, seed0=seed0, temperature_table=orc.arena_T_table(n * n))
    o = orc.Oracle(n, k, S)
    w = l = d = 0
    for g in range(G):
        ro = o.arena_game(oc, ob, g, np.random.RandomState(seed0 + g).random_sample(n * n))
        assert int(r["nply"][g]) == ro["nply"] and int(r["results"][g]) == ro["result"], f"game {g}"
        assert np.array_equal(r["actions"][g][:ro["nply"]], ro["actions"]), f"game {g}: actions"
        w += ro["result"] == 1; l += ro["result"] == 2; d += ro["result"] == 3
    assert (r["wins"], r["losses"], r["draws"]) == (w, l, d)
    assert {net for net, _ in ev.requests} == {0, 1}
    c = e.counters()
    assert e.ext_stats()["items"] == c["expansions"] + c["root_evals"]
    assert e.ext_stats()["requests"] <= 2 * c["steps"]
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. search_batch: three waves on a 16-slot engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("n,k,S,fixtures,tag", [(5, 4, 20, ["netgame_5x4.npz", "netgame_confident_5x4.npz"], "ckpt_saved"),
                                                 (9, 5, 8, ["netgame_9x5.npz", "netgame_full_9x5.npz"], "seeded")])
def test_search_batch_through_the_seam(n, k, S, fixtures, tag, with_noise):
    # 40 positions on 16 slots: three waves.  netgame_5x4.npz alone holds 31 positions, so each size takes the first 40 of its
    # two recorded games files (the helper of the search_batch tests would top up with random undecided positions)
    pos = _positions(n, k, 40, fixtures, seed=62)
    assert len(pos) == 40
    noise, us, Ts = _draws(pos, 61, with_noise)
    onet = orc.Net(n, weights_from_fixture(n, tag))
    o = orc.Oracle(n, k, S)
    e = _engine(n, k, S, 16)
    ev = CpuEvaluator(e, net_eval(onet))
    r = _batch(e, pos, noise, us, Ts)
    refs = _oracle_searches(o, onet, pos, noise, us, Ts)
    _assert_equal(r, refs, f"{n}x{n} search_batch vs the oracle")
    want = np.stack([o.encode(b, pl, la) for b, pl, la in pos[:16]])
    assert ev.requests[0] == (0, 16) and np.array_equal(ev.first_planes, want), "the first request: the first wave's positions, in order"
    c = e.counters()
    assert e.ext_stats()["items"] == c["expansions"] + c["root_evals"] and c["root_evals"] == 40
    # a loop of search_callback with the same evaluator (it ignores the setting: one position, one leaf per round trip)
    def cb(cells, player, last):
        _, P, v = onet.eval(o.encode(cells, player, last))
        return P, v
    for i, (b, pl, la) in enumerate(pos):
        rc = e.search_callback(b, pl, la, Ts[i], cb, None if noise is None else noise[i], us[i])
        for key in ("N", "W", "P", "pi"):
            assert np.array_equal(r[key][i], rc[key]), f"position {i}: {key} differs from search_callback"
        assert int(r["action"][i]) == rc["action"]
    assert e.external_evaluator()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. options, by identity with the native path
# ---------------------------------------------------------------------------------------------------------------------
def test_start_positions_resignation_and_virtual_loss_equal_the_native_engine():
    n, k, S, G, L, seed0 = 5, 4, 32, 6, 4, 300
    sd = weights_from_fixture(n, "ckpt_saved")
    nat = _engine(n, k, S, 4)
    nat.load_weights(sd, 0)
    nat.set_virtual_loss(L)
    # start positions: what the native games reach after two plies
    nat.selfplay(G, seed0=seed0)
    rec = nat.records(); nply, _ = nat.games()
    offs = np.concatenate([[0], np.cumsum(nply)[:-1]])
    assert (nply > 2).all()
    starts = (rec["boards"][offs + 2], rec["movers"][offs + 2], rec["lasts"][offs + 2])
    nat.set_start_positions(*starts)
    nat.selfplay(G, seed0=seed0)
    vals = nat.values(); nply, _ = nat.games()
    thr, crossing = choose_threshold(np.split(vals.astype(np.float64), np.cumsum(nply)[:-1]))
    nat.set_resign(thr)
    c_nat = nat.selfplay(G, seed0=seed0)
    want = dict(rec=nat.records(), values=nat.values(), resign=nat.resign_info(), games=nat.games())
    assert (want["resign"][0] >= 0).any(), "the threshold is low enough that some game crosses (the native run alone)"

    e = _engine(n, k, S, 4)
    e.set_virtual_loss(L)
    CpuEvaluator(e, net_eval(orc.Net(n, sd)))
    e.set_start_positions(*starts)
    e.set_resign(thr)
    c = e.selfplay(G, seed0=seed0)
    got = dict(rec=e.records(), values=e.values(), resign=e.resign_info(), games=e.games())
    for key in want["rec"]:
        assert np.array_equal(got["rec"][key], want["rec"][key]), f"records: {key}"
    assert np.array_equal(got["values"], want["values"])
    for a, b in zip(got["resign"] + got["games"], want["resign"] + want["games"]):
        assert np.array_equal(a, b)
    for key in ("plies", "simulations", "expansions", "root_evals", "terminal_hits", "depth_sum", "duplicate_leaves"):
        assert c[key] == c_nat[key], key
    nat.close(); e.close()


def test_deep_engine_through_the_seam():
    n, k, S, G, cut = 5, 4, 1040, 2, 2
    e = _engine(n, k, S, 2, deep=True)
    ev = CpuEvaluator(e, synth_eval(n))
    _play_vs_oracle(e, ev, orc.Oracle(n, k, S, synthetic=True), None, n, G, 77, cut, "deep 5x5")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. lifecycle
# ---------------------------------------------------------------------------------------------------------------------
def _episode(e, G=3, seed0=5, cut=0):
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    nply, res = e.games()
    return e.records(), nply.copy(), res.copy(), {key: c[key] for key in ("plies", "expansions", "simulations", "depth_sum")}


def _same_episode(a, b):
    return all(np.array_equal(a[0][key], b[0][key]) for key in a[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_calls_come_on_the_callers_thread_and_steps_without_items_make_none():
    n, k, S = 9, 5, 6
    e = _engine(n, k, S, 4, engines=2)
    assert e.lanes() == 2
    ev = CpuEvaluator(e, synth_eval(n))
    # both step APIs: begin / step / end
    e.selfplay_begin(4, seed0=3, max_plies=3)
    active = 1
    while active:
        active, _ = e.selfplay_step(1)
    c = e.selfplay_end()
    assert set(ev.threads) == {threading.get_ident()}, "no library thread ever calls the evaluator"
    gs = _oracle_games(orc.Oracle(n, k, S, synthetic=True), None, n, 4, 3, cut=3)
    _assert_games(e, gs, "step API, two lanes", cut=3)
    assert e.ext_stats()["items"] == c["expansions"] + c["root_evals"]
    e.close()
    # a search whose simulations all end in terminal leaves after the root: one request (the root), then steps without a call
    n, k, S = 3, 3, 12
    board = np.array([1, 2, 1, 2, 1, 2, 2, 1, 0], np.uint8)         # one empty cell: every simulation ends in a full board
    e = _engine(n, k, S, 1)
    ev = CpuEvaluator(e, synth_eval(n))
    r = e.search(board, 1, 6, 1.0)
    assert r["action"] == 8 and int(r["N"][8]) == S
    assert ev.requests == [(0, 1)] and e.ext_stats() == dict(requests=1, items=1)
    e.close()


def test_a_failing_evaluator_surfaces_and_the_engine_stays_usable():
    n, k, S = 5, 4, 16
    sd = weights_from_fixture(n, "ckpt_saved")
    e = _engine(n, k, S, 3)
    e.load_weights(sd, 0)
    before = _episode(e)
    ev = CpuEvaluator(e, net_eval(orc.Net(n, sd)))
    # a raised Python exception comes back as itself, after the C call has returned
    ev.fail_after = 5
    with pytest.raises(KeyError, match="gave up"):
        e.selfplay(3, seed0=5)
    with pytest.raises(az.AzError):
        e.games()                                    # the episode was closed, there is none
    # a non-zero return through the raw C-ABI: AZ_ERR_INVALID and its text
    import ctypes as C
    from alphazero_piskvorky_amd import _capi
    cb = _capi._EVAL_BATCH_FN(lambda user, net, count: 3)
    raw = _capi.az_ext_evaluator(ev.planes.data_ptr(), ev.policy.data_ptr(), ev.value.data_ptr(), e.ext_capacity(), cb, None)
    assert _capi.lib().az_set_external_evaluator(e.h, C.byref(raw)) == 0
    with pytest.raises(az.AzError, match=r"\(-1\).*the evaluator returned 3"):
        e.selfplay(3, seed0=5)
    # the evaluator again, healthy: the engine is usable and exact
    ev.fail_after = None
    e.set_external_evaluator(ev.planes.data_ptr(), ev.policy.data_ptr(), ev.value.data_ptr(), e.ext_capacity(), ev)
    assert _same_episode(_episode(e), before), "the oracle net through the seam = the same weights natively"
    # cleared: a native episode equals its earlier self, records included (ext_eval was put back)
    e.clear_external_evaluator()
    assert not e.external_evaluator()
    assert _same_episode(_episode(e), before)
    # ... and after a failed external episode as well
    ev.fail_after = 2
    e.set_external_evaluator(ev.planes.data_ptr(), ev.policy.data_ptr(), ev.value.data_ptr(), e.ext_capacity(), ev)
    with pytest.raises(KeyError):
        e.selfplay(3, seed0=5)
    e.clear_external_evaluator()
    assert _same_episode(_episode(e), before)
    e.close()


def test_search_callback_leaves_the_engines_state_alone():
    """search_callback searches through an evaluator of the engine's own; the public one, its statistics and the counters of
    the last call are as they were afterwards, whether the callback answered or raised."""
    n, k, S = 5, 4, 8
    sd = weights_from_fixture(n, "ckpt_saved")
    onet, o = orc.Net(n, sd), orc.Oracle(n, k, S)
    boards = np.zeros((3, n * n), np.uint8)
    boards[1, [6, 7]] = 1; boards[1, 12] = 2
    boards[2, [12, 13]] = 1; boards[2, [6, 18]] = 2
    players, lasts = np.array([1, 2, 1], np.uint8), np.array([-1, 7, 18], np.int16)
    e = _engine(n, k, S, 4)
    ev = CpuEvaluator(e, net_eval(onet))
    e.search_batch(boards, players, lasts, 1.0)
    stats, counters = e.ext_stats(), e.counters()
    assert stats["requests"] == len(ev.requests) > 0 and counters["root_evals"] == 3

    def cb(cells, player, last):
        _, P, v = onet.eval(o.encode(cells, player, last))
        return P, v

    def gives_up(cells, player, last):
        raise KeyError("the callback gave up")

    for fn in (cb, gives_up):
        if fn is cb:
            r = e.search_callback(boards[1], 2, 7, 1.0, fn)
            assert int(r["N"].sum()) == S
        else:
            with pytest.raises(KeyError, match="gave up"):
                e.search_callback(boards[1], 2, 7, 1.0, fn)
        assert e.external_evaluator()
        assert e.ext_stats() == stats and e.counters() == counters
        assert len(ev.requests) == stats["requests"], "the public evaluator is not called by search_callback"
        e.search_batch(boards, players, lasts, 1.0)
        assert len(ev.requests) == 2 * stats["requests"] and e.ext_stats() == stats, "the public evaluator serves the next search_batch"
        del ev.requests[stats["requests"]:]
        counters = e.counters()
    got =_episode(e, G=2, seed0=5, cut=2)
    e.close()
    fresh = _engine(n, k, S, 4)
    fresh.load_weights(sd, 0)
    assert _same_episode(got, _episode(fresh, G=2, seed0=5, cut=2))
    fresh.close()


def test_the_evaluation_cache_is_bypassed_and_back_in_force_after_clear():
    n, k, S = 5, 4, 16
    sd = weights_from_fixture(n, "ckpt_saved")
    e = _engine(n, k, S, 3)
    e.load_weights(sd, 0)
    e.set_eval_cache(4096)
    before = _episode(e)
    hits = e.counters()["cache_hits"]
    ev = CpuEvaluator(e, net_eval(orc.Net(n, sd)))
    assert _same_episode(_episode(e), before)
    c = e.counters()
    assert c["cache_lookups"] == c["cache_hits"] == 0, "the evaluation cache is bypassed on this path"
    e.clear_external_evaluator()
    assert _same_episode(_episode(e), before)
    assert e.counters()["cache_hits"] >= hits > 0, "the cache is back in force"
    e.close()


def test_refusals():
    n, k, S = 5, 4, 8
    e = _engine(n, k, S, 4)
    ev = CpuEvaluator(e, synth_eval(n))
    args = (ev.planes.data_ptr(), ev.policy.data_ptr(), ev.value.data_ptr())
    # reuse and leaf symmetry, in either order
    for setter in (e.set_subtree_reuse, e.set_leaf_symmetry):
        with pytest.raises(az.AzError, match=r"\(-1\)"):
            setter(True)
        e.clear_external_evaluator()
        setter(True)
        with pytest.raises(az.AzError, match=r"\(-1\)"):
            e.set_external_evaluator(*args, e.ext_capacity(), ev)
        assert not e.external_evaluator()
        setter(False)
        e.set_external_evaluator(*args, e.ext_capacity(), ev)
    # an open episode
    e.selfplay_begin(2, seed0=1, max_plies=2)
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.clear_external_evaluator()
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.set_external_evaluator(*args, e.ext_capacity(), ev)
    e.selfplay_step(1 << 20)
    e.selfplay_end()
    # a short capacity: at once, and at the next episode begin after raising L
    with pytest.raises(az.AzError, match=r"\(-1\)"):
        e.set_external_evaluator(*args, e.ext_capacity() - 1, ev)
    assert e.external_evaluator(), "a refused setting keeps the one in force"
    e.set_virtual_loss(2)
    assert e.ext_capacity() == 8
    for play in (lambda: e.selfplay(2, seed0=1), lambda: e.selfplay_begin(2, seed0=1), lambda: e.arena(2, seed0=1),
                 lambda: e.search(np.zeros(n * n, np.uint8), 1, -1, 1.0)):
        with pytest.raises(az.AzError, match=r"\(-1\).*hold 4 items"):
            play()
    e.set_virtual_loss(1)
    e.selfplay(2, seed0=1, max_plies=2)
    # NULL pointers and a NULL callback through the raw C-ABI
    import ctypes as C
    from alphazero_piskvorky_amd import _capi
    cb = _capi._EVAL_BATCH_FN(lambda user, net, count: 0)
    for bad in ((0, args[1], args[2], cb), (args[0], 0, args[2], cb), (args[0], args[1], 0, cb), (args[0], args[1], args[2], _capi._EVAL_BATCH_FN())):
        raw = _capi.az_ext_evaluator(bad[0], bad[1], bad[2], 4, bad[3], None)
        assert _capi.lib().az_set_external_evaluator(e.h, C.byref(raw)) == -1
    with pytest.raises(ValueError):
        e.set_external_evaluator(0, args[1], args[2], 4, ev)
    with pytest.raises(TypeError):
        e.set_external_evaluator(*args, 4, None)
    assert e.persistent() == 0
    e.clear_external_evaluator()
    e.close()
    # natively this engine shape runs the persistent kernel; with the evaluator set it never does
    e = _engine(n, k, S, 4, synthetic=True)
    e.selfplay(2, seed0=1, max_plies=2)
    assert e.persistent() > 0
    CpuEvaluator(e, synth_eval(n))
    e.selfplay(2, seed0=1, max_plies=2)
    assert e.persistent() == 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the Python seams
# ---------------------------------------------------------------------------------------------------------------------
def _controller(tag, n=5):
    m = az_net.GomokuNet(board_size=n)
    m.load_state_dict({key: torch.tensor(v) for key, v in weights_from_fixture(n, tag).items()})
    m.eval()
    return NeuralNetworkController(m, device=DEV)


def _oracle_batch_fn(onets):
    """a BatchPolicyValueFn whose answers are the oracle's: exact, so the shims can be compared bit for bit"""
    def fn(planes, net):
        pl = planes.cpu().numpy()
        out = list(_POOL.map(lambda j: onets[net].eval(pl[j]), range(len(pl))))
        return torch.from_numpy(np.stack([o[1] for o in out])), torch.tensor([o[2] for o in out], dtype=torch.float32)
    return BatchPolicyValueFn(fn, DEV)


def _states(fixture, n, k, count):
    out = []
    for b, pl, la in _fixture_positions(fixture)[:count]:
        s = az_games.Gomoku(n, k)
        s.cells = b.reshape(n, n).copy(); s.current_player = "X" if pl == 1 else "O"
        s.last_action = None if la < 0 else (la // n, la % n)
        out.append(s)
    return out


def test_mcts_with_a_batch_evaluator_equals_the_plain_callable():
    n, k, S = 5, 4, 12
    onet = orc.Net(n, weights_from_fixture(n, "ckpt_saved"))
    o = orc.Oracle(n, k, S)
    states = _states("netgame_5x4.npz", n, k, 10)

    def plain(state):
        _, P, v = onet.eval(o.encode(state.cells.reshape(-1), state.player_code(), state.last_index()))
        return P.reshape(n, n), v

    mb = MCTS(_oracle_batch_fn((onet,)), num_simulations=S, c_puct=2.0)
    mp = MCTS(plain, num_simulations=S, c_puct=2.0)
    for noise in (False, True):
        np.random.seed(17); rb = mb.run_many(states, 0.7, add_root_noise=noise); vb = mb.last_visits
        after_b = np.random.random_sample()
        np.random.seed(17); rp = mp.run_many(states, 0.7, add_root_noise=noise); vp = mp.last_visits
        assert after_b == np.random.random_sample(), "the same draws from numpy's global RNG, in the same order"
        assert np.array_equal(vb, vp)
        for (pb, ab), (pp, ap) in zip(rb, rp):
            assert ab == ap and np.array_equal(pb, pp)
    np.random.seed(4); one_b = mb.run(states[3], 1.0, add_root_noise=True)
    np.random.seed(4); one_p = mp.run(states[3], 1.0, add_root_noise=True)
    assert one_b[1] == one_p[1] and np.array_equal(one_b[0], one_p[0]) and np.array_equal(mb.last_visits, mp.last_visits)


def test_self_play_manager_and_model_evaluator_with_evaluators():
    n = 5
    sd_c, sd_b = weights_from_fixture(n, "ckpt_saved"), weights_from_fixture(n, "ckpt_0802")
    cand, base = _controller("ckpt_saved"), _controller("ckpt_0802")
    oc, ob = orc.Net(n, sd_c), orc.Net(n, sd_b)
    params = {"num_simulations": 16, "c_puct": 2.0}
    native = SelfPlayManager(cand, DEV, mcts_params=params, concurrent_games=3, seed=9).generate_self_play(4)
    ext = SelfPlayManager(cand, DEV, mcts_params=params, concurrent_games=3, seed=9,
                          evaluator=_oracle_batch_fn((oc,))).generate_self_play(4)
    assert len(native) == len(ext) > 0
    for (s0, p0, z0), (s1, p1, z1) in zip(native, ext):
        assert s0.numpy().tobytes() == s1.numpy().tobytes() and p0.tobytes() == p1.tobytes() and z0 == z1
    with pytest.raises(TypeError):
        SelfPlayManager(cand, DEV, evaluator=lambda planes, net: None)
    with pytest.raises(ValueError):
        SelfPlayManager(cand, DEV, evaluator=_oracle_batch_fn((oc,)), subtree_reuse=True)
    from alphazero_piskvorky_amd import constants
    saved = constants.NUM_EVAL_SIMULATIONS
    constants.NUM_EVAL_SIMULATIONS = 16
    try:
        wr0, m0 = ModelEvaluator(device=DEV, seed=31).evaluate(cand, base, num_games=6)
        wr1, m1 = ModelEvaluator(device=DEV, seed=31, evaluators=(_oracle_batch_fn((oc,)), _oracle_batch_fn((ob, ob)))).evaluate(cand, base, num_games=6)
        wr2, m2 = ModelEvaluator(device=DEV, seed=31, evaluators=True).evaluate(cand, base, num_games=6)
    finally:
        constants.NUM_EVAL_SIMULATIONS = saved
    assert (wr0, m0) == (wr1, m1)
    assert m2["total"] == 6              # torch's numbers: the contract, not bit-exactness


def test_make_batch_policy_value_fn_contract_and_tolerance():
    n, k = 5, 4
    ctrl = _controller("ckpt_saved")
    bf = make_batch_policy_value_fn(ctrl.net)
    assert isinstance(bf, BatchPolicyValueFn)
    pos = _fixture_positions("netgame_5x4.npz")[:24]
    o = orc.Oracle(n, k, 1)
    planes = torch.from_numpy(np.stack([o.encode(b, pl, la) for b, pl, la in pos])).to(DEV)
    P, v = bf.fn(planes, 0)
    assert P.shape == (24, n * n) and v.reshape(-1).shape == (24,) and P.is_cuda and not P.requires_grad
    np.testing.assert_allclose(P.sum(dim=1).cpu().numpy(), 1.0, rtol=0, atol=1e-5)
    e = az.Engine(n, k, 1, 4)
    e.load_weights(ctrl.net.state_dict(), 0)
    _, Pn, vn = e.net_eval(np.stack([b for b, _, _ in pos]), [pl for _, pl, _ in pos], [la for _, _, la in pos])
    e.close()
    # the tolerances the project already grants torch's numbers
    np.testing.assert_allclose(P.cpu().numpy(), Pn, rtol=0, atol=1e-6)
    np.testing.assert_allclose(v.reshape(-1).cpu().numpy(), vn, rtol=0, atol=2e-6)
    # through the engine: searches run, pi is a distribution
    m = MCTS(bf, num_simulations=10, c_puct=2.0)
    np.random.seed(1)
    for pi, a in m.run_many(_states("netgame_5x4.npz", n, k, 6), 1.0, add_root_noise=True):
        assert pi.shape == (n, n) and abs(float(pi.sum()) - 1.0) < 1e-5 and a is not None
    with pytest.raises(TypeError):
        make_batch_policy_value_fn(lambda x: x)
    # a (candidate, baseline) pair answers by net id
    pair = make_batch_policy_value_fn((ctrl.net, _controller("ckpt_0802").net))
    assert not torch.equal(pair.fn(planes, 0)[0], pair.fn(planes, 1)[0])


def test_train_loop_runs_on_the_torch_evaluator():
    from alphazero_piskvorky_amd import constants, train
    saved = (constants.BATCHES_PER_EPISODE, constants.NUM_EPOCHS, constants.BATCH_SIZE)
    constants.BATCHES_PER_EPISODE, constants.NUM_EPOCHS, constants.BATCH_SIZE = 2, 1, 256
    try:
        hist = train.run(episodes=1, games=8, sims=12, eval_games=4, device=DEV, seed=3, log=lambda *_: None, torch_eval=True)
    finally:
        constants.BATCHES_PER_EPISODE, constants.NUM_EPOCHS, constants.BATCH_SIZE = saved
    assert len(hist) == 1 and hist[0]["examples"] > 0 and np.isfinite(hist[0]["loss"])
    assert hist[0]["total"] == 4 and hist[0]["wins"] + hist[0]["losses"] + hist[0]["draws"] == 4
