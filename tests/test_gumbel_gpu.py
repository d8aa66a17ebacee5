"""az_set_gumbel on the GPU, against the numpy restatement in tests/gumbel.py (which with the option off is the oracle's search,
tests/test_gumbel_cpu.py).  The evaluator of the restatement is the engine's own az_net_eval (logits, policy, value) with the
fixture nets.  Comparisons are exact -- integer equality for visits and actions, == on the float64 W and on the float32 priors
-- except pi against numpy: the engine's exp and np.exp differ far below 2^-24 relative, so the two float32 roundings are at
most one float32 spacing apart.  Against az_gumbel_target, fed the engine's own root statistics, pi is exact as well."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import gumbel
from tests.test_playout_cap_cpu import np_full
from tests.util import ROOT, load, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

C_PUCT = 2.0
SIZES = ((5, 4), (9, 5), (15, 5))
M1, S1 = 16, 32
REC_KEYS = ("boards", "movers", "lasts", "actions", "visits", "z")


# ---------------------------------------------------------------------------------------------------------------------
# nets, evaluators, positions and references (computed once, never modified)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(n, model="plain"):
    if model == "resnet":
        z = load("resnet_ckpt_5.npz")
        return {k[3:]: z[k] for k in z.files if k.startswith("w__")}
    return weights_from_fixture(n, "ckpt_saved" if n == 5 else "seeded")


_EVAL = {}


def evaluator(n, k, model="plain"):
    """evaluate(board, player, last) -> (logits, P, v) through az_net_eval of an engine of its own; answers are remembered"""
    if (n, model) not in _EVAL:
        e = az.Engine(n, k, 1, 1, model=model)
        e.load_weights(weights(n, model), 0)
        seen = {}

        def evaluate(board, player, last):
            key = (np.asarray(board, np.uint8).tobytes(), int(player), int(last))
            if key not in seen:
                lg, P, v = e.net_eval(np.asarray(board, np.uint8)[None], [player], [last])
                seen[key] = (lg[0].copy(), P[0].copy(), np.float32(v[0]))
            return seen[key]
        _EVAL[(n, model)] = (e, evaluate)
    return _EVAL[(n, model)][1]


FEW = np.array([1, 1, 2, 2, 1,
                2, 2, 1, 1, 2,
                1, 1, 2, 2, 1,
                2, 2, 1, 1, 2,
                1, 2, 0, 0, 0], np.uint8)          # 5x5, k = 4: three empty cells, no line, X to move after O at cell 21


@functools.lru_cache(maxsize=None)
def positions(n, k):
    """the empty board and two mid-game positions, each with its Gumbel draws, uniform and temperature"""
    out = []
    for i, (stones, seed) in enumerate(((0, 1), (6, 2), (11, 3))):
        board, player, last = gumbel.random_position(n, k, stones, seed)
        rs = np.random.RandomState(1000 * n + i)
        g = rs.gumbel(size=int((board == 0).sum()))
        out.append(dict(board=board, player=player, last=last, noise=g, u=float(rs.random_sample()), T=(1.0, 0.5, 1e-9)[i]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def few_position():
    assert not any(gumbel.wins_through(FEW, a, 5, 4) for a in np.flatnonzero(FEW))
    return dict(board=FEW, player=1, last=21, noise=np.random.RandomState(77).gumbel(size=3), u=0.5, T=1.0)


_TREES = {}


def tree(p, n, k, S, m, cv=50.0, cs=1.0, model="plain", key=None):
    kk = (key, n, S, m, cv, cs, model)
    if key is None or kk not in _TREES:
        r = gumbel.search_move(evaluator(n, k, model), n, k, S, p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"],
                               m=m, c_visit=cv, c_scale=cs, c_puct=C_PUCT)
        if key is None:
            return r
        _TREES[kk] = r
    return _TREES[kk]


def engine(n, k, S, slots, model="plain", **kw):
    e = az.Engine(n, k, S, slots, log_table=orc.numpy_log_table(S), c_puct=C_PUCT, model=model, **kw)
    e.load_weights(weights(n, model), 0)
    return e


def assert_search(r, want, p, n, k, m, what, cv=50.0, cs=1.0, model="plain"):
    board = p["board"]
    legal = np.flatnonzero(board == 0)
    assert np.array_equal(r["N"], want["N"]), f"{what}: visits"
    assert np.array_equal(r["W"], want["W"]), f"{what}: W"
    assert np.array_equal(r["P"], want["P"]), f"{what}: priors"
    lg, P0, v0 = evaluator(n, k, model)(board, p["player"], p["last"])
    assert np.array_equal(r["P"][legal], P0[legal]), f"{what}: the prior is the unmixed softmax"
    assert int(r["action"]) == want["action"], f"{what}: action"
    pi, a = _capi.gumbel_target(lg[legal], p["noise"], r["N"][legal], r["W"][legal], r["P"][legal], v0, cv, cs)
    assert r["pi"].dtype == np.float32 and np.array_equal(r["pi"][legal], pi) and not r["pi"][board != 0].any(), f"{what}: pi = az_gumbel_target"
    assert int(legal[a]) == int(r["action"])
    assert gumbel.within_one_float32_step(r["pi"], want["pi64"]), f"{what}: pi against numpy"
    S = int(r["N"].sum())
    assert sorted(r["N"][r["N"] > 0].tolist()) == gumbel.schedule_visits(min(m, len(legal)), S), f"{what}: the schedule's visits"


def batch(e, ps):
    rb = e.search_batch(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps],
                        np.array([p["T"] for p in ps]), [p["noise"] for p in ps], [p["u"] for p in ps])
    return [{key: val[i] for key, val in rb.items()} for i in range(len(ps))]


# ---------------------------------------------------------------------------------------------------------------------
# 1. single searches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", SIZES)
def test_single_searches_equal_the_restatement(n, k):
    """5x5: one cell per lane and the persistent kernel (az_search one game per workgroup, az_search_batch two); 9x9: two cells
    per lane; 15x15: four.  m = 16, S = 32; the same search with the option off gives other visits on every position."""
    e = engine(n, k, S1, 4)
    ps = positions(n, k)
    off = [e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"]) for p in ps]
    e.set_gumbel(M1)
    assert e.gumbel() == dict(m=M1, c_visit=50.0, c_scale=1.0)
    rbs = batch(e, ps)
    assert (e.persistent() > 0) == (n == 5)
    for i, (p, rb) in enumerate(zip(ps, rbs)):
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        assert (e.persistent() > 0) == (n == 5)
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, tree(p, n, k, S1, M1, key=i), p, n, k, M1, f"{n}x{n} position {i} {what}")
        assert not np.array_equal(r["N"], off[i]["N"]), f"{n}x{n} position {i}: the option changes nothing"
        assert not np.array_equal(r["P"], off[i]["P"]), "the option-off search mixes the draws in as Dirichlet noise"
    e.close()


@pytest.mark.parametrize("m,S,which", [(4, 16, 1), (16, 8, 1), (16, 32, "few"), (1, 16, 2), (25, 32, 0)],
                         ids=["m4-S16", "S-below-m", "m-above-legal", "m1", "m-all-cells"])
def test_edges(m, S, which):
    n, k = 5, 4
    p = few_position() if which == "few" else positions(n, k)[which]
    e = engine(n, k, S, 2)
    e.set_gumbel(m)
    want = tree(p, n, k, S, m)
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    rb = batch(e, [p, p])[1]
    for got, what in ((r, "az_search"), (rb, "az_search_batch")):
        assert_search(got, want, p, n, k, m, f"m {m} S {S} {which} {what}")
    if m == 1:
        assert (r["N"] > 0).sum() == 1
    e.close()


def test_other_constants():
    n, k = 9, 5
    p = positions(n, k)[1]
    e = engine(n, k, S1, 1)
    for cv, cs in ((0.0, 0.1), (20.0, 3.0)):
        e.set_gumbel(8, cv, cs)
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        assert_search(r, tree(p, n, k, S1, 8, cv, cs), p, n, k, 8, f"c_visit {cv} c_scale {cs}", cv, cs)
    e.close()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import test_gumbel_gpu as t
e = t.engine(5, 4, t.S1, 4)
e.set_gumbel(t.M1)
ps = t.positions(5, 4)
out = {}
for i, (p, rb) in enumerate(zip(ps, t.batch(e, ps))):
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    assert e.persistent() == 0
    for tag, got in (("s", r), ("b", rb)):
        for key in ("N", "W", "P", "pi"):
            out[f"{tag}{i}_{key}"] = got[key]
        out[f"{tag}{i}_action"] = np.int64(got["action"])
e.close()
np.savez(sys.argv[2], **out)
"""


def test_lock_step_path_in_a_fresh_process(tmp_path):
    """AZ_PERSIST=0: the 5x5 searches through k_step instead of the persistent kernel"""
    path = str(tmp_path / "child.npz")
    env = {key: v for key, v in os.environ.items() if key not in ("AZ_COMPACT", "AZ_GRAPH", "AZ_PROFILE_EVENTS")}
    env["AZ_PERSIST"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(path)
    for i, p in enumerate(positions(5, 4)):
        for tag in "sb":
            got = {key: z[f"{tag}{i}_{key}"] for key in ("N", "W", "P", "pi", "action")}
            assert_search(got, tree(p, 5, 4, S1, M1, key=i), p, 5, 4, M1, f"AZ_PERSIST=0 position {i} {tag}")


def test_deep_engine_1100_simulations():
    """16-bit counts, the DEEP tree kernel, a schedule row of 1100 entries"""
    n, k, S = 5, 4, 1100
    p = positions(n, k)[1]
    want = tree(p, n, k, S, M1)
    assert want["N"].max() > 256
    e = engine(n, k, S, 1, deep=True)
    e.set_gumbel(M1)
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    assert e.persistent() == 0
    assert_search(r, want, p, n, k, M1, "deep")
    e.close()


@pytest.mark.parametrize("persist", ["1", "0"], ids=["persistent", "lock-step"])
def test_residual_block_net_5x5(persist, monkeypatch):
    monkeypatch.setenv("AZ_PERSIST", persist)
    n, k = 5, 4
    e = engine(n, k, S1, 4, model="resnet")
    e.set_gumbel(M1)
    ps = positions(n, k)
    for i, (p, rb) in enumerate(zip(ps, batch(e, ps))):
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        assert (e.persistent() > 0) == (persist == "1")
        for got, what in ((r, "az_search"), (rb, "az_search_batch")):
            assert_search(got, tree(p, n, k, S1, M1, model="resnet", key=i), p, n, k, M1, f"resnet position {i} {what}", model="resnet")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. whole self-play games
# ---------------------------------------------------------------------------------------------------------------------
GAMES, MG, SG = 6, 8, 16


@functools.lru_cache(maxsize=None)
def ref_games(n, k, seed0, cap=None):
    return tuple(gumbel.selfplay_game(evaluator(n, k), n, k, SG, _capi.selfplay_tape_gumbel(seed0 + g, n), MG, cap=cap,
                                      full_fn=lambda s, p, pm: np_full(s, p, pm), seed=seed0 + g) for g in range(GAMES))


def episode(e, seed0, games=GAMES, **kw):
    c = e.selfplay(games, seed0=seed0, **kw)
    nply, res = e.games()
    return dict(rec=e.records(), nply=nply, res=res, values=e.values(), c=c)


def assert_games(ep, games, what):
    assert ep["nply"].tolist() == [g["nply"] for g in games], f"{what}: plies per game"
    assert ep["res"].tolist() == [g["result"] for g in games], f"{what}: results"
    for key in REC_KEYS:
        exp = np.concatenate([g[key] for g in games])
        assert ep["rec"][key].shape == exp.shape and np.array_equal(ep["rec"][key], exp), f"{what}: {key}"
    assert np.array_equal(ep["values"], np.concatenate([g["values"] for g in games])), f"{what}: values"
    full = np.concatenate([g["full"] for g in games])
    pis, pis64 = np.concatenate([g["pis"] for g in games]), np.concatenate([g["pis64"] for g in games])
    assert np.array_equal(ep["rec"]["pis"][~full], pis[~full]), f"{what}: pi of the FAST plies"
    assert gumbel.within_one_float32_step(ep["rec"]["pis"][full], pis64[full]), f"{what}: pi of the Gumbel plies"


@pytest.mark.parametrize("n,k,seed0,cap", [pytest.param(5, 4, 5300, None, id="5x5"), pytest.param(9, 5, 5400, None, id="9x9"),
                                           pytest.param(5, 4, 5300, (4, 500), id="5x5-cap"), pytest.param(9, 5, 5400, (4, 500), id="9x9-cap")])
def test_self_play_games_equal_the_restatement_ply_by_ply(n, k, seed0, cap):
    """m = 8, S = 16, six games on four slots (refill happens), the engine's own tapes = _capi.selfplay_tape_gumbel.  With the
    playout cap (F = 4, 500 permille) the FAST plies are the plain search without noise, the FULL ones the Gumbel search."""
    games = ref_games(n, k, seed0, cap)
    e = engine(n, k, SG, 4)
    e.set_gumbel(MG)
    if cap:
        e.set_playout_cap(cap[0], cap[1] / 1000)
        full = np.concatenate([g["full"] for g in games])
        assert full.any() and not full.all()
    ep = episode(e, seed0)
    assert (e.persistent() > 0) == (n == 5 and not cap)
    assert_games(ep, games, f"{n}x{n} cap {cap}")
    # both step APIs: the same episode through begin / step / end
    e.selfplay_begin(GAMES, seed0=seed0)
    while e.selfplay_step(3)[0]:
        pass
    e.selfplay_end()
    nply, res = e.games()
    assert_games(dict(rec=e.records(), nply=nply, res=res, values=e.values()), games, f"{n}x{n} cap {cap}, step API")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. option combinations
# ---------------------------------------------------------------------------------------------------------------------
def test_the_evaluation_cache_changes_nothing():
    n, k, seed0 = 5, 4, 5300
    out = []
    for cache in (0, 1 << 12):
        e = engine(n, k, SG, 4)
        e.set_gumbel(MG)
        e.set_eval_cache(cache)
        ep = episode(e, seed0)
        out.append(ep)
        if cache:
            assert ep["c"]["cache_hits"] > 0
        e.close()
    for key in out[0]["rec"]:
        assert out[0]["rec"][key].tobytes() == out[1]["rec"][key].tobytes(), key
    assert_games(out[1], ref_games(n, k, seed0), "eval cache")


def test_options_the_restatement_does_not_cover_do_not_depend_on_slots_and_lanes():
    """Leaf symmetry (the logits are read through it) and the bf16x3 trunk (not bit-exact by design), with start positions,
    resignation and max_plies: the episode is the same on 6 slots in 2 lanes and on 4 slots in 1 lane, and it is not the
    episode with the option off."""
    n, k, S, G, seed0 = 5, 4, 32, 8, 5500
    ps = positions(n, k)[1:]

    def run(slots, lanes, m):
        e = engine(n, k, S, slots, engines=lanes)
        e.set_leaf_symmetry(True)
        e.set_trunk_mode("bf16x3")
        e.set_resign(0.9, 2, 0.25)
        e.set_start_positions(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps])
        if m:
            e.set_gumbel(m)
        e.selfplay(G, seed0=seed0, max_plies=18)
        nply, res = e.games()
        out = dict(e.records(), values=e.values(), nply=nply, res=res)
        e.close()
        return out
    a, b, off = run(6, 2, M1), run(4, 1, M1), run(4, 1, 0)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["visits"].tobytes() != off["visits"].tobytes()


def test_searches_without_noise_the_arena_and_fast_plies_are_untouched():
    """The all-FAST episode runs on an explicit tape: a tape the engine generates itself holds other uniforms under the
    option (a Gumbel draw takes one random_sample, a Dirichlet sample a varying number), an explicit one is taken as given."""
    n, k, S = 5, 4, 32
    p = positions(n, k)[1]
    tapes = [_capi.rng_selfplay_tape(5200 + g, n) for g in range(4)]
    nz, ut = np.stack([t[0] for t in tapes]), np.stack([t[1] for t in tapes])

    def run(m):
        e = engine(n, k, S, 4)
        e.load_weights(weights_from_fixture(n, "seeded"), 1)
        if m:
            e.set_gumbel(m)
        s = e.search(p["board"], p["player"], p["last"], p["T"], None, p["u"])
        sb = e.search_batch(p["board"][None], [p["player"]], [p["last"]], p["T"], None, [p["u"]])
        ar = e.arena(4, seed0=77, temperature_table=orc.arena_T_table(n * n))
        ar_rec = e.records()
        e.set_playout_cap(8, 0.0)                  # every ply FAST: no noise anywhere
        e.selfplay(4, seed0=5200, noise_tape=nz, u_tape=ut)
        fast = dict(e.records(), values=e.values(), nply=e.games()[0])
        e.close()
        return s, sb, ar, ar_rec, fast
    a, b = run(0), run(M1)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key in x:
            assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), key


@pytest.mark.parametrize("n,k", [(5, 4), (9, 5)], ids=["persistent", "lock-step"])
def test_a_captured_ply_graph_does_not_outlive_the_setting(n, k):
    """the same engine, more games than slots: on, off, on again.  Both paths replay a captured graph of the ply."""
    e = engine(n, k, 16, 2)

    def run():
        c = e.selfplay(3, seed0=9, max_plies=6)
        return c["expansions"], e.records()["visits"].copy(), e.records()["pis"].copy()
    e.set_gumbel(MG)
    a = run()
    e.set_gumbel(0)
    b = run()
    e.set_gumbel(MG)
    c = run()
    assert (e.persistent() > 0) == (n == 5)
    assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2]) and a[0] == c[0] and not np.array_equal(a[1], b[1])
    onet = orc.Net(n, weights(n))
    assert np.array_equal(b[1], np.concatenate([orc.Oracle(n, k, 16).selfplay_game(onet, *_capi.rng_selfplay_tape(9 + g, n, max_plies=6),
                                                                                   maxply=6)["visits"] for g in range(3)]))
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the setters
# ---------------------------------------------------------------------------------------------------------------------
def test_setters():
    L = _capi.lib()
    e = engine(5, 4, 16, 2)
    off = dict(m=0, c_visit=50.0, c_scale=1.0)
    assert e.gumbel() == off
    e.set_gumbel(16)
    on = dict(m=16, c_visit=50.0, c_scale=1.0)
    assert e.gumbel() == on
    for bad in ((-1, 50.0, 1.0), (26, 50.0, 1.0), (65, 50.0, 1.0), (8, -1.0, 1.0), (8, float("nan"), 1.0), (8, float("inf"), 1.0),
                (8, 50.0, 0.0), (8, 50.0, -2.0), (8, 50.0, float("inf")), (8, 50.0, float("nan"))):
        assert L.az_set_gumbel(e.h, *bad) == -1, bad
        assert e.gumbel() == on
    e.set_gumbel(25, 0.0, 0.5)
    assert e.gumbel() == dict(m=25, c_visit=0.0, c_scale=0.5)
    assert L.az_get_gumbel(e.h, None, None, None) == 0
    e.set_gumbel(16)
    # every refused pair, the Gumbel search set first ...
    refused = r"\(-1\)"
    with pytest.raises(az.AzError, match=refused):
        e.set_subtree_reuse(True)
    with pytest.raises(az.AzError, match=refused):
        e.set_virtual_loss(4)
    with pytest.raises(az.AzError, match=refused):
        e.set_forced_playouts(2.0)
    import torch
    from alphazero_piskvorky_amd.controller import BatchPolicyValueFn
    fn = BatchPolicyValueFn(lambda planes, net: (torch.zeros(len(planes), 25), torch.zeros(len(planes))), "cuda:0")
    with pytest.raises(az.AzError, match=refused):
        fn.attach(e)
    p = positions(5, 4)[1]
    with pytest.raises(az.AzError, match=refused):
        e.search_callback(p["board"], p["player"], p["last"], 1.0, lambda c, pl, la: (np.full(25, 0.04, np.float32), 0.0), p["noise"], 0.5)
    e.search_callback(p["board"], p["player"], p["last"], 1.0, lambda c, pl, la: (np.full(25, 0.04, np.float32), 0.0), None, 0.5)
    assert e.gumbel() == on
    # ... and second; switching off is always allowed
    assert L.az_set_gumbel(e.h, 0, -7.0, -7.0) == 0 and e.gumbel()["m"] == 0
    for setup, undo in ((lambda: e.set_subtree_reuse(True), lambda: e.set_subtree_reuse(False)),
                        (lambda: e.set_virtual_loss(4), lambda: e.set_virtual_loss(1)),
                        (lambda: e.set_forced_playouts(2.0), lambda: e.set_forced_playouts(0.0)),
                        (lambda: fn.attach(e), lambda: e.clear_external_evaluator())):
        setup()
        with pytest.raises(az.AzError, match=refused):
            e.set_gumbel(16)
        assert e.gumbel()["m"] == 0
        e.set_gumbel(0)
        undo()
        e.set_gumbel(16)
        e.set_gumbel(0)
    s = az.Engine(5, 4, 16, 2, synthetic=True)
    with pytest.raises(az.AzError, match=refused):
        s.set_gumbel(16)
    s.close()
    # an open episode
    e.set_gumbel(16)
    e.selfplay_begin(2, seed0=1)
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.set_gumbel(8)
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.set_gumbel(0)
    e.selfplay_step(1 << 20)
    e.selfplay_end()
    assert e.gumbel() == on
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the shims
# ---------------------------------------------------------------------------------------------------------------------
def _controller(n=5):
    import torch
    from alphazero_piskvorky_amd import net
    from alphazero_piskvorky_amd.controller import NeuralNetworkController
    m = net.GomokuNet(board_size=n)
    m.load_state_dict({key: torch.tensor(v) for key, v in weights(n).items()})
    m.eval()
    return NeuralNetworkController(m, device="cuda:0")


def test_self_play_manager_shim():
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    n, k, seed0 = 5, 4, 5300
    mgr = SelfPlayManager(_controller(), "cuda:0", mcts_params={"num_simulations": SG, "c_puct": C_PUCT}, concurrent_games=4, seed=seed0,
                          gumbel={"m": MG})
    data = mgr.generate_self_play(GAMES)
    assert mgr._engine.gumbel() == dict(m=MG, c_visit=50.0, c_scale=1.0)
    eng = mgr._engine
    nply, res = eng.games()
    assert_games(dict(rec=eng.records(), nply=nply, res=res, values=eng.values()), ref_games(n, k, seed0), "SelfPlayManager")
    assert len(data) == 4 * int(nply.sum())
    mgr.gumbel = None                              # the next episode switches the engine's option off again
    mgr.generate_self_play(2)
    assert mgr._engine.gumbel()["m"] == 0


def test_mcts_run_shim_with_a_seeded_global_rng():
    from alphazero_piskvorky_amd import games
    from alphazero_piskvorky_amd.controller import make_policy_value_fn
    from alphazero_piskvorky_amd.mcts import MCTS
    n, k = 5, 4
    m = MCTS(make_policy_value_fn(_controller()), num_simulations=S1, c_puct=C_PUCT, gumbel={"m": M1})
    p = positions(n, k)[1]
    s = games.Gomoku(n, k)
    s.cells = p["board"].copy(); s.current_player = "X" if p["player"] == 1 else "O"
    s.last_action = (p["last"] // n, p["last"] % n)
    states = [s, games.Gomoku(n, k)]
    np.random.seed(4242)
    got = [m.run(st, temperature=1.0, add_root_noise=True) for st in states]
    np.random.seed(4242)
    many = m.run_many(states, 1.0, add_root_noise=True)
    rs = np.random.RandomState(4242)
    for st, (pi, a), (pi2, a2) in zip(states, got, many):
        board = np.asarray(st.cells, np.uint8).reshape(-1)
        g = rs.gumbel(size=int((board == 0).sum()))
        u = rs.random_sample()
        q = dict(board=board, player=st.player_code(), last=st.last_index(), noise=g, u=u, T=1.0)
        want = tree(q, n, k, S1, M1)
        assert a == (want["action"] // n, want["action"] % n) == a2
        assert gumbel.within_one_float32_step(pi.reshape(-1), want["pi64"]) and np.array_equal(pi, pi2)
    # without root noise the shim is the plain search
    np.random.seed(1)
    pi_off, _ = m.run(s, temperature=1.0)
    np.random.seed(1)
    pi_ref, _ = MCTS(make_policy_value_fn(_controller()), num_simulations=S1, c_puct=C_PUCT).run(s, temperature=1.0)
    assert np.array_equal(pi_off, pi_ref)
