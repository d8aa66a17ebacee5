"""az_set_playout_cap on the GPU.  The reference is the unchanged CPU oracle, restated ply by ply: two Oracle objects, one with
num_simulations = S and one with F, and a Python loop over the plies of every game that calls Oracle.search on the one the
header's hash picks -- with the ply's slice of the noise tape for a FULL ply, with noise = None for a FAST one -- applies the
action and checks the end with Oracle.replay.  The engine has to produce exactly those games: array_equal everywhere, no
tolerances.

Where the oracle cannot serve (its single search cannot name the ply, which the leaf-symmetry hash needs; the emulated
trunks are not bit-exact by design) the two end points and independence stand in: 1000 permille is the episode with the cap
off, and the records of a capped episode do not depend on slots, lanes or compaction.

Every case first asserts, from the formula alone, that its own configuration mixes both kinds of ply."""
import functools
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_playout_cap_cpu import full_table, np_full
from tests.test_resign_gpu import choose_threshold, first_cross
from tests.util import ROOT, load, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

REC_KEYS = ("boards", "movers", "lasts", "actions", "pis", "visits", "z")
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------------
# the reference: the oracle loop
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(n, tag):
    """(weights for the engine, oracle net, engine model kind); tag None = the synthetic evaluator"""
    if tag is None:
        return None, None, "plain"
    if tag == "resnet_ckpt":
        from alphazero_piskvorky_amd.net import fold_resnet_state_dict
        z = load("resnet_ckpt_5.npz")
        sd = {k[3:]: z[k] for k in z.files if k.startswith("w__")}
        return sd, orc.Net(n, resnet_tensors=fold_resnet_state_dict(sd)), "resnet"
    sd = weights_from_fixture(n, tag)
    return sd, orc.Net(n, sd), "plain"


def _z(movers, res):
    movers = np.asarray(movers, np.int64)
    return (np.full(len(movers), 99) if res == 0 else (np.zeros(len(movers)) if res == 3 else np.where(movers == res, 1, -1))).astype(np.int8)


def capped_game(oS, oF, net, n, seed, permille, cut=0, prefix=()):
    """one game of the rule, restated: ply m is searched by oS with its noise when FULL, by oF without noise when FAST.
    prefix: actions already on the board (the game continues a start position; plies stay absolute)."""
    nn = n * n
    noise, us = orc.selfplay_tape(seed, n, maxply=cut or None)
    T = orc.selfplay_T_table(nn)
    actions = [int(a) for a in prefix]
    rc, _, board, player, res = oS.replay(actions)
    assert rc == 0 and res == 0
    last = actions[-1] if actions else -1
    out = {key: [] for key in REC_KEYS[:-1] + ("values", "sims")}
    m = len(actions)
    off = sum(nn - i for i in range(m))
    while True:
        full = bool(np_full(seed, m, permille))
        o = oS if full else oF
        ro = o.search(net, board, player, last, T[m], noise[off:off + nn - m] if full else None, us[m], game=seed)
        a = int(ro["action"])
        astar = int(np.argmax(ro["N"]))
        assert ro["N"].sum() == o.S and board[a] == 0
        out["boards"].append(board.copy()); out["movers"].append(player); out["lasts"].append(last); out["actions"].append(a)
        out["pis"].append(ro["pi"]); out["visits"].append(ro["N"])
        out["values"].append(np.float32(np.float64(ro["W"][astar]) / np.float64(ro["N"][astar])))
        out["sims"].append(o.S)
        actions.append(a)
        board = board.copy(); board[a] = player
        last, player, off, m = a, 3 - player, off + nn - m, m + 1
        rc, _, b2, p2, res = oS.replay(actions)
        assert rc == 0 and np.array_equal(b2, board) and p2 == player
        if res != 0 or (cut and m >= cut):
            break
    g = dict(boards=np.array(out["boards"], np.uint8), movers=np.array(out["movers"], np.uint8), lasts=np.array(out["lasts"], np.int16),
             actions=np.array(out["actions"], np.int16), pis=np.array(out["pis"], np.float32), visits=np.array(out["visits"], np.int32),
             values=np.array(out["values"], np.float32), sims=np.array(out["sims"], np.int32), result=int(res), start=len(prefix))
    g["nply"] = len(g["actions"])
    g["z"] = _z(g["movers"], g["result"])
    return g


@functools.lru_cache(maxsize=None)
def _ref(n, k, S, F, G, seed0, permille, tag, cut=0, vl=0):
    """G games of the oracle loop with seeds seed0 + g, computed once per configuration and never modified"""
    oS = orc.Oracle(n, k, S, synthetic=tag is None, virtual_loss=vl)
    oF = orc.Oracle(n, k, F, synthetic=tag is None, virtual_loss=vl)
    net = _weights(n, tag)[1]
    with ThreadPoolExecutor(max_workers=8) as ex:
        return tuple(ex.map(lambda g: capped_game(oS, oF, net, n, seed0 + g, permille, cut), range(G)))


def _engine(n, k, S, slots, tag, **kw):
    sd, _, model = _weights(n, tag)
    e = az.Engine(n, k, S, slots, synthetic=tag is None, log_table=orc.numpy_log_table(S), model=model, **kw)
    if sd is not None:
        e.load_weights(sd, 0)
    return e


def _episode(e, G, seed0, cut=0):
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    return _collect(e, c)


def _collect(e, c):
    nply, res = e.games()
    return dict(rec=e.records(), nply=nply, res=res, values=e.values(), sims=e.sims(), c=c)


def assert_games(ep, games, what):
    """the engine's episode = these games: lengths, results, every record field, the value and the simulations of every record,
    and the work counters as sums over them"""
    assert ep["nply"].tolist() == [g["nply"] for g in games], f"{what}: plies per game"
    assert ep["res"].tolist() == [g["result"] for g in games], f"{what}: results"
    for key in REC_KEYS:
        exp = np.concatenate([g[key] for g in games])
        assert ep["rec"][key].shape == exp.shape and np.array_equal(ep["rec"][key], exp), f"{what}: {key} differ"
    assert ep["values"].dtype == np.float32 and np.array_equal(ep["values"], np.concatenate([g["values"] for g in games])), f"{what}: values"
    sims = np.concatenate([g["sims"] for g in games])
    assert ep["sims"].dtype == np.int32 and np.array_equal(ep["sims"], sims), f"{what}: sims"
    c, plies = ep["c"], len(sims)
    assert c["plies"] == c["records"] == c["root_evals"] == plies and c["games"] == len(games), f"{what}: plies"
    assert c["simulations"] == int(sims.sum()) == int(ep["sims"].sum()), f"{what}: simulations"


def assert_same(a, b, what):
    for key in REC_KEYS:
        assert np.array_equal(a["rec"][key], b["rec"][key]), f"{what}: {key}"
    for key in ("nply", "res", "values", "sims"):
        assert np.array_equal(a[key], b[key]), f"{what}: {key}"
    assert a["c"]["simulations"] == b["c"]["simulations"] and a["c"]["plies"] == b["c"]["plies"], f"{what}: counters"


def first_wave(G, slots, lanes):
    """game ids every lane holds after the first refill: an equal share of the games, as many as its slots take, in lane order"""
    per, share = (slots + lanes - 1) // lanes, (G + lanes - 1) // lanes
    out, nxt = [], 0
    for i in range(lanes):
        take = min(min(per, slots - i * per), share, G - nxt)
        out.append(list(range(nxt, nxt + take)))
        nxt += take
    return out


def assert_mixed(seed0, G, permille, plies, slots=None, lanes=1, lockstep=0):
    """both kinds of ply among plies 0 .. plies - 1 of the games; with `lockstep`, every lane's first wave of games -- which plays
    its first `lockstep` plies in lock step, before any game can end -- has a ply where some but not all of them are FULL"""
    t = full_table(seed0, G, plies, permille)
    assert t.any() and not t.all(), "the configuration does not mix FULL and FAST plies"
    if lockstep:
        for ids in first_wave(G, slots, lanes):
            n_full = t[ids][:, :lockstep].sum(axis=0)
            assert len(ids) > 1 and ((n_full > 0) & (n_full < len(ids))).any(), f"lane with games {ids} never sees 0 < n_full < active"


# ---------------------------------------------------------------------------------------------------------------------
# 1. mixed games against the oracle loop
# ---------------------------------------------------------------------------------------------------------------------
CFG5 = (5, 4, 24, 6, 16, 7, 250, "ckpt_saved")          # n, k, S, F, G, seed0, permille, tag


def test_symbols_and_5x5_mixed_games_on_six_slots_two_lanes():
    """16 games on 6 slots in 2 lanes of 3 (not a multiple of the 4 games per tree-step workgroup): slots < games, so refill and
    the full-first compaction run all the time.  A 5x5 game with 4 in a row cannot end before ply 6."""
    n, k, S, F, G, seed0, permille, tag = CFG5
    assert_mixed(seed0, G, permille, 5, slots=6, lanes=2, lockstep=5)
    t = full_table(seed0, G, 5, permille)
    assert int(t.sum()) == 21 and int(t[:, 0].sum()) == 4
    games = _ref(*CFG5)
    e = _engine(n, k, S, 6, tag, engines=2)
    assert e.lanes() == 2 and e.playout_cap() == dict(fast_sims=0, full=0.0, export_full_only=False)
    e.set_playout_cap(F, permille / 1000)
    assert e.playout_cap() == dict(fast_sims=F, full=0.25, export_full_only=True)
    ep = _episode(e, G, seed0)
    assert e.persistent() == 0
    assert_games(ep, games, "5x5")
    assert set(ep["sims"].tolist()) == {S, F} and len(set(ep["nply"].tolist())) > 1
    e.close()


@pytest.mark.parametrize("n,k,S,F,G,slots,seed0,cut,tag", [
    pytest.param(9, 5, 16, 4, 12, 8, 7200, 6, "seeded", id="9x9"),
    pytest.param(15, 5, 12, 3, 8, 8, 7300, 4, "seeded", id="15x15"),
    pytest.param(5, 4, 24, 6, 8, 4, 7400, 0, None, id="5x5-synthetic"),
    pytest.param(5, 4, 24, 6, 6, 4, 7500, 0, "resnet_ckpt", id="5x5-resnet"),
])
def test_mixed_games_on_every_size_and_evaluator(n, k, S, F, G, slots, seed0, cut, tag):
    assert_mixed(seed0, G, 250, cut or 5, slots=slots, lanes=1, lockstep=cut or 5)
    games = _ref(n, k, S, F, G, seed0, 250, tag, cut)
    e = _engine(n, k, S, slots, tag, engines=1)
    e.set_playout_cap(F, 0.25)
    ep = _episode(e, G, seed0, cut)
    assert_games(ep, games, f"{n}x{n} {tag}")
    assert e.persistent() == 0
    e.close()


@pytest.mark.parametrize("F", [1, 24])
def test_edge_budgets_one_simulation_and_as_many_as_a_full_ply(F):
    """F = 1: a FAST ply is the root evaluation and one simulation.  F = S: the capped game differs from the plain one only by
    the missing noise on its FAST plies, and `sims` cannot tell the two kinds apart."""
    n, k, S, G, seed0, tag = 5, 4, 24, 8, 7600, "ckpt_saved"
    assert_mixed(seed0, G, 500, 5, slots=4, lanes=1, lockstep=5)
    games = _ref(n, k, S, F, G, seed0, 500, tag)
    e = _engine(n, k, S, 4, tag)
    e.set_playout_cap(F, 0.5)
    ep = _episode(e, G, seed0)
    assert_games(ep, games, f"F = {F}")
    if F == S:
        plain = [orc.Oracle(n, k, S).selfplay_game(_weights(n, tag)[1], *orc.selfplay_tape(seed0 + g, n)) for g in range(G)]
        assert any(p["nply"] != g["nply"] or not np.array_equal(p["visits"], g["visits"]) for p, g in zip(plain, games)), "the noise made no difference"
        # ... but the export still goes by the hash: the records of the FULL plies
        assert e.export_count() == sum(int(np_full(seed0 + i, np.arange(g["nply"]), 500).sum()) for i, g in enumerate(games)) < ep["c"]["records"]
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the two end points
# ---------------------------------------------------------------------------------------------------------------------
def test_1000_permille_is_the_episode_with_the_cap_off():
    n, k, S, F, G, seed0, _, tag = CFG5
    e = _engine(n, k, S, 6, tag, engines=2)
    off = _episode(e, G, seed0)
    assert e.persistent() > 0 and (off["sims"] == S).all()
    e.set_playout_cap(F, 1.0)
    on = _episode(e, G, seed0)
    assert e.persistent() == 0
    assert_same(off, on, "1000 permille vs cap off")
    for key in ("expansions", "terminal_hits", "depth_sum", "root_evals", "records"):
        assert off["c"][key] == on["c"][key], key
    e.set_playout_cap(0)
    again = _episode(e, G, seed0)
    assert e.persistent() > 0
    assert_same(off, again, "cap switched off again")
    e.close()


def test_0_permille_plays_all_fast_games_without_a_second_phase():
    n, k, S, F, G, seed0, tag = 5, 4, 24, 6, 4, 7700, "ckpt_saved"
    games = _ref(n, k, S, F, G, seed0, 0, tag)
    e = _engine(n, k, S, G, tag, engines=1)
    e.set_playout_cap(F, 0.0)
    ep = _episode(e, G, seed0)
    assert_games(ep, games, "0 permille")
    assert (ep["sims"] == F).all() and e.export_count() == 0
    # one lane, as many slots as games: the lane plays max(nply) plies of 1 + F evaluation batches each, none of phase B
    assert ep["c"]["steps"] == int(ep["nply"].max()) * (1 + F)
    e.set_playout_cap(F, 1.0)
    assert _episode(e, G, seed0)["c"]["steps"] % (1 + S) == 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. search options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [7, 3])
def test_virtual_loss_batches_of_four(F):
    """F = 7: the second batch of a FAST search is a partial one (3 leaves); F = 3: fewer simulations than one batch"""
    n, k, S, G, seed0, tag = 5, 4, 24, 8, 7800, "ckpt_saved"
    assert_mixed(seed0, G, 250, 5, slots=4, lanes=1, lockstep=5)
    games = _ref(n, k, S, F, G, seed0, 250, tag, vl=4)
    e = _engine(n, k, S, 4, tag)
    e.set_virtual_loss(4)
    e.set_playout_cap(F, 0.25)
    ep = _episode(e, G, seed0)
    assert_games(ep, games, f"virtual loss, F = {F}")
    e.close()


def test_evaluation_cache_changes_nothing():
    n, k, S, F, G, seed0, permille, tag = CFG5
    games = _ref(*CFG5)
    e = _engine(n, k, S, 6, tag, engines=2)
    e.set_eval_cache(1 << 12)
    e.set_playout_cap(F, permille / 1000)
    ep = _episode(e, G, seed0)
    assert ep["c"]["cache_lookups"] > 0 and ep["c"]["cache_hits"] > 0
    assert_games(ep, games, "cache on")
    e.set_eval_cache(0)
    assert_same(ep, _episode(e, G, seed0), "cache off vs on")
    e.close()


def _independence(make, G, seed0, S, F, cut, what):
    """the oracle's single search cannot restate these: the 1000 permille end point, and a 250 permille episode that is the same
    on 6 slots in 2 lanes and on 4 slots in 1 lane (other slots, other lanes, other compaction and refill order)"""
    assert_mixed(seed0, G, 250, cut or 5)
    a = make(6, 2)
    off = _episode(a, G, seed0, cut)
    a.set_playout_cap(F, 1.0)
    assert_same(off, _episode(a, G, seed0, cut), f"{what}: 1000 permille vs cap off")
    a.set_playout_cap(F, 0.25)
    mixed = _episode(a, G, seed0, cut)
    a.close()
    assert set(mixed["sims"].tolist()) == {S, F} and mixed["c"]["simulations"] == int(mixed["sims"].sum())
    assert not np.array_equal(mixed["rec"]["visits"][:len(off["rec"]["visits"])], off["rec"]["visits"][:len(mixed["rec"]["visits"])])
    b = make(4, 1)
    b.set_playout_cap(F, 0.25)
    assert_same(mixed, _episode(b, G, seed0, cut), f"{what}: 6 slots in 2 lanes vs 4 slots in 1 lane")
    b.close()


def test_leaf_symmetry():
    n, k, S, F, tag = 5, 4, 24, 6, "ckpt_saved"

    def make(slots, lanes):
        e = _engine(n, k, S, slots, tag, engines=lanes)
        e.set_leaf_symmetry(True)
        return e
    _independence(make, 10, 7900, S, F, 0, "leaf symmetry")


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
def test_emulated_trunks(mode):
    n, k, S, F, tag = 9, 5, 16, 4, "seeded"

    def make(slots, lanes):
        e = _engine(n, k, S, slots, tag, engines=lanes)
        e.set_trunk_mode(mode)
        return e
    _independence(make, 8, 8000, S, F, 6, mode)


def test_deep_engine():
    n, k, S, F, G, seed0, cut = 5, 4, 1100, 30, 4, 8100, 3
    assert_mixed(seed0, G, 500, cut, slots=4, lanes=1, lockstep=cut)
    games = _ref(n, k, S, F, G, seed0, 500, None, cut)
    e = _engine(n, k, S, 4, None, deep=True, engines=1)
    e.set_playout_cap(F, 0.5)
    ep = _episode(e, G, seed0, cut)
    assert_games(ep, games, "deep")
    e.close()


def test_start_positions_fullness_goes_by_the_absolute_ply():
    """game g continued from ply 3 of the oracle-loop game g is the rest of that game"""
    n, k, S, F, G, seed0, permille, tag = CFG5
    games = _ref(*CFG5)[:6]
    assert all(g["nply"] > 4 for g in games)
    t = full_table(seed0, 6, 8, permille)
    assert not np.array_equal(t[:, 3:8], t[:, 0:5])          # a ply counted from the start position would be searched differently
    e = _engine(n, k, S, 4, tag, engines=1)
    e.set_start_positions(np.array([g["boards"][3] for g in games]), np.array([g["movers"][3] for g in games]),
                          np.array([g["lasts"][3] for g in games]))
    e.set_playout_cap(F, permille / 1000)
    ep = _episode(e, 6, seed0)
    rest = [dict(g, nply=g["nply"] - 3, **{key: g[key][3:] for key in REC_KEYS + ("values", "sims")}) for g in games]
    assert_games(ep, rest, "continued from ply 3")
    e.close()


def test_resignation_truncates_the_capped_game():
    n, k, S, F, G, seed0, permille, tag = CFG5
    games = _ref(*CFG5)
    values = [g["values"].astype(np.float64) for g in games]
    thr, crossing = choose_threshold(values)
    assert 1 <= len(crossing) < G
    want = []
    for g, v in zip(games, values):
        m = first_cross(v, thr)
        if m < 0 or (m == g["nply"] - 1 and g["result"] != 0):
            want.append(g)
            continue
        res = 3 - int(g["movers"][m])
        w = dict(g, nply=m + 1, result=res, **{key: g[key][:m + 1] for key in REC_KEYS + ("values", "sims")})
        w["z"] = _z(w["movers"], res)
        want.append(w)
    assert any(w["nply"] < g["nply"] for w, g in zip(want, games))
    e = _engine(n, k, S, 6, tag, engines=2)
    e.set_playout_cap(F, permille / 1000)
    e.set_resign(thr)
    ep = _episode(e, G, seed0)
    assert_games(ep, want, "resignation on")
    cross, _ = e.resign_info()
    assert cross.tolist() == [first_cross(v, thr) if first_cross(v, thr) < w["nply"] else -1 for v, w in zip(values, want)]
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. launch paths
# ---------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import test_playout_cap_gpu as t
n, k, S, F, G, seed0, permille, tag = t.CFG5
e = t._engine(n, k, S, 6, tag, engines=1)
e.set_playout_cap(F, permille / 1000)
ep = t._episode(e, G, seed0)
e.close()
out = dict(ep["rec"], steps=np.int64(ep["c"]["steps"]), simulations=np.int64(ep["c"]["simulations"]))
for key in ("nply", "res", "values", "sims"):
    out[key] = ep[key]
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("switch", ["AZ_COMPACT", "AZ_GRAPH"])
def test_environment_switch_in_a_fresh_process(switch, tmp_path):
    """AZ_COMPACT=0 (phase B runs over every slot and the budgets keep the FAST ones idle) and AZ_GRAPH=0, each in a process of
    its own, give the same games.  One lane, so that the games a ply holds do not depend on timing: the evaluation batches
    launched (a ply has a phase B when any of its games is FULL) are then the same with and without compaction."""
    n, k, S, F, G, seed0, permille, tag = CFG5
    games = _ref(*CFG5)
    e = _engine(n, k, S, 6, tag, engines=1)
    e.set_playout_cap(F, permille / 1000)
    here = _episode(e, G, seed0)
    e.close()
    assert_games(here, games, "in this process")
    path = str(tmp_path / "child.npz")
    env = {key: v for key, v in os.environ.items() if key not in ("AZ_COMPACT", "AZ_GRAPH", "AZ_PROFILE_EVENTS", "AZ_PERSIST")}
    env[switch] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(path)
    plies = sum(g["nply"] for g in games)
    ep = dict(rec={key: z[key] for key in REC_KEYS}, nply=z["nply"], res=z["res"], values=z["values"], sims=z["sims"],
              c=dict(plies=plies, records=plies, root_evals=plies, games=len(games), simulations=int(z["simulations"])))
    assert_games(ep, games, f"{switch}=0")
    assert int(z["steps"]) == here["c"]["steps"], f"{switch}=0: evaluation batches launched"
    assert (1 + F) * 25 < here["c"]["steps"] < (1 + S) * plies      # some plies without a phase B, none searched alone


def test_profiling_the_step_api_and_one_lane():
    n, k, S, F, G, seed0, permille, tag = CFG5
    games = _ref(*CFG5)
    e = _engine(n, k, S, 6, tag, engines=2)
    e.set_playout_cap(F, permille / 1000)
    e.set_profiling(True)
    ep = _episode(e, G, seed0)
    assert_games(ep, games, "profiled")
    assert ep["c"]["trunk_seconds"] > 0 and ep["c"]["step_seconds"] > 0 and ep["c"]["nn_seconds"] >= ep["c"]["trunk_seconds"]
    e.set_profiling(False)
    e.selfplay_begin(G, seed0=seed0)
    active, steps = 1, 0
    while active:
        active, _ = e.selfplay_step(1)
        steps += 1
    assert steps > max(g["nply"] for g in games)            # 16 games on 6 slots: more lane plies than the longest game has
    assert_games(_collect(e, e.selfplay_end()), games, "begin / step(1) / end")
    e.close()
    one = _engine(n, k, S, 6, tag, engines=1)
    one.set_playout_cap(F, permille / 1000)
    assert one.lanes() == 1
    assert_games(_episode(one, G, seed0), games, "one lane")
    one.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. export
# ---------------------------------------------------------------------------------------------------------------------
def _pack(e, count):
    rb = e.record_bytes
    dev = torch.full(((count + 2) * rb,), 0xAB, dtype=torch.uint8, device=DEV)
    val = torch.full((count + 2,), float("nan"), dtype=torch.float32, device=DEV)
    e.pack_into(dev.data_ptr())
    e.pack_values_into(val.data_ptr())
    torch.cuda.synchronize()
    host, hv = dev.cpu().numpy(), val.cpu().numpy()
    assert (host[count * rb:] == 0xAB).all() and np.isnan(hv[count:]).all(), "the export wrote past its count"
    return dev, host[:count * rb].reshape(count, rb), hv[:count]


def _examples(e, dev, count):
    n = e.n
    st = torch.empty((count * 8, 4, n, n), dtype=torch.float32, device=DEV)
    pi = torch.empty((count * 8, n, n), dtype=torch.float32, device=DEV)
    z = torch.empty(count * 8, dtype=torch.float32, device=DEV)
    e.examples_from_packed(dev.data_ptr(), count, 8, st.data_ptr(), pi.data_ptr(), z.data_ptr())
    torch.cuda.synchronize()
    return st.cpu().numpy().reshape(count, -1), pi.cpu().numpy().reshape(count, -1), z.cpu().numpy().reshape(count, -1)


def test_export_carries_the_full_records_only_when_asked():
    n, k, S, F, G, seed0, permille, tag = CFG5
    e = _engine(n, k, S, 6, tag, engines=2)
    e.set_playout_cap(F, permille / 1000, export_full_only=False)
    ep = _episode(e, G, seed0)
    R = ep["c"]["records"]
    mask = ep["sims"] == S
    assert 0 < mask.sum() < R and e.export_count() == R
    dev_all, rows_all, vals_all = _pack(e, R)
    assert np.array_equal(vals_all, ep["values"])
    ex_all = _examples(e, dev_all, R)
    e.set_playout_cap(F, permille / 1000, export_full_only=True)
    ep2 = _episode(e, G, seed0)
    assert_same(ep, ep2, "export_full_only changes no record")
    count = e.export_count()
    assert count == int(mask.sum())
    dev_full, rows_full, vals_full = _pack(e, count)
    assert np.array_equal(rows_full, rows_all[mask]) and np.array_equal(vals_full, vals_all[mask])
    for got, exp in zip(_examples(e, dev_full, count), ex_all):
        assert np.array_equal(got, exp[mask])
    e.set_playout_cap(0)
    off = _episode(e, G, seed0)
    assert e.export_count() == off["c"]["records"] and (off["sims"] == S).all()
    e.close()


def test_selfplay_manager_returns_the_examples_of_the_full_plies():
    from alphazero_piskvorky_amd import net
    from alphazero_piskvorky_amd.controller import NeuralNetworkController
    from alphazero_piskvorky_amd.self_play import SelfPlayManager, playout_cap_stats
    m = net.GomokuNet(board_size=5)
    m.load_state_dict({kk: torch.tensor(v) for kk, v in weights_from_fixture(5, "ckpt_saved").items()})
    ctl = NeuralNetworkController(m.eval(), device=DEV)
    params = {"num_simulations": 24, "c_puct": 2.0}
    every = SelfPlayManager(ctl, DEV, mcts_params=params, concurrent_games=4, seed=7,
                            playout_cap={"fast_sims": 6, "full": 0.25, "train_on_fast": True})
    all_ex = every.generate_self_play(8)
    sims = every._engine.sims()
    mask = sims == 24
    assert len(all_ex) == 4 * len(sims) and 0 < mask.sum() < len(sims)
    assert every.last_playout_cap_stats == playout_cap_stats(sims, mask)
    assert every.last_playout_cap_stats["full_records"] == int(mask.sum())
    mgr = SelfPlayManager(ctl, DEV, mcts_params=params, concurrent_games=4, seed=7, playout_cap={"fast_sims": 6, "full": 0.25})
    got = mgr.generate_self_play(8)
    exp = [all_ex[4 * r + a] for r in np.flatnonzero(mask) for a in range(4)]
    assert len(got) == len(exp) == 4 * int(mask.sum())
    for i, ((s1, p1, z1), (s2, p2, z2)) in enumerate(zip(got, exp)):
        assert torch.equal(s1, s2) and np.array_equal(p1, p2) and z1 == z2, f"example {i}"
    assert mgr.last_playout_cap_stats == every.last_playout_cap_stats
    # fast_sims = num_simulations: the statistics go by the hash like the export, not by the simulations
    mgr.playout_cap = {"fast_sims": 24, "full": 0.5}
    same = mgr.generate_self_play(8)
    st = mgr.last_playout_cap_stats
    assert (mgr._engine.sims() == 24).all() and st["mean_sims_per_ply"] == 24.0
    assert 0 < st["full_records"] < st["records"] and len(same) == 4 * st["full_records"] == 4 * mgr._engine.export_count()
    mgr.playout_cap = None
    plain = mgr.generate_self_play(8)
    assert mgr.last_playout_cap_stats is None and mgr._engine.playout_cap()["fast_sims"] == 0
    assert len(plain) == 4 * mgr._engine.last_records


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals and neighbours
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_keep_the_previous_setting():
    e = _engine(5, 4, 24, 4, None)
    e.set_playout_cap(6, 0.25)
    L = _capi.lib()
    for bad in ((25, 250, 1), (-1, 250, 1), (6, -1, 1), (6, 1001, 1), (6, 250, 2), (6, 250, -1)):
        assert L.az_set_playout_cap(e.h, *bad) == -1, bad
        assert e.playout_cap() == dict(fast_sims=6, full=0.25, export_full_only=True)
    assert L.az_set_playout_cap(e.h, 0, 5000, 7) == 0 and e.playout_cap()["fast_sims"] == 0      # off: the rest is ignored
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.sims()
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.export_count()
    e.selfplay_begin(2, seed0=1)
    with pytest.raises(az.AzError, match=r"\(-6\)"):
        e.set_playout_cap(6, 0.25)
    e.selfplay_step(1 << 20)
    e.selfplay_end()
    assert (e.sims() == 24).all() and e.export_count() == e.last_records
    e.close()


def test_reuse_and_the_external_evaluator_are_refused_in_either_order():
    n, S = 5, 24
    e = _engine(n, 4, S, 4, None)
    e.set_playout_cap(6, 0.25)
    with pytest.raises(az.AzError, match=r"\(-1\).*playout cap"):
        e.set_subtree_reuse(True)
    cap = e.ext_capacity()
    planes = torch.zeros((cap, 4, n, n), dtype=torch.float32, device=DEV)
    pol = torch.zeros((cap, n * n), dtype=torch.float32, device=DEV)
    val = torch.zeros(cap, dtype=torch.float32, device=DEV)
    with pytest.raises(az.AzError, match=r"\(-1\).*playout cap"):
        e.set_external_evaluator(planes.data_ptr(), pol.data_ptr(), val.data_ptr(), cap, lambda net, count: None)
    e.set_playout_cap(0)
    e.set_subtree_reuse(True)
    with pytest.raises(az.AzError, match=r"\(-1\).*playout cap"):
        e.set_playout_cap(6, 0.25)
    e.set_subtree_reuse(False)
    e.set_external_evaluator(planes.data_ptr(), pol.data_ptr(), val.data_ptr(), cap, lambda net, count: None)
    with pytest.raises(az.AzError, match=r"\(-1\).*playout cap"):
        e.set_playout_cap(6, 0.25)
    assert e.playout_cap()["fast_sims"] == 0
    e.clear_external_evaluator()
    e.set_playout_cap(6, 0.25)
    e.close()


def test_arena_and_search_batch_ignore_the_cap():
    n, k, S, tag = 5, 4, 24, "ckpt_saved"
    e = _engine(n, k, S, 6, tag)
    e.load_weights(weights_from_fixture(n, "ckpt_0802"), 1)
    games = _ref(*CFG5)
    boards = np.array([g["boards"][2] for g in games[:5]])
    players = np.array([g["movers"][2] for g in games[:5]])
    lasts = np.array([g["lasts"][2] for g in games[:5]])
    noise = [np.random.RandomState(40 + i).dirichlet([0.3] * (n * n - 2)) for i in range(5)]

    def both():
        return e.arena(6, seed0=31), e.search_batch(boards, players, lasts, 1.0, noise=noise)
    a0, s0 = both()
    e.set_playout_cap(6, 0.25)
    a1, s1 = both()
    for key in ("results", "actions", "nply"):
        assert np.array_equal(a0[key], a1[key]), key
    for key in ("action", "pi", "N", "W", "P"):
        assert np.array_equal(s0[key], s1[key]), key
    assert (s1["N"].sum(axis=1) == S).all()
    e.close()
