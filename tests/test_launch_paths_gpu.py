"""How a ply gets onto the GPU (host-side sequencing in csrc/az_engine.hip, k_refill in csrc/az_tree.h), against the oracle:

A. lanes wider than one k_refill chunk of 1024 slots (the second trip through its claim loop and its compaction loop);
B. the three ways lane_plies launches a ply -- replayed graph, kernel by kernel (AZ_GRAPH=0), kernel by kernel with HIP
   events (az_set_profiling / AZ_PROFILE_EVENTS=1) -- on one episode, and the timing fields the events feed;
C. one engine walked through every mode setter and back, against a fresh engine per mode: the graph cache (ply_graph keys
   its graphs by the whole LaunchCtx) must never replay the previous mode's kernel sequence;
E. one engine through the delta switch, its tile threshold, an option the delta path does not serve and a net_eval_delta call
   (csrc/az_delta.h), against a fresh engine per configuration.  B and C hold a 15x15 entry too, whose plies launch
   k_trunk_base / k_trunk_delta / k_trunk_rest, with delta_stats equal on every launch path and lane count.

Records go by game id and games are seeded per id, so every layout, launch path and mode history must give identical
episodes; every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.util import weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.weights import synthetic_state_dict

WORK = ("games", "plies", "simulations", "expansions", "terminal_hits", "depth_sum")
ORACLE_KEYS = ("actions", "boards", "visits", "pis", "z")
SWITCHES = ("AZ_GRAPH", "AZ_PROFILE_EVENTS", "AZ_STREAM_PRIORITY", "AZ_HOST_THREADS", "AZ_TAPE_THREADS", "AZ_PERSIST", "AZ_COMPACT")

_ORACLE = {}         # oracle games, computed once and shared by the cases that need them


def _clean_env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        if value is not None:
            monkeypatch.setenv(name, value)


def _episode(e, G, seed0, cut=0):
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    nply, res = e.games()
    return dict(rec=e.records(), nply=nply, res=res, c=c)


def _assert_same_episode(a, b, what, counters=WORK):
    for key in a["rec"]:
        assert np.array_equal(a["rec"][key], b["rec"][key]), f"{what}: {key}"
    assert np.array_equal(a["nply"], b["nply"]), f"{what}: nply"
    assert np.array_equal(a["res"], b["res"]), f"{what}: result"
    for key in counters:
        assert a["c"][key] == b["c"][key], f"{what}: counter {key}: {a['c'][key]} != {b['c'][key]}"


def _assert_same_arena(a, b, what):
    for key in ("actions", "results", "nply"):
        assert np.array_equal(a[key], b[key]), f"{what}: arena {key}"
    for key in ("wins", "losses", "draws", "total"):
        assert a[key] == b[key], f"{what}: arena {key}"


def _oracle_games(tag, o, onet, n, seed0, ids, cut=0):
    """oracle self-play games by id, computed once per (tag, id)"""
    out = {}
    for g in ids:
        if (tag, g) not in _ORACLE:
            noise, us = orc.selfplay_tape(seed0 + g, n, maxply=cut or None)
            _ORACLE[(tag, g)] = o.selfplay_game(onet, noise, us, maxply=cut or None, game=seed0 + g)
        out[g] = _ORACLE[(tag, g)]
    return out


def _assert_oracle_games(ep, ref, what):
    starts = np.concatenate([[0], np.cumsum(ep["nply"])])
    for g, r in ref.items():
        sl = slice(int(starts[g]), int(starts[g + 1]))
        assert int(ep["nply"][g]) == r["nply"], f"{what}: game {g}: nply"
        assert int(ep["res"][g]) == r["result"], f"{what}: game {g}: result"
        for key in ORACLE_KEYS:
            assert np.array_equal(ep["rec"][key][sl], r[key]), f"{what}: game {g}: {key} differs from the oracle"


def _oracle_arena(tag, o, oc, ob, n, seed0, ids, key0=None):
    out = {}
    for g in ids:
        if (tag, g) not in _ORACLE:
            us = np.random.RandomState(seed0 + g).random_sample(n * n)
            _ORACLE[(tag, g)] = o.arena_game(oc, ob, g, us, key=None if key0 is None else key0 + g)
        out[g] = _ORACLE[(tag, g)]
    return out


def _assert_oracle_arena(a, ref, what):
    for g, r in ref.items():
        assert int(a["nply"][g]) == r["nply"] and int(a["results"][g]) == r["result"], f"{what}: arena game {g}"
        assert np.array_equal(a["actions"][g][:r["nply"]], r["actions"]), f"{what}: arena game {g}: actions"
        assert (a["actions"][g][r["nply"]:] == -1).all()


def _assert_every_game_played_once(ep, G, S):
    """Counter identities, not a list of claims: every id of [0, G) has plies (a dropped claim leaves nply 0), and the simulations
    the kernels counted slot by slot are exactly S per recorded ply (a game claimed by two slots is searched twice and recorded
    once, so it shows here as long as both copies run)."""
    assert len(ep["nply"]) == G and (ep["nply"] > 0).all()
    assert ep["c"]["games"] == G
    assert ep["c"]["plies"] == int(ep["nply"].sum()) == len(ep["rec"]["actions"])
    assert ep["c"]["simulations"] == S * ep["c"]["plies"]
    assert ep["c"]["expansions"] + ep["c"]["terminal_hits"] == ep["c"]["simulations"]
    assert ((ep["res"] >= 1) & (ep["res"] <= 3)).all()


# ------------------------------------------------------------------------------------------------
# A. lanes wider than one k_refill chunk
# ------------------------------------------------------------------------------------------------
PERSIST = [pytest.param("0", id="lockstep"), pytest.param(None, id="persistent")]


def _wide_run(monkeypatch, persist, n, k, S, slots, engines, G, seed0, lanes, compact=None, sd=None):
    _clean_env(monkeypatch, AZ_PERSIST=persist, AZ_COMPACT=compact)
    e = az.Engine(n, k, S, slots, engines=engines, synthetic=sd is None, log_table=orc.numpy_log_table(S))
    assert e.lanes() == lanes
    if lanes == 1:
        assert slots > 1024 or slots in (1023, 1024)       # the lane under test: its width is the subject
    if sd is not None:
        e.load_weights(sd, 0)
    ep = _episode(e, G, seed0)
    assert e.persistent() == (0 if persist == "0" else 2)
    e.close()
    return ep


@pytest.mark.parametrize("persist", PERSIST)
def test_lane_of_three_refill_chunks_gives_the_single_chunk_episode(monkeypatch, persist):
    """3x3, 2500 slots in ONE lane: k_refill walks chunks of 1024, 1024 and 452 slots.  6000 games: every chunk claims ids again
    and again, the queue runs dry in the middle of a chunk, and compaction moves slots across both chunk boundaries.  Equal to
    the same episode on three lanes of 834 slots (the single-chunk path), to the wide lane without compaction, and to the
    oracle game by game at the chunk-boundary ids."""
    n, k, S, slots, G, seed0 = 3, 3, 8, 2500, 6000, 4100
    assert slots > 1024
    wide = _wide_run(monkeypatch, persist, n, k, S, slots, 1, G, seed0, lanes=1)
    _assert_every_game_played_once(wide, G, S)
    three = _wide_run(monkeypatch, persist, n, k, S, slots, 3, G, seed0, lanes=3)
    _assert_same_episode(wide, three, "one lane of 2500 slots vs three lanes of 834")
    flat = _wide_run(monkeypatch, persist, n, k, S, slots, 1, G, seed0, lanes=1, compact="0")
    _assert_same_episode(wide, flat, "compacted vs AZ_COMPACT=0")
    assert len(set(wide["nply"].tolist())) > 2              # games of different lengths: slots emptied at different plies
    ids = [0, 1023, 1024, 2047, 2048, 2499, 2500, 3523, 5999]
    ids += [int(g) for g in np.random.RandomState(0).randint(0, G, 40)]
    ref = _oracle_games("A1", orc.Oracle(n, k, S, synthetic=True), None, n, seed0, sorted(set(ids)))
    _assert_oracle_games(wide, ref, "wide lane")


@pytest.mark.parametrize("persist", PERSIST)
@pytest.mark.parametrize("slots", [1023, 1024, 1025])
def test_lane_at_the_chunk_boundary(monkeypatch, persist, slots):
    """A partial single chunk, exactly one chunk, and the smallest lane with a second chunk (one slot in it)."""
    n, k, S, seed0 = 3, 3, 8, 4100
    G = 2 * slots + 3
    wide = _wide_run(monkeypatch, persist, n, k, S, slots, 1, G, seed0, lanes=1)
    _assert_every_game_played_once(wide, G, S)
    two = _wide_run(monkeypatch, persist, n, k, S, slots, 2, G, seed0, lanes=2)
    _assert_same_episode(wide, two, f"one lane of {slots} slots vs two lanes")
    ids = sorted({0, 1022, 1023, 1024, slots - 1, slots, slots + 1, 2 * slots - 1, 2 * slots, G - 1})
    ref = _oracle_games("A1", orc.Oracle(n, k, S, synthetic=True), None, n, seed0, ids)      # same seeds as the 2500-slot case
    _assert_oracle_games(wide, ref, f"{slots} slots")


@pytest.mark.parametrize("persist", PERSIST)
def test_wide_lane_with_the_net_5x5(monkeypatch, persist):
    """5x5 / 4 with the net evaluator, 1100 slots and the lane count left to the library (one lane up to 5x5): complete games
    with one refill round, against two lanes of 550 and against the oracle."""
    n, k, S, slots, G, seed0 = 5, 4, 12, 1100, 2300, 5200
    assert slots > 1024
    sd = synthetic_state_dict(n)
    wide = _wide_run(monkeypatch, persist, n, k, S, slots, 0, G, seed0, lanes=1, sd=sd)
    _assert_every_game_played_once(wide, G, S)
    two = _wide_run(monkeypatch, persist, n, k, S, slots, 2, G, seed0, lanes=2, sd=sd)
    _assert_same_episode(wide, two, "one lane of 1100 slots vs two lanes of 550")
    ids = [0, 1, 1023, 1024, 1025, 1099, 1100, 1101, 2123, 2124, 2200, 2299]
    ref = _oracle_games("A2", orc.Oracle(n, k, S), orc.Net(n, sd), n, seed0, ids)
    _assert_oracle_games(wide, ref, "wide lane")


@pytest.mark.parametrize("persist", PERSIST)
def test_arena_on_a_wide_lane(monkeypatch, persist):
    """k_refill's side assignment (odd game ids start with the baseline) in a second chunk: 1500 arena games on one lane of
    1100 slots against two lanes of 550, and against the oracle at the chunk boundary and the first refilled ids."""
    n, k, S, slots, G, seed0 = 3, 3, 4, 1100, 1500, 66
    cand, base = synthetic_state_dict(n, seed=0), synthetic_state_dict(n, seed=7)
    out = []
    for engines in (1, 2):
        _clean_env(monkeypatch, AZ_PERSIST=persist)
        e = az.Engine(n, k, S, slots, engines=engines, log_table=orc.numpy_log_table(S))
        assert e.lanes() == engines and slots > 1024
        e.load_weights(cand, 0); e.load_weights(base, 1)
        out.append(e.arena(G, seed0=seed0, temperature_table=orc.arena_T_table(n * n)))
        assert e.persistent() == (0 if persist == "0" else 1)
        e.close()
    _assert_same_arena(out[0], out[1], "one lane of 1100 slots vs two lanes of 550")
    assert (out[0]["nply"] > 0).all() and out[0]["total"] == G
    ids = [0, 1, 1022, 1023, 1024, 1025, 1098, 1099, 1100, 1101, 1498, 1499]
    ref = _oracle_arena("A3", orc.Oracle(n, k, S), orc.Net(n, cand), orc.Net(n, base), n, seed0, ids)
    _assert_oracle_arena(out[0], ref, "wide lane")


# ------------------------------------------------------------------------------------------------
# B. graph replay, eager, profiled: one episode
# ------------------------------------------------------------------------------------------------
LAUNCH_COUNTERS = WORK + ("trunk_launches", "trunk_boards", "steps", "duplicate_leaves", "cache_lookups", "cache_hits")
B_CONFIGS = {
    "lockstep": dict(n=9, k=5, S=12, slots=12, engines=3, G=20, cut=6),
    "virtual_loss": dict(n=9, k=5, S=12, slots=12, engines=3, G=20, cut=6, vl=4),
    "eval_cache": dict(n=9, k=5, S=12, slots=12, engines=3, G=20, cut=6, cache=1024),
    "eval_cache_one_slot": dict(n=9, k=5, S=12, slots=1, engines=1, G=4, cut=6, cache=1024, oracle="B-9x9"),
    "eval_cache_one_slot_persistent": dict(n=5, k=4, S=30, slots=1, engines=0, G=3, cut=0, cache=1024, oracle="B-persistent"),
    "persistent": dict(n=5, k=4, S=30, slots=7, engines=0, G=15, cut=0),
    "arena": dict(n=9, k=5, S=12, slots=6, engines=3, arena=6),
    # 15x15, the plain net: the plies launch k_trunk_base once and k_trunk_delta / k_trunk_rest for every batch (csrc/az_delta.h)
    "delta_15x15": dict(n=15, k=5, S=12, slots=6, engines=3, G=8, cut=3, delta=True),
}
B_SEED = 2024
# cache_hits (and trunk_boards, which subtracts it) are a function of the episode only where one position is looked up or written
# per launch: the cache is direct-mapped and shared by every slot of every lane, two positions that map to one entry are written
# by concurrent workgroups of one launch (the later write, or neither when the entry is torn, survives), and lanes on their own
# host threads interleave freely.  Measured on the twelve-slot shape on ONE lane: 180 hits of 1560 lookups on the replayed
# graph, 179 kernel by kernel.  So the one-slot shapes (one game, one evaluation item per launch, lock-step and persistent)
# compare every cache counter exactly across the four launch paths -- a stale cache_gen, cache_mask or cache pointer on one path
# changes hits and nothing else -- and the twelve-slot shape compares everything but these two, which it bounds.
CACHE_ORDER_COUNTERS = ("cache_hits", "trunk_boards")


def _b_weights(cfg):
    n = cfg["n"]
    return (weights_from_fixture(5, "ckpt_saved") if n == 5 else weights_from_fixture(n, "seeded")), synthetic_state_dict(n, seed=7)


def _b_engine(cfg):
    e = az.Engine(cfg["n"], cfg["k"], cfg["S"], cfg["slots"], engines=cfg["engines"], log_table=orc.numpy_log_table(cfg["S"]))
    sd, sd2 = _b_weights(cfg)
    e.load_weights(sd, 0)
    if "arena" in cfg:
        e.load_weights(sd2, 1)
    if "vl" in cfg:
        e.set_virtual_loss(cfg["vl"])
    if "cache" in cfg:
        e.set_eval_cache(cfg["cache"])
    return e


def _b_play(e, cfg):
    """one episode of the configuration -> (episode or None, arena or None, counters)"""
    if "arena" in cfg:
        a = e.arena(cfg["arena"], seed0=B_SEED, temperature_table=orc.arena_T_table(cfg["n"] ** 2))
        return None, a, e.counters()
    assert cfg["G"] >= cfg["slots"]                 # the first plies run the full grid: the default run replays a graph
    ep = _episode(e, cfg["G"], B_SEED, cfg["cut"])
    return ep, None, ep["c"]


def _b_batches(cfg):
    return 1 + -(-cfg["S"] // cfg.get("vl", 1))


def _assert_b_path(cfg, e, c, profiled):
    """what shows which way the ply went: lock-step = one trunk launch per net and evaluation batch, persistent = one launch
    per ply; events = the seconds"""
    nnets = 2 if "arena" in cfg else 1
    persistent = cfg["n"] <= 5
    assert c["steps"] > 0 and c["steps"] % _b_batches(cfg) == 0
    if persistent:
        assert e.persistent() == 2 and c["trunk_launches"] * _b_batches(cfg) == c["steps"]
    else:
        assert e.persistent() == 0 and c["trunk_launches"] == nnets * c["steps"]
    if not profiled:
        assert c["trunk_seconds"] == 0.0 and c["nn_seconds"] == 0.0 and c["step_seconds"] == 0.0
    elif persistent:
        assert c["trunk_seconds"] > 0          # events 0..1 wrap the whole search; 1..3 are recorded back to back
    else:
        assert 0 < c["trunk_seconds"] <= c["nn_seconds"] and c["step_seconds"] > 0
        assert c["nn_seconds"] + c["step_seconds"] <= c["seconds"]      # inside the wall time: the lanes ran one after another


def _assert_b_same(ref, got, what, counters=LAUNCH_COUNTERS):
    if ref[0] is not None:
        _assert_same_episode(ref[0], got[0], what, counters=())
    else:
        _assert_same_arena(ref[1], got[1], what)
    for key in counters:
        assert ref[2][key] == got[2][key], f"{what}: counter {key}: {ref[2][key]} != {got[2][key]}"


@pytest.mark.parametrize("name", list(B_CONFIGS))
def test_graph_eager_and_profiled_plies_give_one_episode(monkeypatch, name):
    cfg = B_CONFIGS[name]
    n, k, S = cfg["n"], cfg["k"], cfg["S"]
    runs, delta = {}, {}
    for variant, env in (("graph", {}), ("eager", dict(AZ_GRAPH="0")), ("set_profiling", {}), ("env_profiled", dict(AZ_PROFILE_EVENTS="1"))):
        _clean_env(monkeypatch, **env)
        e = _b_engine(cfg)
        if variant == "set_profiling":
            e.set_profiling(True)
        profiled = variant in ("set_profiling", "env_profiled")
        runs[variant] = _b_play(e, cfg)
        delta[variant] = e.delta_stats(by_tiles=True)
        _assert_b_path(cfg, e, runs[variant][2], profiled)
        if variant == "set_profiling":          # and off again: zeros, same records
            e.set_profiling(False)
            again = _b_play(e, cfg)
            _assert_b_path(cfg, e, again[2], False)
            _assert_b_same(runs[variant], again, "after set_profiling(False)", counters=WORK + ("trunk_launches", "steps"))   # (a warm cache hits more)
        e.close()
    racy = "cache" in cfg and cfg["slots"] > 1
    counters = tuple(key for key in LAUNCH_COUNTERS if not (racy and key in CACHE_ORDER_COUNTERS))
    for variant in ("eager", "set_profiling", "env_profiled"):
        _assert_b_same(runs["graph"], runs[variant], f"{name}: graph vs {variant}", counters=counters)
    for c in (run[2] for run in runs.values()):
        assert c["trunk_boards"] == c["expansions"] + c["root_evals"] - c["cache_hits"]
        if "cache" in cfg:
            assert 0 < c["cache_hits"] < c["cache_lookups"]
        else:
            assert c["cache_lookups"] == c["cache_hits"] == 0
    sd, sd2 = _b_weights(cfg)
    o = orc.Oracle(n, k, S, virtual_loss=cfg.get("vl", 0))
    if "arena" in cfg:
        ref = _oracle_arena("B-" + name, o, orc.Net(n, sd), orc.Net(n, sd2), n, B_SEED, range(cfg["arena"]))
        _assert_oracle_arena(runs["graph"][1], ref, name)
    else:
        tag = cfg.get("oracle") or ("B-9x9" if name in ("lockstep", "eval_cache") else "B-" + name)       # the cache and the slot count change no result
        ref = _oracle_games(tag, o, orc.Net(n, sd), n, B_SEED, range(cfg["G"]), cut=cfg["cut"])
        _assert_oracle_games(runs["graph"][0], ref, name)
    if cfg.get("delta"):
        # the same episode on one lane of six slots: every lane count owns its base activations, flags and counters
        _clean_env(monkeypatch)
        e = _b_engine(dict(cfg, engines=1))
        assert e.lanes() == 1
        runs["one lane"] = _b_play(e, cfg)
        delta["one lane"] = e.delta_stats(by_tiles=True)
        e.close()
        _assert_b_same(runs["graph"], runs["one lane"], f"{name}: three lanes vs one", counters=WORK + ("trunk_boards",))
        c = runs["graph"][2]
        assert delta["graph"]["delta"] > 0 and delta["graph"]["delta"] + delta["graph"]["full"] == c["trunk_boards"]
        assert delta["graph"]["base"] == 2 * c["plies"]
        for variant, st in delta.items():
            assert st == delta["graph"], f"{name}: delta_stats: graph vs {variant}"
    else:
        assert all(st == dict(delta=0, full=0, tiles=0, base=0, by_tiles=[0] * 16) for st in delta.values())


def test_stream_priority_and_host_thread_switches_keep_the_records(monkeypatch):
    cfg = B_CONFIGS["lockstep"]
    _clean_env(monkeypatch)
    e = _b_engine(cfg)
    want = _b_play(e, cfg)
    e.close()
    _clean_env(monkeypatch, AZ_STREAM_PRIORITY="0", AZ_HOST_THREADS="1", AZ_TAPE_THREADS="1")
    e = _b_engine(cfg)
    got = _b_play(e, cfg)
    _assert_b_path(cfg, e, got[2], False)
    e.close()
    _assert_b_same(want, got, "AZ_STREAM_PRIORITY=0 AZ_HOST_THREADS=1 AZ_TAPE_THREADS=1")
    assert got[2]["tape_threads"] == 1
    ref = _oracle_games("B-9x9", orc.Oracle(cfg["n"], cfg["k"], cfg["S"]), orc.Net(cfg["n"], _b_weights(cfg)[0]), cfg["n"], B_SEED,
                        range(cfg["G"]), cut=cfg["cut"])
    _assert_oracle_games(got[0], ref, "switches")


# ------------------------------------------------------------------------------------------------
# C. one engine through the modes and back
# ------------------------------------------------------------------------------------------------
C_CONFIGS = {
    "9x9": dict(n=9, k=5, S=16, slots=8, engines=2, G=8, cut=5),
    "5x5": dict(n=5, k=4, S=24, slots=6, engines=0, G=6, cut=0),
    # 15x15, the plain net: the default mode and every mode switched off again evaluate leaves as deltas (csrc/az_delta.h); one
    # arena game, which runs to its end on a board of 225 cells
    "15x15": dict(n=15, k=5, S=12, slots=6, engines=3, G=6, cut=3, arena=1, delta=True),
}
C_SEED = 7300
DEFAULT_MODE = dict(w0="first", w1=None, cache=0, vl=1, leaf_sym=False, trunk="f32", reuse=False)


def _c_weights(cfg):
    n = cfg["n"]
    first = weights_from_fixture(5, "ckpt_saved") if n == 5 else weights_from_fixture(n, "seeded")
    second = weights_from_fixture(5, "ckpt_0802") if n == 5 else synthetic_state_dict(n, seed=7)
    return dict(first=first, second=second)


def _c_fresh(cfg, mode, weights):
    """an engine created directly in `mode`"""
    e = az.Engine(cfg["n"], cfg["k"], cfg["S"], cfg["slots"], engines=cfg["engines"], log_table=orc.numpy_log_table(cfg["S"]))
    e.load_weights(weights[mode["w0"]], 0)
    if mode["w1"]:
        e.load_weights(weights[mode["w1"]], 1)
    if mode["cache"]:
        e.set_eval_cache(mode["cache"])
    if mode["vl"] > 1:
        e.set_virtual_loss(mode["vl"])
    if mode["leaf_sym"]:
        e.set_leaf_symmetry(True)
    if mode["trunk"] != "f32":
        e.set_trunk_mode(mode["trunk"])
    if mode["reuse"]:
        e.set_subtree_reuse(True)
    return e


def _c_oracle(cfg, mode):
    return orc.Oracle(cfg["n"], cfg["k"], cfg["S"], reuse=mode["reuse"], virtual_loss=mode["vl"] if mode["vl"] > 1 else 0,
                      leaf_sym=mode["leaf_sym"])


def _c_position(cfg):
    n = cfg["n"]
    board = np.zeros(n * n, np.uint8)
    board[n + 1] = 1; board[2 * n + 2] = 2; board[n + 2] = 1
    noise = np.random.RandomState(3).dirichlet([0.3] * (n * n - 3))
    return board, 2, n + 2, 0.6, noise, 0.81


def _c_boards(cfg):
    n, rs = cfg["n"], np.random.RandomState(17)
    cnt = cfg["slots"] + 3                        # more boards than slots: a second pass with a ragged tail
    boards = np.zeros((cnt, n * n), np.uint8); players = np.zeros(cnt, np.uint8); lasts = np.full(cnt, -1, np.int16)
    for i in range(cnt):
        m = int(rs.randint(0, n * n // 2))
        cells = rs.permutation(n * n)[:m]
        for j, cell in enumerate(cells):
            boards[i, cell] = 1 + (j % 2)
        players[i] = 1 + (m % 2)
        lasts[i] = cells[-1] if m else -1
    return boards, players, lasts


@pytest.mark.parametrize("name", list(C_CONFIGS))
def test_one_engine_through_the_modes_and_back(monkeypatch, name):
    """After every setter the kept engine's episode must be that of an engine created directly in the mode (a stale graph
    would replay the previous mode's kernels or buffers), and the oracle's where the oracle restates the mode."""
    _clean_env(monkeypatch)
    cfg = C_CONFIGS[name]
    n, k, S, G, cut = cfg["n"], cfg["k"], cfg["S"], cfg["G"], cfg["cut"]
    weights = _c_weights(cfg)
    onets = {tag: orc.Net(n, sd) for tag, sd in weights.items()}
    mode = dict(DEFAULT_MODE)
    kept = _c_fresh(cfg, mode, weights)
    assert kept.lanes() == (cfg["engines"] or 1)
    episodes = []

    def check(step):
        ep = _episode(kept, G, C_SEED, cut)
        lockstep = n > 7 or mode["vl"] > 1 or mode["trunk"] != "f32"
        assert (kept.persistent() == 0) == lockstep, step
        fresh = _c_fresh(cfg, mode, weights)
        want = _episode(fresh, G, C_SEED, cut)
        want_delta = fresh.delta_stats(by_tiles=True)
        fresh.close()
        _assert_same_episode(want, ep, f"{name}: {step}: fresh engine vs kept engine", counters=WORK + ("trunk_launches", "steps", "duplicate_leaves"))
        # delta evaluation: in the modes it serves, counted from zero in every episode; nothing of it in the others
        st = kept.delta_stats(by_tiles=True)
        if cfg.get("delta") and mode["vl"] == 1 and not mode["leaf_sym"] and mode["trunk"] == "f32" and not mode["reuse"]:
            assert st["delta"] > 0 and st["base"] == 2 * ep["c"]["plies"] and st["delta"] + st["full"] == ep["c"]["trunk_boards"], step
            assert sum(st["by_tiles"]) == st["delta"] and sum(t * x for t, x in enumerate(st["by_tiles"])) == st["tiles"], step
            if not mode["cache"]:              # (with the cache the evaluations left over depend on the order of its writes: CACHE_ORDER_COUNTERS)
                assert st == want_delta, f"{name}: {step}: delta_stats: fresh engine vs kept engine"
        else:
            assert st == want_delta == dict(delta=0, full=0, tiles=0, base=0, by_tiles=[0] * 16), step
        if mode["trunk"] == "f32":
            tag = ("C", name, mode["w0"], mode["vl"], mode["leaf_sym"], mode["reuse"])
            ref = _oracle_games(tag, _c_oracle(cfg, mode), onets[mode["w0"]], n, C_SEED, range(G), cut=cut)
            _assert_oracle_games(ep, ref, f"{name}: {step}")
        episodes.append(ep)

    check("default")
    kept.set_eval_cache(2048); mode["cache"] = 2048
    check("set_eval_cache(2048)")
    kept.load_weights(weights["second"], 0); mode["w0"] = "second"
    check("load_weights(second, 0)")
    kept.set_virtual_loss(4); mode["vl"] = 4
    check("set_virtual_loss(4)")
    kept.set_virtual_loss(1); mode["vl"] = 1
    check("set_virtual_loss(1)")
    kept.set_leaf_symmetry(True); mode["leaf_sym"] = True
    check("set_leaf_symmetry(True)")
    kept.set_leaf_symmetry(False); mode["leaf_sym"] = False
    check("set_leaf_symmetry(False)")
    kept.set_trunk_mode("bf16x3"); mode["trunk"] = "bf16x3"
    check("set_trunk_mode(bf16x3)")
    kept.set_trunk_mode("f32"); mode["trunk"] = "f32"
    check("set_trunk_mode(f32)")
    kept.set_subtree_reuse(True); mode["reuse"] = True
    check("set_subtree_reuse(True)")
    kept.set_subtree_reuse(False); mode["reuse"] = False
    check("set_subtree_reuse(False)")
    kept.set_eval_cache(0); mode["cache"] = 0
    check("set_eval_cache(0)")
    for step in (2, 4, 6, 8, 10, 11):           # every mode that was switched off again left the episode of step 2
        _assert_same_episode(episodes[2], episodes[step], f"{name}: episode {step} vs episode 2")

    # the arena, one search and one net evaluation on the kept engine, against a fresh engine and the oracle
    kept.load_weights(weights["first"], 1); mode["w1"] = "first"
    fresh = _c_fresh(cfg, mode, weights)
    o = _c_oracle(cfg, mode)
    T = orc.arena_T_table(n * n)
    A = cfg.get("arena", 4)
    a, fa = kept.arena(A, seed0=C_SEED, temperature_table=T), fresh.arena(A, seed0=C_SEED, temperature_table=T)
    _assert_same_arena(fa, a, f"{name}: arena")
    _assert_oracle_arena(a, _oracle_arena(("C-arena", name), o, onets["second"], onets["first"], n, C_SEED, range(A)), f"{name}: arena")
    board, pl, last, temp, noise, u = _c_position(cfg)
    for slot, tag in ((0, "second"), (1, "first")):
        r, fr = kept.search(board, pl, last, temp, noise, u, slot=slot), fresh.search(board, pl, last, temp, noise, u, slot=slot)
        ro = o.search(onets[tag], board, pl, last, temp, noise, u)
        for other, what in ((fr, "fresh engine"), (ro, "oracle")):
            for key in ("N", "W", "P", "pi"):
                assert np.array_equal(r[key], other[key]), f"{name}: search with slot {slot} vs {what}: {key}"
            assert r["action"] == other["action"]
    boards, players, lasts = _c_boards(cfg)
    got, want = kept.net_eval(boards, players, lasts), fresh.net_eval(boards, players, lasts)
    for x, y in zip(got, want):
        assert np.array_equal(x, y), f"{name}: net_eval vs fresh engine"
    for i in range(len(players)):
        ol, oP, ov = onets["second"].eval(o.encode(boards[i], int(players[i]), int(lasts[i])))
        assert np.array_equal(got[0][i], ol) and np.array_equal(got[1][i], oP) and got[2][i] == np.float32(ov), f"{name}: net_eval board {i}"
    fresh.close()

    kept.load_weights(weights["first"], 0); mode["w0"] = "first"
    check("reload of the first weights")
    check("default again")
    kept.close()
    _assert_same_episode(episodes[0], episodes[-2], f"{name}: after the reload vs the first episode")
    _assert_same_episode(episodes[0], episodes[-1], f"{name}: last episode vs the first")


def _d_positions(n):
    """three undecided positions: the empty board, three stones, four stones"""
    boards = np.zeros((3, n * n), np.uint8)
    boards[1, [n + 1, n + 2]] = 1; boards[1, 2 * n + 2] = 2
    boards[2, [2 * n + 2, 2 * n + 3]] = 1; boards[2, [n + 1, 3 * n + 3]] = 2
    players, lasts = np.array([1, 2, 1], np.uint8), np.array([-1, n + 2, 3 * n + 3], np.int16)
    rs = np.random.RandomState(29)
    noise = [rs.dirichlet([0.3] * int((b == 0).sum())) for b in boards]
    return boards, players, lasts, noise, rs.random_sample(3), np.array([1.0, 0.6, 0.05])


def _d_searches(e, n):
    """every search entry point on the fixed positions -> {what: result}"""
    from tests.ties import levels_of
    boards, players, lasts, noise, us, Ts = _d_positions(n)
    lv = np.exp(levels_of("three", n).astype(np.float64))
    table, v = (lv / lv.sum()).astype(np.float32), float(np.tanh(-0.5))       # the constant evaluator of tests/test_ties_gpu.py
    out = {}
    for slot in (0, 1):
        for i in range(3):
            out[f"search {i} slot {slot}"] = e.search(boards[i], int(players[i]), int(lasts[i]), Ts[i], noise[i], us[i], slot=slot)
            out[f"batch of one {i} slot {slot}"] = e.search_batch(boards[i:i + 1], players[i:i + 1], lasts[i:i + 1], Ts[i:i + 1], noise[i:i + 1], us[i:i + 1], slot=slot)
        out[f"batch of three slot {slot}"] = e.search_batch(boards, players, lasts, Ts, noise, us, slot=slot)
        out[f"batch of three without noise slot {slot}"] = e.search_batch(boards, players, lasts, Ts, None, us, slot=slot)
    for i in range(3):
        out[f"callback {i}"] = e.search_callback(boards[i], int(players[i]), int(lasts[i]), Ts[i], lambda cells, pl, la: (table, v), noise[i], us[i])
        out[f"callback {i} without noise"] = e.search_callback(boards[i], int(players[i]), int(lasts[i]), Ts[i], lambda cells, pl, la: (table, v), None, us[i])
    return out


def test_searches_on_a_used_engine_equal_a_fresh_engine(monkeypatch):
    """Every search entry point sets the whole lane state for itself: after resignation, start positions, a playout cap, a
    self-play episode, an arena and a noised batch search on a two-lane engine, search / search_batch / search_callback give
    exactly what an engine gives that did none of it.  And search is search_batch with one position."""
    _clean_env(monkeypatch)
    n, k, S, slots = 5, 4, 8, 4
    sd, sd2 = weights_from_fixture(n, "ckpt_saved"), weights_from_fixture(n, "ckpt_0802")

    def engine():
        e = az.Engine(n, k, S, slots, engines=2, log_table=orc.numpy_log_table(S))
        assert e.lanes() == 2
        e.load_weights(sd, 0); e.load_weights(sd2, 1)
        return e

    boards, players, lasts, noise, us, Ts = _d_positions(n)
    used = engine()
    used.set_resign(0.05, min_ply=1)
    used.set_start_positions(boards[1:], players[1:], lasts[1:])
    used.set_playout_cap(3, full=0.5)
    c = used.selfplay(5, seed0=88, max_plies=7)
    assert c["plies"] > 0
    assert used.arena(4, seed0=88, temperature_table=orc.arena_T_table(n * n))["total"] == 4
    used.search_batch(boards, players, lasts, Ts, noise, us)
    got = _d_searches(used, n)
    used.close()
    fresh = engine()
    want = _d_searches(fresh, n)
    fresh.close()
    for what, w in want.items():
        for key in ("action", "pi", "N", "W", "P"):
            assert np.array_equal(got[what][key], w[key]), f"{what}: {key}: used engine vs fresh engine"
    for slot in (0, 1):
        for i in range(3):
            one, batch = want[f"search {i} slot {slot}"], want[f"batch of one {i} slot {slot}"]
            for key in ("pi", "N", "W", "P"):
                assert np.array_equal(one[key], batch[key][0]), f"search vs search_batch of one: position {i}, slot {slot}: {key}"
            assert one["action"] == int(batch["action"][0])
            assert int(one["N"].sum()) == S


# ------------------------------------------------------------------------------------------------
# E. one engine through the delta switch
# ------------------------------------------------------------------------------------------------
def _e_leaves(n):
    """a root and four of its leaves for net_eval_delta: one stone in a corner, two stones, three, and nine (evaluated in full)"""
    root = np.zeros(n * n, np.uint8)
    root[[7 * n + 7, 3 * n + 3]] = 1; root[[7 * n + 8, 11 * n + 2]] = 2
    boards, players, lasts = [], [], []
    for cells in ([0], [6 * n + 6, n * n - 1], [8 * n + 8, 14 * n, 2 * n + 9], [4 * n + j for j in range(9)]):
        b, pl = root.copy(), 1
        for c in cells:
            b[c] = pl
            pl = 3 - pl
        boards.append(b); players.append(pl); lasts.append(cells[-1])
    return root, 1, np.stack(boards), np.array(players, np.uint8), np.array(lasts, np.int16)


def test_one_engine_through_the_delta_switch_and_back(monkeypatch):
    """Consecutive episodes of the same seeds on one engine, the delta switch, its tile threshold and an option it does not serve
    changed in between (set_delta_eval and delta_max_tiles are rows of the graph key).  Every episode is the one a fresh engine
    plays in that configuration, records as bytes and delta_stats alike: the counters restart, the graph is captured again,
    and a net_eval_delta call leaves nothing behind in the lane's base activations, flags and counters."""
    _clean_env(monkeypatch)
    cfg = B_CONFIGS["delta_15x15"]
    n, k, S, G, cut = cfg["n"], cfg["k"], cfg["S"], cfg["G"], cfg["cut"]
    zero = dict(delta=0, full=0, tiles=0, base=0, by_tiles=[0] * 16)

    def configure(e, on, tiles, vl):
        e.set_delta_eval(on)
        assert e.delta_max_tiles(tiles) == tiles
        e.set_virtual_loss(vl)

    def fresh(on, tiles, vl):
        e = _b_engine(cfg)
        configure(e, on, tiles, vl)
        ep = _episode(e, G, B_SEED, cut)
        st = e.delta_stats(by_tiles=True)
        e.close()
        return ep, st

    kept = _b_engine(cfg)
    assert kept.lanes() == cfg["engines"] and kept.delta_eval() and kept.delta_max_tiles() == 12
    ref = _oracle_games("B-delta_15x15", orc.Oracle(n, k, S), orc.Net(n, _b_weights(cfg)[0]), n, B_SEED, range(G), cut=cut)
    stats = []
    steps = (("switch on", True, 12, 1, False), ("switch off", False, 12, 1, False), ("threshold 3", True, 3, 1, False),
             ("threshold 12 again", True, 12, 1, False), ("virtual loss 4", True, 12, 4, False), ("virtual loss 1 again", True, 12, 1, False),
             ("after a net_eval_delta call", True, 12, 1, True))
    for step, on, tiles, vl, call in steps:
        configure(kept, on, tiles, vl)
        if call:
            root, pl, boards, players, lasts = _e_leaves(n)
            got = kept.net_eval_delta(root, pl, boards, players, lasts)
            want = kept.net_eval(boards, players, lasts)
            for x, y in zip(got[:3], want):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{step}: net_eval_delta vs net_eval"
            assert (got[3][:3] > 0).all() and got[3][3] == -1
        ep = _episode(kept, G, B_SEED, cut)
        st = kept.delta_stats(by_tiles=True)
        want_ep, want_st = fresh(on, tiles, vl)
        _assert_same_episode(want_ep, ep, f"{step}: fresh engine vs kept engine", counters=LAUNCH_COUNTERS)
        for key in ep["rec"]:
            assert ep["rec"][key].tobytes() == want_ep["rec"][key].tobytes(), f"{step}: {key}"
        assert st == want_st, f"{step}: delta_stats: kept engine {st}, fresh engine {want_st}"
        if vl == 1:
            _assert_oracle_games(ep, ref, step)
        stats.append(st)
    on12, off, on3, back12, vl4, vl1, called = stats
    assert off == vl4 == zero                                    # the switch off, and an option the path does not serve
    assert on12 == back12 == vl1 == called and on12["delta"] > 0 and on12["base"] == 2 * ep["c"]["plies"]
    # threshold 3: the same evaluations, those above 3 tiles in full (an interior depth-1 leaf has 4)
    assert on3["delta"] + on3["full"] == on12["delta"] + on12["full"] and on3["full"] > on12["full"] and on3["delta"] > 0
    assert on3["by_tiles"][:4] == on12["by_tiles"][:4] and not any(on3["by_tiles"][4:])
    kept.close()
