"""az_set_resign and the search value per record, on the GPU.  The reference for everything is the unchanged CPU oracle:
its free-running games (Oracle.selfplay_game), and for every ply of them Oracle.search on the recorded position with that
ply's noise, u and temperature, which gives the root's N and W.  From those numpy computes the search value by the header's
definition, v = W[a*] / N[a*] with a* the most visited cell (lowest index on ties), chooses every threshold, and truncates
the games by the rule.  The engine has to produce exactly that: array_equal everywhere, no tolerances.

Two places where the oracle cannot serve and what stands in for it:
  * subtree reuse: the oracle's reuse game records no W, and Oracle.search always starts from a fresh root, so only the first
    ply of a reuse game has an oracle value.  There the threshold is chosen from the engine's own resign-off values; the games
    themselves are still the oracle's reuse games, truncated.
  * a natural end on a crossing ply: with a net that evaluates sensibly the side that completes a line is not the side whose
    value is low, so the case is built with the synthetic evaluator, whose values are random: the oracle's games are
    scanned for final, winning plies with a negative search value, and the engine is started one move before that win."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_resign_cpu import np_exempt
from tests.util import build_weights, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.self_play import resign_stats

REC_KEYS = ("boards", "movers", "lasts", "actions", "pis", "visits", "z")
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------------
# the reference: oracle games, their search values, the rule in numpy
# ---------------------------------------------------------------------------------------------------------------------
def search_value(N, W):
    """the header's definition on one root row: illegal cells have N = 0 and the maximum is >= 1, argmax takes the first"""
    a = int(np.argmax(N))
    assert N[a] >= 1
    return np.float64(W[a]) / np.float64(N[a])


def _onet(n, tag):
    return None if tag is None else orc.Net(n, weights_from_fixture(n, tag))


@functools.lru_cache(maxsize=None)
def _ref(n, k, S, G, seed0, tag, cut=0, leaf_sym=False, vl=0, reuse=False):
    """(games, values, ties): G free-running oracle games with seeds seed0 + g; values[g][m] = the search value of ply m from
    Oracle.search (None with reuse); ties = plies whose maximal visit count is shared by several cells.  Computed once per
    configuration and never modified."""
    nn = n * n
    o = orc.Oracle(n, k, S, synthetic=tag is None, leaf_sym=leaf_sym, virtual_loss=vl, reuse=reuse)
    net = _onet(n, tag)
    T = orc.selfplay_T_table(nn)

    def one(g):
        noise, us = orc.selfplay_tape(seed0 + g, n, maxply=cut or None)
        r = o.selfplay_game(net, noise, us, maxply=cut or None, game=seed0 + g)
        if reuse:
            return r, None, 0
        vs, ties, off = [], 0, 0
        for m in range(r["nply"]):
            ro = o.search(net, r["boards"][m], int(r["movers"][m]), int(r["lasts"][m]), T[m], noise[off:off + nn - m], us[m],
                          game=seed0 + g)
            assert np.array_equal(ro["N"], r["visits"][m]) and int(ro["action"]) == int(r["actions"][m]), "the oracle disagrees with itself"
            vs.append(search_value(ro["N"], ro["W"]))
            ties += int((ro["N"] == ro["N"].max()).sum() > 1)
            off += nn - m
        return r, np.array(vs, np.float64), ties
    with ThreadPoolExecutor(max_workers=8) as ex:
        out = list(ex.map(one, range(G)))
    return tuple(x[0] for x in out), tuple(x[1] for x in out), sum(x[2] for x in out)


def choose_threshold(values, min_ply=0):
    """-threshold midway between two neighbouring distinct per-game minima of v over plies >= min_ply, as many games below it
    as possible while at least one stays above and the threshold is in (0, 1] -> (threshold, games that cross)"""
    minima = [float(v[min_ply:].min()) if len(v) > min_ply else np.inf for v in values]
    distinct = sorted(set(x for x in minima if np.isfinite(x)))
    for j in range(len(distinct) - 2, -1, -1):
        mid = (distinct[j] + distinct[j + 1]) / 2
        crossing = [g for g, x in enumerate(minima) if x < mid]
        if distinct[j] < mid < distinct[j + 1] and -1.0 <= mid < 0.0 and len(crossing) < len(values):
            return -mid, crossing
    raise AssertionError(f"no threshold separates the minima {minima}")


def first_cross(v, thr, min_ply=0):
    return next((m for m in range(len(v)) if m >= min_ply and v[m] < -thr), -1)


def truncate(r, v, thr, min_ply=0, exempt=False):
    """game r under the rule: cut after its first crossing ply, the mover of that ply loses -- unless the game is exempt or
    that very move ended it"""
    out = {key: r[key] for key in REC_KEYS + ("nply", "result")}
    m = out["cross"] = first_cross(v, thr, min_ply)
    if m < 0 or exempt or (m == r["nply"] - 1 and r["result"] != 0):
        return out
    res = 3 - int(r["movers"][m])
    for key in REC_KEYS:
        out[key] = r[key][:m + 1]
    out["z"] = np.where(out["movers"] == res, 1, -1).astype(np.int8)
    out["nply"], out["result"] = m + 1, res
    return out


def _engine(n, k, S, slots, tag, **kw):
    e = az.Engine(n, k, S, slots, synthetic=tag is None, log_table=orc.numpy_log_table(S), **kw)
    if tag is not None:
        e.load_weights(weights_from_fixture(n, tag), 0)
    return e


def assert_episode(e, c, want, values, S, what, exempt=None, sims=True):
    """the engine's last episode = the games `want` (dicts of truncate): lengths, results, every record field, the value of
    every record, cross_ply, exempt, and the work counters as sums over these games"""
    nply, res = e.games()
    rec = e.records()
    assert nply.tolist() == [w["nply"] for w in want], f"{what}: plies per game"
    assert res.tolist() == [w["result"] for w in want], f"{what}: results"
    for key in REC_KEYS:
        exp = np.concatenate([w[key] for w in want])
        assert rec[key].shape == exp.shape and np.array_equal(rec[key], exp), f"{what}: {key} differ"
    if values is not None:
        exp = np.concatenate([np.float32(v[:w["nply"]]) for v, w in zip(values, want)])
        got = e.values()
        assert got.dtype == np.float32 and np.array_equal(got, exp), f"{what}: values differ"
    cross, ex = e.resign_info()
    assert cross.tolist() == [w["cross"] for w in want], f"{what}: cross_ply"
    assert ex.tolist() == (list(exempt) if exempt is not None else [False] * len(want)), f"{what}: exempt"
    plies = sum(w["nply"] for w in want)
    assert c["plies"] == c["records"] == plies and c["games"] == len(want), f"{what}: plies"
    if sims:
        assert c["root_evals"] == plies and c["simulations"] == S * plies, f"{what}: work counters"
    return rec


def _off(games, values):
    return [truncate(r, v if v is not None else np.zeros(r["nply"]), 2.0) for r, v in zip(games, values)]     # nothing crosses -2


def _values_then_prefix(n, k, S, G, slots, seed0, tag, cut=0, leaf_sym=False, vl=0, cache=0, what="", **kw):
    """the two tests that show the kernel is right: resign off -> every value is float32(v), on the host and packed on the
    device; resign on with a threshold from the oracle's values -> the truncated oracle games"""
    games, values, _ = _ref(n, k, S, G, seed0, tag, cut, leaf_sym, vl)
    thr, crossing = choose_threshold(values)
    assert 3 * len(crossing) >= G and 1 <= len(crossing) < G, f"{what}: {len(crossing)} of {G} games cross"      # on the oracle's numbers
    e = _engine(n, k, S, slots, tag, **kw)
    if leaf_sym:
        e.set_leaf_symmetry(True)
    if vl:
        e.set_virtual_loss(vl)
    if cache:
        e.set_eval_cache(cache)
    assert e.resign() == dict(threshold=0.0, min_ply=0, playout=0.0)
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    off = [dict(w, cross=-1) for w in _off(games, values)]
    assert_episode(e, c, off, values, S, f"{what} off")
    dev = torch.full((c["records"] + 64,), float("nan"), dtype=torch.float32, device=DEV)
    e.pack_values_into(dev.data_ptr())
    torch.cuda.synchronize()
    host = dev.cpu().numpy()
    assert np.array_equal(host[:c["records"]], e.values()) and np.isnan(host[c["records"]:]).all(), f"{what}: pack_values"
    e.set_resign(thr)
    assert e.resign() == dict(threshold=thr, min_ply=0, playout=0.0)
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    want = [truncate(r, v, thr) for r, v in zip(games, values)]
    assert [g for g, w in enumerate(want) if w["cross"] >= 0] == crossing
    assert_episode(e, c, want, values, S, f"{what} on")
    for g in range(G):
        if g not in crossing:
            assert want[g]["nply"] == games[g]["nply"] and want[g]["result"] == games[g]["result"]
    return e, games, values, thr, want


# ---------------------------------------------------------------------------------------------------------------------
# 1. shapes: the smallest at which k_move's reduction can go wrong
# ---------------------------------------------------------------------------------------------------------------------
CFG5 = (5, 4, 24, 6, 7100, "ckpt_saved")          # n, k, S, G, seed0, tag
CFG9 = (9, 5, 16, 8, 7200, "seeded")


@pytest.mark.parametrize("persist", ["1", "0"])
def test_5x5_values_and_prefix_property(persist, monkeypatch):
    monkeypatch.setenv("AZ_PERSIST", persist)
    n, k, S, G, seed0, tag = CFG5
    e, *_ = _values_then_prefix(n, k, S, G, 4, seed0, tag, what=f"5x5 AZ_PERSIST={persist}")
    assert (e.persistent() > 0) == (persist == "1")
    e.close()


def test_9x9_two_cells_per_lane_refilled_slots_two_lanes():
    n, k, S, G, seed0, tag = CFG9
    e, *_ = _values_then_prefix(n, k, S, G, 6, seed0, tag, engines=2, what="9x9")
    assert e.lanes() == 2 and e.persistent() == 0
    e.close()


def test_15x15_four_cells_per_lane_games_cut_at_12_plies():
    """a cut by max_plies stays a cut (result 0, z = 99) unless the ply crossed; on a crossing ply the resignation is the result"""
    e, games, values, thr, want = _values_then_prefix(15, 5, 12, 3, 3, 7300, "seeded", cut=12, what="15x15")
    assert all(r["nply"] == 12 and r["result"] == 0 for r in games)
    assert any(w["result"] == 0 and (w["z"] == 99).all() for w in want) and any(w["result"] in (1, 2) for w in want)
    e.close()


def test_5x5_synthetic_ties_pin_the_lowest_cell():
    n, k, S, G, seed0 = 5, 4, 8, 6, 7400
    _, _, ties = _ref(n, k, S, G, seed0, None)
    assert ties > 0, "no ply of the oracle's games has a tie for the most visited cell"
    e, *_ = _values_then_prefix(n, k, S, G, 4, seed0, None, what="5x5 synthetic S=8")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. search options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["virtual_loss", "cache", "leaf_symmetry"])
def test_options_keep_the_prefix_property(opt):
    n, k, S, G, seed0, tag = CFG5
    kw = dict(virtual_loss=dict(vl=4), cache=dict(cache=1 << 12), leaf_symmetry=dict(leaf_sym=True))[opt]
    e, *_ = _values_then_prefix(n, k, S, G, 4, seed0 + 50, tag, what=opt, **kw)
    if opt == "cache":
        assert e.counters()["cache_lookups"] > 0
    e.close()


def test_leaf_symmetry_at_9x9_on_the_lock_step_pipeline():
    n, k, S, G, seed0, tag = CFG9
    e, *_ = _values_then_prefix(n, k, S, 5, 3, seed0 + 50, tag, leaf_sym=True, what="9x9 leaf symmetry")
    e.close()


def test_deep_engine_cut_at_3_plies():
    S, G = 1040, 4
    e, *_ = _values_then_prefix(5, 4, S, G, 2, 7500, None, cut=3, deep=True, what="deep S=1040")
    assert e.persistent() == 0
    e.close()


def test_subtree_reuse_a_resigned_slot_starts_its_next_game_from_a_fresh_root():
    """(see the module docstring: the threshold comes from the engine's resign-off values here; the games are the oracle's)
    4 slots, 9 games: every slot that resigns is refilled, and the refilled game's first record is a fresh-root search"""
    n, k, S, G, seed0, tag = 5, 4, 24, 9, 7600, "ckpt_saved"
    games, _, _ = _ref(n, k, S, G, seed0, tag, reuse=True)
    fresh = orc.Oracle(n, k, S)
    e = _engine(n, k, S, 4, tag)
    e.set_subtree_reuse(True)
    c = e.selfplay(G, seed0=seed0)
    assert_episode(e, c, [dict(w, cross=-1) for w in _off(games, [None] * G)], None, S, "reuse off", sims=False)
    val, nply = e.values(), e.games()[0]
    values = [val[s:s + L].astype(np.float64) for s, L in zip(np.cumsum(nply) - nply, nply)]
    T, onet = orc.selfplay_T_table(n * n), _onet(n, tag)
    for g in range(G):           # what the oracle can pin: ply 0 of every game is searched from a fresh root
        noise, us = orc.selfplay_tape(seed0 + g, n)
        ro = fresh.search(onet, games[g]["boards"][0], 1, -1, T[0], noise[:n * n], us[0])
        assert values[g][0] == np.float32(search_value(ro["N"], ro["W"])), f"game {g}: value of the first ply"
    thr, crossing = choose_threshold(values)
    assert 3 * len(crossing) >= G and len(crossing) < G
    e.set_resign(thr)
    c = e.selfplay(G, seed0=seed0)
    want = [truncate(r, v, thr) for r, v in zip(games, values)]
    assert sum(w["nply"] < r["nply"] for w, r in zip(want, games)) >= 3
    assert_episode(e, c, want, values, S, "reuse on", sims=False)
    assert c["root_evals"] < c["plies"]                      # roots were retained, just never across a resignation
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the rule's edges
# ---------------------------------------------------------------------------------------------------------------------
def test_strictness_min_ply_and_exemption():
    n, k, S, G, seed0, tag = CFG5
    games, values, _ = _ref(n, k, S, G, seed0, tag)
    thr, crossing = choose_threshold(values)
    e = _engine(n, k, S, 4, tag)
    # strict: -threshold equal to one game's minimum -> that ply does not cross
    g0 = crossing[-1]
    m0 = int(np.argmin(values[g0]))
    t_eq = float(-values[g0][m0])
    assert 0.0 < t_eq <= 1.0 and not values[g0][m0] < -t_eq
    e.set_resign(t_eq)
    c = e.selfplay(G, seed0=seed0)
    want = [truncate(r, v, t_eq) for r, v in zip(games, values)]
    assert want[g0]["cross"] != m0 and want[g0]["nply"] == games[g0]["nply"]        # its minimum is its only candidate
    assert_episode(e, c, want, values, S, "strict")
    # min_ply just above a game's first crossing ply: it ends at its next crossing at or after min_ply, or naturally
    g1 = crossing[0]
    m1 = first_cross(values[g1], thr)
    e.set_resign(thr, min_ply=m1 + 1)
    assert e.resign()["min_ply"] == m1 + 1
    c = e.selfplay(G, seed0=seed0)
    want = [truncate(r, v, thr, m1 + 1) for r, v in zip(games, values)]
    assert want[g1]["cross"] == -1 or want[g1]["cross"] > m1
    assert want[g1]["nply"] > m1 + 1 and all(w["cross"] == -1 or w["cross"] > m1 for w in want)
    assert_episode(e, c, want, values, S, "min_ply")
    e.close()


def _exemption_case():
    n, k, S, G, seed0, tag = CFG5
    games, values, _ = _ref(n, k, S, G, seed0, tag)
    thr, crossing = choose_threshold(values)
    for permille in range(50, 1000, 50):         # some, but not all, of the crossing games exempt
        ex = np_exempt(seed0, G, permille)
        if 0 < ex[crossing].sum() < len(crossing):
            return games, values, thr, crossing, permille, ex
    raise AssertionError("no playout share splits the crossing games")


def test_exempt_games_play_on_and_report_their_crossing():
    n, k, S, G, seed0, tag = CFG5
    games, values, thr, crossing, permille, ex = _exemption_case()
    want = [truncate(r, v, thr, exempt=bool(x)) for r, v, x in zip(games, values, ex)]
    for g in crossing:
        if ex[g]:
            assert want[g]["nply"] == games[g]["nply"] and want[g]["result"] == games[g]["result"] and want[g]["cross"] >= 0
    assert any(w["nply"] < r["nply"] for w, r in zip(want, games))
    # two engines with different slot and lane counts agree
    for slots, lanes in ((4, 1), (3, 3)):
        e = _engine(n, k, S, slots, tag, engines=lanes)
        e.set_resign(thr, playout=permille / 1000)
        assert e.resign()["playout"] == permille / 1000
        c = e.selfplay(G, seed0=seed0)
        assert_episode(e, c, want, values, S, f"exemption slots={slots} lanes={lanes}", exempt=ex)
        # ... and so does a "rank" that plays the id block [lo, hi) with seed0 + lo
        if lanes == 1:
            lo, hi = 2, G
            c = e.selfplay(hi - lo, seed0=seed0 + lo)
            assert_episode(e, c, want[lo:hi], values[lo:hi], S, "exemption id block", exempt=ex[lo:hi])
        e.close()


def _winning_last_plies(n, k, S, seed0, count):
    """oracle games (synthetic evaluator) whose last ply wins the game although its search value is negative"""
    found = []
    for s in range(seed0, seed0 + count, 8):
        games, values, _ = _ref(n, k, S, 8, s, None)
        for g, (r, v) in enumerate(zip(games, values)):
            if r["result"] in (1, 2) and v[-1] < 0.0:
                found.append((s + g, r, v))
    return found


def test_a_natural_end_wins_over_resignation():
    """the engine starts one move before the win (set_start_positions, plies stay absolute) with -threshold just above that
    ply's value: the ply crosses, the sampled move completes the line, the mover wins as in the oracle's game"""
    n, k, S = 5, 4, 8
    found = _winning_last_plies(n, k, S, 7700, 32)
    assert found, "no oracle game ends on a winning move with a negative search value"
    e = _engine(n, k, S, 2, None)
    for seed, r, v in found[:3]:
        m = r["nply"] - 1
        thr = float(-v[m]) / 2
        assert 0.0 < thr < 1.0 and v[m] < -thr
        e.set_start_positions(r["boards"][m][None], r["movers"][m:m + 1], r["lasts"][m:m + 1])
        e.set_resign(thr)
        c = e.selfplay(1, seed0=seed)
        nply, res = e.games()
        assert nply.tolist() == [1] and res.tolist() == [r["result"]] and r["result"] == int(r["movers"][m]), f"seed {seed}"
        rec = e.records()
        assert int(rec["actions"][0]) == int(r["actions"][m]) and rec["z"].tolist() == [1]
        assert e.values().tolist() == [np.float32(v[m])] and e.resign_info()[0].tolist() == [m]
        # the same position one ply earlier in a game that does not end there: the crossing ply resigns
        if m >= 1 and v[m - 1] < 0.0:
            thr1 = float(-v[m - 1]) / 2
            e.set_start_positions(r["boards"][m - 1][None], r["movers"][m - 1:m], r["lasts"][m - 1:m])
            e.set_resign(thr1)
            e.selfplay(1, seed0=seed)
            nply, res = e.games()
            assert nply.tolist() == [1] and res.tolist() == [3 - int(r["movers"][m - 1])]
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. arena
# ---------------------------------------------------------------------------------------------------------------------
def test_arena_resigns_by_the_same_rule_and_no_game_is_exempt():
    n, k, S, G, seed0 = 5, 4, 32, 8, 7800
    nn = n * n
    sd_a, sd_b = weights_from_fixture(n, "ckpt_saved"), build_weights(n, seed=77)
    o, na, nb = orc.Oracle(n, k, S), orc.Net(n, sd_a), orc.Net(n, sd_b)
    T = orc.arena_T_table(nn)
    ogs, values, movers = [], [], []
    for g in range(G):
        us = np.random.RandomState(seed0 + g).random_sample(nn)
        r = o.arena_game(na, nb, g, us)
        board, pl, last, vs, mv = np.zeros(nn, np.uint8), 2 if g & 1 else 1, -1, [], []
        for ply in range(r["nply"]):
            ro = o.search(na if pl == 1 else nb, board, pl, last, T[(ply + 1) >> 1], None, us[ply])
            assert int(ro["action"]) == int(r["actions"][ply])
            vs.append(search_value(ro["N"], ro["W"])); mv.append(pl)
            board[ro["action"]] = pl
            pl, last = 3 - pl, int(ro["action"])
        ogs.append(r); values.append(np.array(vs)); movers.append(mv)
    thr, crossing = choose_threshold(values)
    assert 3 * len(crossing) >= G and len(crossing) < G
    want = []
    for r, v, mv in zip(ogs, values, movers):
        m = first_cross(v, thr)
        if m < 0 or (m == r["nply"] - 1 and r["result"] != 0):
            want.append((r["nply"], r["result"], m))
        else:
            want.append((m + 1, 3 - mv[m], m))
    e = az.Engine(n, k, S, 8, log_table=orc.numpy_log_table(S))
    e.load_weights(sd_a, 0); e.load_weights(sd_b, 1)
    plain = e.arena(G, seed0=seed0, temperature_table=T)
    assert plain["nply"].tolist() == [r["nply"] for r in ogs] and plain["results"].tolist() == [r["result"] for r in ogs]
    assert np.array_equal(e.values(), np.concatenate([np.float32(v) for v in values]))
    e.set_resign(thr, playout=1.0)                # every self-play game would be exempt; no arena game is
    r = e.arena(G, seed0=seed0, temperature_table=T)
    assert r["nply"].tolist() == [w[0] for w in want] and r["results"].tolist() == [w[1] for w in want]
    for g in range(G):
        L = want[g][0]
        assert np.array_equal(r["actions"][g][:L], ogs[g]["actions"][:L]) and (r["actions"][g][L:] == -1).all()
    cross, ex = e.resign_info()
    assert cross.tolist() == [w[2] for w in want] and not ex.any()
    assert np.array_equal(e.values(), np.concatenate([np.float32(v[:w[0]]) for v, w in zip(values, want)]))
    tally = [sum(w[1] == x for w in want) for x in (1, 2, 3)]
    assert [r["wins"], r["losses"], r["draws"]] == tally and r["total"] == G
    assert r["win_rate"] == (tally[0] + 0.5 * tally[2]) / G
    assert any(w[0] < g["nply"] for w, g in zip(want, ogs))
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. one engine through the settings; the contract
# ---------------------------------------------------------------------------------------------------------------------
def _snapshot(e, c):
    return e.records(), e.games(), e.values(), e.resign_info(), (c["plies"], c["simulations"], c["root_evals"])


def _same(a, b, what):
    for key in REC_KEYS:
        assert np.array_equal(a[0][key], b[0][key]), f"{what}: {key}"
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]) and np.array_equal(a[2], b[2]), what
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1]) and a[4] == b[4], what


@pytest.mark.parametrize("cfg,slots", [(CFG5, 4), (CFG9, 3)], ids=["5x5-persistent", "9x9-lock-step"])
def test_mode_walk_on_one_engine(cfg, slots):
    """off, on, off: a captured ply graph that outlived the setter would show as a second episode equal to the first"""
    n, k, S, G, seed0, tag = cfg
    games, values, _ = _ref(n, k, S, G, seed0, tag)
    thr, crossing = choose_threshold(values)
    e = _engine(n, k, S, slots, tag)
    first = _snapshot(e, e.selfplay(G, seed0=seed0))
    e.set_resign(thr)
    c = e.selfplay(G, seed0=seed0)
    assert_episode(e, c, [truncate(r, v, thr) for r, v in zip(games, values)], values, S, "second episode")
    second = _snapshot(e, c)
    e.set_resign(0)
    third = _snapshot(e, e.selfplay(G, seed0=seed0))
    e.close()
    _same(first, third, "first and third episode")
    assert first[1][0].tolist() == [r["nply"] for r in games] and second[4][0] < first[4][0]
    fresh = _engine(n, k, S, slots, tag)
    fresh.set_resign(thr)
    _same(second, _snapshot(fresh, fresh.selfplay(G, seed0=seed0)), "second episode and a fresh engine's")
    fresh.close()


def test_contract():
    n, k, S, G, seed0, tag = CFG5
    L = _capi.lib()
    e = _engine(n, k, S, 4, tag)
    # nothing to report before any episode
    for call in (e.values, e.resign_info):
        with pytest.raises(az.AzError, match=r"\(-6\)"):
            call()
    e.set_resign(0.6, min_ply=3, playout=0.25)
    for bad in ((-0.1, 0, 0), (1.5, 0, 0), (float("nan"), 0, 0), (0.5, -1, 0), (0.5, 0, -1), (0.5, 0, 1001)):
        assert L.az_set_resign(e.h, *bad) == -1, bad                      # AZ_ERR_INVALID
        assert "az_set_resign" in L.az_last_error(e.h).decode()
        assert e.resign() == dict(threshold=0.6, min_ply=3, playout=0.25)   # the previous setting is kept
    assert L.az_set_resign(e.h, 1.0, 0, 1000) == 0 and e.resign() == dict(threshold=1.0, min_ply=0, playout=1.0)
    # searches ignore the setting
    games, values, _ = _ref(n, k, S, G, seed0, tag)
    pos = (np.stack([r["boards"][3] for r in games]), np.array([r["movers"][3] for r in games], np.uint8),
           np.array([r["lasts"][3] for r in games], np.int16))
    rs = np.random.RandomState(3)
    noise = [rs.dirichlet([0.3] * int((b == 0).sum())) for b in pos[0]]
    us = rs.random_sample(G)
    e.set_resign(0)
    before_b = e.search_batch(pos[0], pos[1], pos[2], 0.7, noise, us)
    before_s = e.search(pos[0][1], pos[1][1], pos[2][1], 0.7, noise[1], us[1])
    e.set_resign(0.001)                                       # nearly every ply would cross
    after_b = e.search_batch(pos[0], pos[1], pos[2], 0.7, noise, us)
    after_s = e.search(pos[0][1], pos[1][1], pos[2][1], 0.7, noise[1], us[1])
    for key in ("N", "W", "P", "pi", "action"):
        assert np.array_equal(before_b[key], after_b[key]) and np.array_equal(before_s[key], after_s[key]), key
    assert e.resign()["threshold"] == 0.001                  # and leave it in force
    with pytest.raises(az.AzError, match=r"\(-6\)"):           # a search forgets the last episode
        e.values()
    # while an episode is open the setting cannot change
    e.selfplay_begin(3, seed0=seed0)
    with pytest.raises(az.AzError, match=r"az_set_resign failed \(-6\)"):
        e.set_resign(0.5)
    e.selfplay_step(1)
    e.selfplay_end()
    assert e.resign()["threshold"] == 0.001 and len(e.values()) == 3 and len(e.resign_info()[0]) == 3
    e.clear_episode()
    for call in (e.values, e.resign_info):
        with pytest.raises(az.AzError, match=r"\(-6\)"):
            call()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the Python seams
# ---------------------------------------------------------------------------------------------------------------------
def _controller(tag, n=5):
    from alphazero_piskvorky_amd import net
    from alphazero_piskvorky_amd.controller import NeuralNetworkController
    m = net.GomokuNet(board_size=n)
    m.load_state_dict({kk: torch.tensor(v) for kk, v in weights_from_fixture(n, tag).items()})
    m.eval()
    return NeuralNetworkController(m, device=DEV)


def test_selfplay_manager_returns_the_truncated_games_examples_and_their_statistics():
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    n, k, S, G, seed0, tag = CFG5
    games, values, thr, crossing, permille, ex = _exemption_case()
    want = [truncate(r, v, thr, exempt=bool(x)) for r, v, x in zip(games, values, ex)]
    params = {"num_simulations": S, "c_puct": 2.0}
    off = SelfPlayManager(_controller(tag), DEV, mcts_params=params, concurrent_games=4, seed=seed0)
    full = off.generate_self_play(G)
    assert off.last_resign_stats is None and len(full) == 4 * sum(r["nply"] for r in games)
    mgr = SelfPlayManager(_controller(tag), DEV, mcts_params=params, concurrent_games=4, seed=seed0,
                          resign={"threshold": thr, "playout": permille / 1000})
    got = mgr.generate_self_play(G)
    # the resign-off examples of the plies that remain, z relabelled by hand from the new results
    exp, at = [], 0
    for r, w in zip(games, want):
        for m in range(w["nply"]):
            for a in range(4):
                st, pi, z = full[at + 4 * m + a]
                if w["nply"] < r["nply"]:
                    z = 1 if int(r["movers"][m]) == w["result"] else -1
                exp.append((st, pi, z))
        at += 4 * r["nply"]
    assert len(got) == len(exp) < len(full)
    for i, ((s1, p1, z1), (s2, p2, z2)) in enumerate(zip(got, exp)):
        assert torch.equal(s1, s2) and np.array_equal(p1, p2) and z1 == z2, f"example {i}"
    movers = [int(r["movers"][w["cross"]]) if w["cross"] >= 0 else 0 for r, w in zip(games, want)]
    stats = resign_stats([w["result"] for w in want], [w["cross"] for w in want], ex, movers)
    assert mgr.last_resign_stats == stats
    assert stats["resigned"] == sum(w["nply"] < r["nply"] for w, r in zip(want, games)) > 0 and stats["exempt_crossed"] > 0
    # the option taken away again: the same manager plays the whole games
    mgr.resign = None
    again = mgr.generate_self_play(G)
    assert len(again) == len(full) and mgr.last_resign_stats is None and mgr._engine.resign()["threshold"] == 0.0


def test_model_evaluator_takes_the_option():
    from alphazero_piskvorky_amd import constants
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator
    constants.NUM_EVAL_SIMULATIONS = 32
    try:
        cand, base = _controller("ckpt_saved"), _controller("ckpt_0802")
        plain = ModelEvaluator(device=DEV, seed=93)
        plain.evaluate(cand, base, num_games=8)
        vals = plain._engine.values()
        nply = plain.last_result["nply"]
        per_game = [vals[s:s + L] for s, L in zip(np.cumsum(nply) - nply, nply)]
        thr, crossing = choose_threshold([v.astype(np.float64) for v in per_game])
        ev = ModelEvaluator(device=DEV, seed=93, resign={"threshold": thr})
        _, metrics = ev.evaluate(cand, base, num_games=8)
        r = ev.last_result
        assert metrics["total"] == 8 and ev._engine.resign()["threshold"] == thr
        for g in range(8):
            m = first_cross(per_game[g].astype(np.float64), thr)
            assert int(r["nply"][g]) == (int(nply[g]) if m < 0 else m + 1)
            assert np.array_equal(r["actions"][g][:r["nply"][g]], plain.last_result["actions"][g][:r["nply"][g]])
        assert (r["nply"] < nply).any()
        ev.resign = None
        ev.evaluate(cand, base, num_games=8)
        assert np.array_equal(ev.last_result["actions"], plain.last_result["actions"])
    finally:
        constants.NUM_EVAL_SIMULATIONS = 200
