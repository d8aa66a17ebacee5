"""az_set_win_rule on the GPU, against the numpy restatement in tests/win_rule.py: the searches of tests/forced.py and
tests/solver.py with their module-level `wins_through` pointed at the exact rule.  The restatement's evaluator is the engine's own
az_net_eval, so every comparison is exact: integer equality for visits, actions, statuses, boards and results, == on the
float64 W and on the float32 priors and pi.

The crafted gap position (tests.win_rule.gap_position) tells the rules apart: the mover holds k of k + 1 cells in a row and a
constant net pulls the search into the gap.  Under FREESTYLE that child is a win at every visit (N = S, W = S, S terminal
simulations); under EXACT it is an overline, worth nothing (W = 0.0, no terminal).  Checked on the CPU at (7,4), (9,5), (15,5)
with S = 32."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import forced, ties
from tests import solver as sv
from tests import win_rule as wr
from tests.util import build_weights

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

C_PUCT = 2.0
S1 = 32
REC_KEYS = ("boards", "movers", "lasts", "actions", "pis", "visits", "z")
SWITCHES = ("AZ_GRAPH", "AZ_PROFILE_EVENTS", "AZ_PERSIST", "AZ_COMPACT", "AZ_VL_FORCE")


def _clean_env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        if value is not None:
            monkeypatch.setenv(name, value)


def engine(n, k, S, slots, sd=None, rule="exact", **kw):
    e = az.Engine(n, k, S, slots, log_table=orc.numpy_log_table(S), c_puct=C_PUCT, **kw)
    e.load_weights(build_weights(n) if sd is None else sd, 0)
    if rule is not None:
        e.set_win_rule(rule)
        assert e.win_rule() == rule
    return e


class NetEval:
    """evaluate(board, player, last) through the engine's az_net_eval (the rule does not touch it), every position once; a
    constant net is evaluated once"""

    def __init__(self, n, k, sd=None, constant=False):
        self.n, self.k, self.sd, self.constant, self.memo, self.eng = n, k, sd, constant, {}, None

    def __call__(self, board, player, last):
        key = () if self.constant else (bytes(board), int(player), int(last))
        if key not in self.memo:
            if self.eng is None:
                self.eng = engine(self.n, self.k, 1, 1, self.sd, rule=None)
            _, P, v = self.eng.net_eval(np.asarray(board, np.uint8)[None], [player], [last])
            self.memo[key] = (P[0].copy(), float(v[0]))
        return self.memo[key]

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None


def gap_net(n, cells, level=4.0):
    return ties.constant_state_dict(n, wr.gap_logits(n, cells, level), 0.0)


def with_draws(p, seed):
    rs = np.random.RandomState(seed)
    return dict(p, noise=rs.dirichlet([0.3] * int((p["board"] == 0).sum())), u=float(rs.random_sample()))


def random_positions(n, k):
    out = []
    for i, (stones, seed) in enumerate(((0, 1), (6, 2), (11, 3))):
        board, player, last = wr.random_position(n, k, stones, seed)
        out.append(with_draws(dict(board=board, player=player, last=last, T=(1.0, 0.5, 1e-9)[i]), 1000 * n + i))
    return out


def gap_case(n, k, gap_at=None, T=1.0):
    board, player, last, gap = wr.gap_position(n, k, gap_at)
    return with_draws(dict(board=board, player=player, last=last, T=T, gap=gap), 77 * n + k)


def plain_search(ev, n, k, S, p, noised, info=None):
    """the plain search of tests/solver.py (solver off: tests/test_solver_cpu.py holds it to Oracle.search), which counts its
    terminal simulations"""
    return sv.search(ev, n, k, S, p["board"], p["player"], p["last"], p["noise"] if noised else None, False, C_PUCT, info=info)


def assert_search(r, want, p, S, what):
    assert np.array_equal(r["N"], want["N"]), f"{what}: visits"
    assert np.array_equal(r["W"], want["W"]), f"{what}: W"
    assert np.array_equal(r["P"], want["P"]), f"{what}: priors"
    legal = np.flatnonzero(p["board"] == 0)
    pi, a = sv.pi_action(r["N"][legal], p["board"], p["T"], p["u"], orc.numpy_log_table(S))
    assert r["pi"].dtype == np.float32 and np.array_equal(r["pi"], pi), f"{what}: pi"
    assert int(r["action"]) == a, f"{what}: action"


def check_searches(e, ev, n, k, S, ps, noised, what):
    """az_search and az_search_batch of every position against the restatement under the rule in force there, terminal hits
    included -> the restatement's terminal counts"""
    rb = e.search_batch(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps],
                        np.array([p["T"] for p in ps]), [p["noise"] for p in ps] if noised else None, [p["u"] for p in ps])
    hits_batch = e.counters()["terminal_hits"]
    terms = []
    for i, p in enumerate(ps):
        info = {}
        want = plain_search(ev, n, k, S, p, noised, info)
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"] if noised else None, p["u"])
        assert e.counters()["terminal_hits"] == info["terminals"], f"{what} position {i}: terminal hits"
        assert_search(r, want, p, S, f"{what} position {i} az_search")
        assert_search({key: val[i] for key, val in rb.items()}, want, p, S, f"{what} position {i} az_search_batch")
        terms.append(info["terminals"])
    assert hits_batch == sum(terms), f"{what}: terminal hits of the batch"
    return terms


# ---------------------------------------------------------------------------------------------------------------------
# 1. rules replay on every size
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(3, 16))
def test_rules_replay_every_size(n):
    """exact runs touching edges and corners (won), k + 1 and 2k - 1 cells with the middle one last (not won, the game goes on),
    2k + 1 cells with the middle one last (the first half to reach k wins, by the numpy replay), an overline crossing an exact
    run (won), the no-wrap cases; then the same engine back on freestyle gives the bytes of an
    engine that never set the rule"""
    e = az.Engine(n, min(n, 3), 8, 4, synthetic=True, log_table=orc.numpy_log_table(8))
    fresh = {}
    for k in sorted({kk for kk in (3, 4, 5, n) if kk <= n}):
        e.close()
        e = az.Engine(n, k, 8, 4, synthetic=True, log_table=orc.numpy_log_table(8))
        cases = wr.line_cases(n, k)
        L = max(len(c) for _, c in cases)
        acts = -np.ones((len(cases), L), np.int16)
        for i, (_, c) in enumerate(cases):
            acts[i, :len(c)] = c
        fresh[k] = e.rules_replay(acts)
        e.set_win_rule("exact")
        r = e.rules_replay(acts)
        won = lost = 0
        for i, (name, c) in enumerate(cases):
            term, board, pl, res = wr.replay(c, n, k, "exact")
            assert int(r["results"][i]) == res, f"{n}x{n} k={k} {name}: {c}"
            assert np.array_equal(r["term_before"][i, :len(c)], term) and np.array_equal(r["boards"][i], board)
            assert int(r["players"][i]) == pl and int(r["first_illegal"][i]) == -1
            if name.startswith("over"):
                assert res == 0 and not term.any(), f"{name}: an overline wins nothing and the game goes on"
                assert int(fresh[k]["results"][i]) == 1
                lost += 1
            if name.startswith(("exact", "cross")):
                assert res == 1, name
                won += 1
            fterm, fboard, fpl, fres = wr.replay(c, n, k, "freestyle")
            assert int(fresh[k]["results"][i]) == fres and np.array_equal(fresh[k]["term_before"][i, :len(c)], fterm)
        assert won > 0 and (lost > 0 or n <= k + 1)
        e.set_win_rule("freestyle")
        back = e.rules_replay(acts)
        for key in back:
            assert back[key].tobytes() == fresh[k][key].tobytes(), key
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. single searches against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noised", [True, False], ids=["noise", "no-noise"])
@pytest.mark.parametrize("n,k,persist", [(5, 4, None), (7, 4, None), (5, 4, "0"), (7, 4, "0"), (9, 5, None), (15, 5, None)],
                         ids=["5x5", "7x7", "5x5-lockstep", "7x7-lockstep", "9x9", "15x15"])
def test_single_searches_equal_the_restatement(n, k, persist, noised, monkeypatch):
    _clean_env(monkeypatch, AZ_PERSIST=persist)
    wr.use_rule(monkeypatch, "exact")
    ev = NetEval(n, k)
    e = engine(n, k, S1, 4)
    check_searches(e, ev, n, k, S1, random_positions(n, k), noised, f"{n}x{n} seeded net")
    assert (e.persistent() > 0) == (n <= 7 and persist is None)
    e.close(); ev.close()


@pytest.mark.parametrize("n,k,persist", [(5, 4, None), (7, 4, None), (5, 4, "0"), (7, 4, "0"), (9, 5, None), (15, 5, None)],
                         ids=["5x5", "7x7", "5x5-lockstep", "7x7-lockstep", "9x9", "15x15"])
def test_the_gap_is_an_overline(n, k, persist, monkeypatch):
    """logit 4.0 on the gap: under EXACT the child takes all the visits it takes under FREESTYLE but is worth nothing.  This is
    the case that fails on an engine without the rule."""
    _clean_env(monkeypatch, AZ_PERSIST=persist)
    p = gap_case(n, k)
    sd = gap_net(n, [p["gap"]])
    ev = NetEval(n, k, sd, constant=True)
    e = engine(n, k, S1, 4, sd)
    wr.use_rule(monkeypatch, "exact")
    terms = check_searches(e, ev, n, k, S1, [p], False, f"{n}x{n} gap, exact")
    r = e.search(p["board"], p["player"], p["last"], 1.0, None, 0.5)
    print(f"{n}x{n} exact: N {r['N'][p['gap']]} W {r['W'][p['gap']]} terminals {terms}")
    if n >= 7:
        assert r["N"][p["gap"]] == S1 and r["W"][p["gap"]] == 0.0 and terms == [0]
    check_searches(e, ev, n, k, S1, [p], True, f"{n}x{n} gap, exact, noised")
    e.set_win_rule("freestyle")
    wr.use_rule(monkeypatch, "freestyle")
    terms = check_searches(e, ev, n, k, S1, [p], False, f"{n}x{n} gap, freestyle")
    r = e.search(p["board"], p["player"], p["last"], 1.0, None, 0.5)
    print(f"{n}x{n} freestyle: N {r['N'][p['gap']]} W {r['W'][p['gap']]} terminals {terms}")
    if n >= 7:
        assert r["N"][p["gap"]] == S1 and r["W"][p["gap"]] == float(S1) and terms == [S1]
    assert (e.persistent() > 0) == (n <= 7 and persist is None)
    e.close(); ev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the probe limit of the wave test
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,rule", [(10, 8, "exact"), (10, 8, "freestyle"), (11, 9, "exact"), (11, 9, "freestyle"), (10, 9, "freestyle"),
                                      (10, 9, "exact")])
def test_probe_limit(n, k, rule, monkeypatch):
    """8 probe lanes per side: EXACT at k = 8 probes s = 1..8 on the wave path, at k = 9 it runs the scalar loop; FREESTYLE stays
    on the wave path up to k = 9.  The gap position (an overline under EXACT), the same with one stone less (exactly k: a win
    under both rules) and, under EXACT, a stone put at the end of an overline that is already on the board: one side alone
    counts k, the capped sum is k + 1"""
    _clean_env(monkeypatch)
    p = gap_case(n, k)
    sd = gap_net(n, [p["gap"], n // 2 * n + k + 1] if n >= k + 2 else [p["gap"]])
    ev = NetEval(n, k, sd, constant=True)
    e = engine(n, k, S1, 2, sd, rule=rule)
    wr.use_rule(monkeypatch, rule)
    terms = check_searches(e, ev, n, k, S1, [p], False, f"{n}x{n} k={k} {rule} gap")
    assert (terms[0] > 0) == (rule == "freestyle")
    q = dict(p, board=p["board"].copy())
    opp = wr.far_cells(n, k, (n // 2,))
    q["board"][n // 2 * n + k] = 0                                # the far end of the segment
    q["board"][opp[-1]] = 0                                       # and one of the opponent's: X stays to move
    q["last"] = opp[-2]
    terms = check_searches(e, ev, n, k, S1, [with_draws(q, 5)], False, f"{n}x{n} k={k} {rule} exact run")
    assert terms[0] > 0
    if rule == "exact" and n >= k + 2:
        board, player, last, cell = wr.overline_position(n, k)
        o = with_draws(dict(board=board, player=player, last=last, T=1.0), 6)
        terms = check_searches(e, ev, n, k, S1, [o], False, f"{n}x{n} k={k} stone at the end of an overline")
        r = e.search(board, player, last, 1.0, None, 0.5)
        assert terms[0] == 0 and r["N"][cell] > 0
    e.close(); ev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. whole games
# ---------------------------------------------------------------------------------------------------------------------
def assert_replay(rec, nply, res, starts, n, k, rule, what):
    """every finished game, replayed with the numpy rule from its start position, ends where the engine ended it"""
    off = 0
    for g in range(len(nply)):
        L = int(nply[g])
        board, player = starts[g % len(starts)][:2] if starts else (np.zeros(n * n, np.uint8), 1)
        assert np.array_equal(rec["boards"][off], board), f"{what} game {g}: first record"
        assert wr.result_after(board, rec["movers"][off], rec["actions"][off:off + L], n, k, rule) == (L, int(res[g])), f"{what} game {g}"
        off += L
    assert off == len(rec["actions"])


@pytest.mark.parametrize("n,k,S,persist", [(5, 3, 24, None), (5, 4, 24, None), (5, 4, 24, "0"), (9, 5, 24, None), (15, 5, 24, None)],
                         ids=["5x5k3", "5x5", "5x5-lockstep", "9x9", "15x15"])
def test_whole_games_from_gap_openings(n, k, S, persist, monkeypatch):
    _clean_env(monkeypatch, AZ_PERSIST=persist)
    G, seed0 = 3, 40
    board, player, last, gaps = wr.opening(n, k)
    sd = gap_net(n, gaps, 2.0)
    ev = NetEval(n, k, sd, constant=True)
    e = engine(n, k, S, 2, sd)
    e.set_start_positions(board[None], [player], [last])
    c = e.selfplay(G, seed0=seed0)
    assert (e.persistent() > 0) == (n <= 7 and persist is None)
    rec, (nply, res) = e.records(), e.games()
    assert_replay(rec, nply, res, [(board, player)], n, k, "exact", f"{n}x{n}")
    off, differ, hits = 0, 0, 0
    for g in range(G):
        wr.use_rule(monkeypatch, "exact")
        want = wr.selfplay_from(ev, n, k, S, seed0 + g, board, player, last)
        wr.use_rule(monkeypatch, "freestyle")
        free = wr.selfplay_from(ev, n, k, S, seed0 + g, board, player, last)
        L = int(nply[g])
        assert L == want["nply"] and int(res[g]) == want["result"], f"game {g}: length / result"
        for key in REC_KEYS:
            assert np.array_equal(rec[key][off:off + L], want[key]), f"game {g}: {key}"
        differ += not (free["nply"] == want["nply"] and np.array_equal(free["actions"], want["actions"])
                       and np.array_equal(free["visits"], want["visits"]))
        off += L
    assert differ > 0, "no compared game tells the rules apart"
    assert c["simulations"] == S * c["plies"] and c["expansions"] + c["terminal_hits"] == c["simulations"]
    e.close(); ev.close()


def test_arena_games_end_where_the_rule_ends_them():
    n, k, S, G = 9, 5, 24, 6
    board, player, last, gaps = wr.opening(n, k)
    sd = gap_net(n, gaps, 2.0)
    for rule in wr.RULES:
        e = engine(n, k, S, 4, sd, rule=rule)
        e.load_weights(build_weights(n), 1)
        e.set_start_positions(board[None], [player], [last])
        a = e.arena(G, seed0=9)
        rec = e.records()
        off = 0
        for g in range(G):
            L = int(a["nply"][g])
            b, pl = (board, player) if g % 2 == 0 else (np.where(board == 0, 0, 3 - board).astype(np.uint8), 3 - player)
            assert np.array_equal(rec["boards"][off], b)
            assert wr.result_after(b, pl, a["actions"][g][:L], n, k, rule) == (L, int(a["results"][g])), (rule, g)
            off += L
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(9, 5), (15, 5)])
def test_virtual_loss_batches(n, k, monkeypatch):
    wr.use_rule(monkeypatch, "exact")
    p = gap_case(n, k)
    sd = gap_net(n, [p["gap"]])
    ev = NetEval(n, k, sd, constant=True)
    e = engine(n, k, S1, 2, sd)
    e.set_virtual_loss(4)
    for noised in (False, True):
        want = forced.search(ev, n, k, S1, p["board"], p["player"], p["last"], p["noise"] if noised else None, 0.0, C_PUCT, L=4)
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"] if noised else None, p["u"])
        assert_search(r, want, p, S1, f"{n}x{n} L=4 noised={noised}")
        assert e.counters()["terminal_hits"] == 0 and r["N"][p["gap"]] > 0      # the overline is visited and ends nothing
    e.close(); ev.close()


@functools.lru_cache(maxsize=None)
def _minimax_memo(n, k):
    return {}


@pytest.mark.parametrize("n,k,S,stones,persist", [(4, 3, 200, (4, 6, 8), None), (4, 3, 200, (4, 6, 8), "0"),
                                                  (5, 4, 200, (15, 17, 19), None), (5, 4, 200, (15, 17, 19), "0")],
                         ids=["4x4", "4x4-lockstep", "5x5", "5x5-lockstep"])
def test_solver_proves_the_exact_game(n, k, S, stones, persist, monkeypatch):
    """every proven edge and root status equals brute-force minimax under EXACT: the solver marks what the descent's own win test
    finds, so it needs no change for the rule"""
    _clean_env(monkeypatch, AZ_PERSIST=persist)
    wr.use_rule(monkeypatch, "exact")
    ps = [with_draws(dict(zip(("board", "player", "last"), wr.random_position(n, k, st, 60 + 7 * i + st)), T=1.0), i)
          for i in range(4) for st in stones]
    e = engine(n, k, S, 4)
    e.set_solver(True)
    rb = e.search_batch(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps], 1.0, None, [p["u"] for p in ps])
    edges, roots = e.last_proof()
    assert (e.persistent() > 0) == (persist is None)
    memo, proven, roots_proven = _minimax_memo(n, k), 0, 0
    for i, p in enumerate(ps):
        for a in np.flatnonzero(edges[i]):
            assert edges[i][a] == sv.minimax_edge(p["board"], p["player"], int(a), n, k, memo), (i, a)
            proven += 1
        if roots[i]:
            assert roots[i] == sv.minimax(p["board"].copy(), p["player"], n, k, memo), i
            roots_proven += 1
    assert proven > 0 and roots_proven > 0
    ev = NetEval(n, k)
    want = sv.search(ev, n, k, S, ps[0]["board"], ps[0]["player"], ps[0]["last"], None, True, C_PUCT)
    assert np.array_equal(rb["N"][0], want["N"]) and np.array_equal(rb["W"][0], want["W"]) and np.array_equal(edges[0], want["st"])
    assert int(roots[0]) == want["root"]
    e.close(); ev.close()


def test_deep_engine(monkeypatch):
    n, k, S = 9, 5, 1100
    wr.use_rule(monkeypatch, "exact")
    p = gap_case(n, k)
    sd = gap_net(n, [p["gap"]])
    ev = NetEval(n, k, sd, constant=True)
    e = engine(n, k, S, 1, sd, deep=True)
    info = {}
    want = plain_search(ev, n, k, S, p, False, info)
    r = e.search(p["board"], p["player"], p["last"], p["T"], None, p["u"])
    assert_search(r, want, p, S, "deep 9x9")
    assert e.counters()["terminal_hits"] == info["terminals"] and r["N"].sum() == S
    e.close(); ev.close()


def test_external_evaluator_and_callback(monkeypatch):
    """the engine's own net behind both seams: the batched external evaluator and az_search_callback give the searches of the
    engine's evaluator, under the rule"""
    import torch
    n, k, S = 9, 5, S1
    wr.use_rule(monkeypatch, "exact")
    p = gap_case(n, k)
    sd = gap_net(n, [p["gap"]])
    ev = NetEval(n, k, sd, constant=True)
    info = {}
    want = plain_search(ev, n, k, S, p, True, info)
    e = engine(n, k, S, 2, sd)
    r = e.search_callback(p["board"], p["player"], p["last"], p["T"], lambda cells, pl, la: ev(cells, pl, la), p["noise"], p["u"])
    assert_search(r, want, p, S, "az_search_callback")
    cap = e.ext_capacity()
    planes = torch.zeros((cap, 4, n, n), dtype=torch.float32, device="cuda:0")
    policy = torch.zeros((cap, n * n), dtype=torch.float32, device="cuda:0")
    value = torch.zeros(cap, dtype=torch.float32, device="cuda:0")
    P0, v0 = ev(p["board"], p["player"], p["last"])

    def fn(net, count):
        policy[:count].copy_(torch.from_numpy(np.tile(P0, (count, 1))))
        value[:count].fill_(v0)
        torch.cuda.synchronize()

    e.set_external_evaluator(planes.data_ptr(), policy.data_ptr(), value.data_ptr(), cap, fn)
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    assert_search(r, want, p, S, "external evaluator")
    assert e.counters()["terminal_hits"] == info["terminals"]
    e.close(); ev.close()


@pytest.mark.parametrize("option", ["eval-cache", "leaf-symmetry", "subtree-reuse", "resign", "playout-cap"])
def test_episodes_under_options_close_consistently(option):
    """the cache gives the records it gives switched off; the other options have no exact-rule restatement: every game they
    play ends where the numpy rule ends it (resigned games: earlier, with the other colour as the winner)"""
    n, k, S, G = 5, 4, 24, 6
    board, player, last, gaps = wr.opening(n, k)
    sd = gap_net(n, gaps, 2.0)
    e = engine(n, k, S, 4, sd)
    e.set_start_positions(board[None], [player], [last])
    e.selfplay(G, seed0=500)
    plain = (e.records(), e.games())
    if option == "eval-cache":
        e.set_eval_cache(1 << 10)
    elif option == "leaf-symmetry":
        e.set_leaf_symmetry(True)
    elif option == "subtree-reuse":
        e.set_subtree_reuse(True)
    elif option == "resign":
        e.set_resign(0.05)
    else:
        e.set_playout_cap(8, 0.5, export_full_only=False)
    for rep in range(2 if option == "eval-cache" else 1):
        e.selfplay(G, seed0=500)
        rec, (nply, res) = e.records(), e.games()
        if option == "eval-cache":
            for key in rec:
                assert rec[key].tobytes() == plain[0][key].tobytes(), key
            assert np.array_equal(nply, plain[1][0]) and np.array_equal(res, plain[1][1])
    off = 0
    for g in range(G):
        L = int(nply[g])
        ended = wr.result_after(board, player, rec["actions"][off:off + L], n, k, "exact")
        if option == "resign" and ended != (L, int(res[g])):
            assert ended == (L, 0) and int(res[g]) == 3 - int(rec["movers"][off + L - 1]), g     # resigned before the end
        else:
            assert ended == (L, int(res[g])), (option, g)
        off += L
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. setter contract
# ---------------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *args, match=None):
    with pytest.raises(_capi.AzError, match=match) as ex:
        fn(*args)
    assert f"({code})" in str(ex.value), str(ex.value)


def test_setter_contract():
    n, k, S = 9, 5, 16
    e = engine(n, k, S, 2, rule=None)
    assert e.win_rule() == "freestyle"
    assert _capi.lib().az_set_win_rule(e.h, 2) == -1 and _capi.lib().az_set_win_rule(e.h, -1) == -1 and e.win_rule() == "freestyle"
    with pytest.raises(ValueError):
        e.set_win_rule("renju")
    e.selfplay_begin(2, seed0=1)
    _refused(-6, e.set_win_rule, "exact")                        # an open episode
    e.selfplay_step(1000)
    e.selfplay_end()
    over = np.zeros(n * n, np.uint8)
    over[9:15] = 1                                               # X holds six in a row: an overline only
    over[[40, 42, 44, 60, 62, 64]] = 2
    run = over.copy()
    run[14] = 0                                                  # exactly five
    run[64] = 0
    _refused(-1, e.set_start_positions, over[None], [1], [64], match="already won.*freestyle")
    _refused(-1, e.set_start_positions, run[None], [1], [62], match="already won")
    e.set_win_rule("exact")
    _refused(-1, e.set_start_positions, run[None], [1], [62], match="already won.*exact")
    e.set_start_positions(over[None], [1], [64])                 # legal under EXACT
    assert e.start_positions() == 1
    _refused(-6, e.set_win_rule, "freestyle")                    # they were validated under the other rule
    e.set_win_rule("exact")                                      # no change: fine
    e.selfplay(2, seed0=3)
    rec, (nply, res) = e.records(), e.games()
    assert np.array_equal(rec["boards"][0], over)
    assert_replay(rec, nply, res, [(over, 1)], n, k, "exact", "overline start")
    e.clear_start_positions()
    e.set_win_rule("freestyle")
    assert e.win_rule() == "freestyle"
    e.close()


@pytest.mark.parametrize("n,k", [(5, 4), (9, 5)])
def test_rule_set_back_gives_the_default_engine(n, k, monkeypatch):
    """AZ_GRAPH on: an episode under EXACT, the rule set back, an episode under FREESTYLE -- a captured ply graph must not be
    replayed with the old rule: the records are the default engine's"""
    _clean_env(monkeypatch, AZ_GRAPH="1")
    S, G = 24, 4
    board, player, last, gaps = wr.opening(n, k)
    sd = gap_net(n, gaps, 2.0)
    outs = []
    for toggle in (False, True):
        e = engine(n, k, S, 4, sd, rule=None)
        e.set_start_positions(board[None], [player], [last])
        if toggle:
            e.selfplay(G, seed0=70)                              # freestyle: captures the graph
            e.clear_start_positions(); e.set_win_rule("exact"); e.set_start_positions(board[None], [player], [last])
            e.selfplay(G, seed0=70)
            exact = (e.records(), e.games())
            e.clear_start_positions(); e.set_win_rule("freestyle"); e.set_start_positions(board[None], [player], [last])
        c = e.selfplay(G, seed0=70)
        outs.append((e.records(), e.games(), {key: c[key] for key in ("simulations", "expansions", "terminal_hits")}))
        e.close()
    a, b = outs
    for key in a[0]:
        assert a[0][key].tobytes() == b[0][key].tobytes(), key
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]
    assert not np.array_equal(exact[1][0], a[1][0]) or exact[0]["actions"].tobytes() != a[0]["actions"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the Python seams
# ---------------------------------------------------------------------------------------------------------------------
def test_python_seams_carry_the_rule():
    """MCTS.run / run_many read the rule from the state (controller-backed and plain-callable evaluators alike); SelfPlayManager
    and ModelEvaluator set it on their cached engines, clearing start positions that were validated under the other rule"""
    import torch
    from alphazero_piskvorky_amd import constants, net
    from alphazero_piskvorky_amd.controller import NeuralNetworkController, make_policy_value_fn
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator
    from alphazero_piskvorky_amd.games import Gomoku
    from alphazero_piskvorky_amd.mcts import MCTS
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    n, k, S = 5, 4, S1
    assert (constants.BOARD_SIZE, constants.WIN_LENGTH) == (n, k)
    board, player, last, gap = wr.gap_position(n, k)
    sd = gap_net(n, [gap], 1.0)                                  # a mild pull: the visits, not only W, tell the rules apart
    m = net.GomokuNet(board_size=n)
    m.load_state_dict({key: torch.tensor(v) for key, v in sd.items()})
    ctl = NeuralNetworkController(m.eval(), device="cuda:0")

    def state(rule):
        g = Gomoku(n, k, win_rule=rule)
        g.cells = board.copy()
        g.current_player, g.last_action = "X", (last // n, last % n)
        return g

    want = {}
    for rule in wr.RULES:
        e = engine(n, k, S, 1, sd, rule=rule)
        want[rule] = e.search(board, player, last, 1.0, None, 0.25)["N"].reshape(n, n)
        e.close()
    assert not np.array_equal(want["exact"], want["freestyle"])
    mcts = MCTS(make_policy_value_fn(ctl), S, C_PUCT)
    ev = NetEval(n, k, sd, constant=True)
    plain = MCTS(lambda s: (ev(s.cells, s.player_code(), s.last_index())[0].reshape(n, n), 0.0), S, C_PUCT)
    for rule in ("exact", "freestyle", "exact"):                 # one cached engine, set on reuse
        for searcher in (mcts, plain):
            searcher.run(state(rule), 1.0)
            assert np.array_equal(searcher.last_visits, want[rule]), rule
        out = mcts.run_many([state(rule), state(rule)], 1.0)
        assert len(out) == 2 and np.array_equal(mcts.last_visits[0], want[rule]) and np.array_equal(mcts.last_visits[1], want[rule])
    with pytest.raises(ValueError, match="win rule"):
        mcts.run_many([state("exact"), state("freestyle")], 1.0)
    ev.close()
    # the managers: an opening with gap patterns as start position, first under EXACT, then the same manager back on freestyle
    ob, opl, ola, _ = wr.opening(n, k)
    mgr = SelfPlayManager(ctl, "cuda:0", mcts_params={"num_simulations": 24, "c_puct": C_PUCT}, concurrent_games=4, seed=3,
                          start_positions=(ob[None], [opl], [ola]), win_rule="exact")
    for rule in ("exact", "freestyle"):
        mgr.win_rule = rule
        mgr.generate_self_play(4)
        eng = mgr._engine
        assert eng.win_rule() == rule and eng.start_positions() == 1
        assert_replay(eng.records(), *eng.games(), [(ob, opl)], n, k, rule, f"manager {rule}")
    arena = ModelEvaluator(device="cuda:0", seed=5, win_rule="exact", start_positions=(ob[None], [opl], [ola]))
    arena.evaluate(ctl, ctl, num_games=4)
    assert arena._engine.win_rule() == "exact"
    arena.win_rule = "freestyle"
    arena.evaluate(ctl, ctl, num_games=4)
    assert arena._engine.win_rule() == "freestyle"
