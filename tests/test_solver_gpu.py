"""az_set_solver on the GPU, against the numpy restatement in tests/solver.py (which with the option off is the oracle's search
and whose proven statuses are minimax values, tests/test_solver_cpu.py).  The restatement's evaluator is the engine's own
az_net_eval, so every comparison is exact: integer equality for visits, statuses and actions, == on the float64 W and on the
float32 priors.  pi and the action are the restatement of mcts.py:144-177 (tests/forced.py, held to the engine exactly by
tests/test_forced_playouts_gpu.py) applied to the counts az_solver_counts returns for the engine's own visits and statuses,
and az_solver_counts in turn equals the rule's definition on the CPU.

Boards up to 7x7 run the persistent LDS-tree kernel with the solver on as with it off (az_get_persistent > 0); the cases at
3x3, 4x4, 5x5 and 7x7 run it, and again the lock-step kernels under AZ_PERSIST=0, both against the same restatement."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import solver as sv
from tests import ties
from tests.test_playout_cap_cpu import np_full
from tests.util import build_weights, load

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi

C_PUCT = 2.0
SIZES = ((5, 4), (7, 4), (9, 5), (15, 5))
S1 = 64
REC_KEYS = ("boards", "movers", "lasts", "actions", "pis", "visits", "z")
SWITCHES = ("AZ_GRAPH", "AZ_PROFILE_EVENTS", "AZ_PERSIST", "AZ_COMPACT", "AZ_VL_FORCE")


# ---------------------------------------------------------------------------------------------------------------------
# nets, evaluators, positions
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(n, tag):
    """(weights for the engine, model kind)"""
    if tag == "resnet_ckpt":
        z = load("resnet_ckpt_5.npz")
        return {k[3:]: z[k] for k in z.files if k.startswith("w__")}, "resnet"
    if tag == "uniform":
        return ties.constant_state_dict(n, np.zeros(n * n, np.float32), 0.0), "plain"
    if tag == "ends":                                    # crafted B: logit 6.0 on the two ends of the opponent's open line
        lg = np.zeros(n * n, np.float32)
        lg[list(sv.crafted_b(n, 5 if n > 5 else 4)[3])] = 6.0
        return ties.constant_state_dict(n, lg, 0.0), "plain"
    return build_weights(n), "plain"


def engine(n, k, S, slots, tag="seeded", solver=True, deep=False, **kw):
    sd, model = weights(n, tag)
    e = az.Engine(n, k, S, slots, log_table=orc.numpy_log_table(S), c_puct=C_PUCT, model=model, deep=deep, **kw)
    e.load_weights(sd, 0)
    if solver:
        e.set_solver(True)
        assert e.solver()
    return e


class NetEval:
    """evaluate(board, player, last) through the engine's az_net_eval, every position once; constant nets are evaluated once"""
    _memo = {}

    def __init__(self, n, k, tag):
        self.n, self.k, self.tag = n, k, tag
        self.memo = NetEval._memo.setdefault((n, tag), {})
        self.eng = None

    def __call__(self, board, player, last):
        key = () if self.tag in ("uniform", "ends") else (bytes(board), int(player), int(last))
        if key not in self.memo:
            if self.eng is None:
                self.eng = engine(self.n, self.k, 1, 1, self.tag, solver=False)
            _, P, v = self.eng.net_eval(np.asarray(board, np.uint8)[None], [player], [last])
            self.memo[key] = (P[0].copy(), float(v[0]))
        return self.memo[key]

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None


@functools.lru_cache(maxsize=None)
def positions(n, k):
    """the empty board and two mid-game positions, each with its Dirichlet sample, uniform and temperature; 5x5 adds a late one"""
    out = []
    for i, (stones, seed) in enumerate(((0, 1), (6, 2), (11, 3)) + (((17, 4),) if n == 5 else ())):
        board, player, last = sv.random_position(n, k, stones, seed)
        rs = np.random.RandomState(1000 * n + i)
        noise = rs.dirichlet([0.3] * int((board == 0).sum()))
        out.append(dict(board=board, player=player, last=last, noise=noise, u=float(rs.random_sample()), T=(1.0, 0.5, 1e-9, 1.0)[i]))
    return tuple(out)


def expect_pi(r, st, p, S):
    legal = np.flatnonzero(p["board"] == 0)
    counts = _capi.solver_counts(r["N"][legal], st[legal])
    return sv.pi_action(counts, p["board"], p["T"], p["u"], orc.numpy_log_table(S))


def assert_search(r, proof, want, p, S, what):
    edges, root = proof
    assert np.array_equal(r["N"], want["N"]), f"{what}: visits"
    assert np.array_equal(r["W"], want["W"]), f"{what}: W"
    assert np.array_equal(r["P"], want["P"]), f"{what}: priors"
    assert edges.dtype == np.int8 and np.array_equal(edges, want["st"]), f"{what}: statuses"
    assert int(root) == want["root"], f"{what}: root status"
    pi, a = expect_pi(r, edges, p, S)
    assert r["pi"].dtype == np.float32 and np.array_equal(r["pi"], pi), f"{what}: pi"
    assert int(r["action"]) == a, f"{what}: action"


def batch(e, ps, noised=True):
    rb = e.search_batch(np.stack([p["board"] for p in ps]), [p["player"] for p in ps], [p["last"] for p in ps],
                        np.array([p["T"] for p in ps]), [p["noise"] for p in ps] if noised else None, [p["u"] for p in ps])
    edges, roots = e.last_proof()
    return [({key: val[i] for key, val in rb.items()}, (edges[i], roots[i])) for i in range(len(ps))]


# ---------------------------------------------------------------------------------------------------------------------
# 1. single searches against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _clean_env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        if value is not None:
            monkeypatch.setenv(name, value)


@pytest.mark.parametrize("noised", [True, False], ids=["noise", "no-noise"])
@pytest.mark.parametrize("n,k,persist", [(5, 4, None), (7, 4, None), (9, 5, None), (15, 5, None), (5, 4, "0"), (7, 4, "0")],
                         ids=["5x5", "7x7", "9x9", "15x15", "5x5-lockstep", "7x7-lockstep"])
def test_single_searches_equal_the_restatement(n, k, persist, noised, monkeypatch):
    """5x5 and 7x7: one cell per lane, the persistent kernel (az_search one game per workgroup, az_search_batch two at 5x5; 7x7
    is its largest board) and, under AZ_PERSIST=0, the lock-step kernels; 9x9: two cells per lane; 15x15: four.  S = 64,
    T in {1, 0.5, 1e-9}."""
    _clean_env(monkeypatch, AZ_PERSIST=persist)
    ev = NetEval(n, k, "seeded")
    e = engine(n, k, S1, 4)
    ps = positions(n, k)
    proven = 0
    for i, (p, (rb, pb)) in enumerate(zip(ps, batch(e, ps, noised))):
        want = sv.search(ev, n, k, S1, p["board"], p["player"], p["last"], p["noise"] if noised else None, True, C_PUCT)
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"] if noised else None, p["u"])
        assert (e.persistent() > 0) == (n <= 7 and persist is None)
        assert_search(r, e.last_proof(), want, p, S1, f"{n}x{n} position {i} az_search")
        assert_search(rb, pb, want, p, S1, f"{n}x{n} position {i} az_search_batch")
        assert r["N"].sum() == S1
        proven += int(want["st"].any())
    if n == 5:
        assert proven > 0           # the late 5x5 position proves edges: the comparison of the statuses is not all zeros
    e.close(); ev.close()


@pytest.mark.parametrize("option", ["plain", "eval-cache"])
def test_resnet_checkpoint_5x5(option):
    """the ResidualBlock checkpoint; with the evaluation cache the searches after the first hit it"""
    n, k = 5, 4
    ev = NetEval(n, k, "resnet_ckpt")
    e = engine(n, k, S1, 4, "resnet_ckpt")
    if option == "eval-cache":
        e.set_eval_cache(1 << 10)
    ps = positions(n, k)
    for rep in range(2 if option == "eval-cache" else 1):
        for i, p in enumerate(ps):
            want = sv.search(ev, n, k, S1, p["board"], p["player"], p["last"], p["noise"], True, C_PUCT)
            r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
            assert_search(r, e.last_proof(), want, p, S1, f"resnet {option} position {i} pass {rep}")
    e.close(); ev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the crafted positions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,S", [(5, 4, 64), (9, 5, 128), (15, 5, 256)])
def test_crafted_a_plays_the_winning_cell(n, k, S):
    """root WIN with a single WIN cell; at T -> 0 pi is exactly one-hot and u = 0.0 and 0.999 both play it.  At T = 1 the
    unchanged temperature path leaves every emptied cell log(0 + 1e-8), a share of pi below float32's spacing at 1."""
    board, player, last, win = sv.crafted_a(n, k)
    ev = NetEval(n, k, "uniform")
    want = sv.search(ev, n, k, S, board, player, last, None, True, C_PUCT)
    assert want["root"] == sv.WIN and np.flatnonzero(want["st"]).tolist() == [win]
    e = engine(n, k, S, 1, "uniform")
    for T, u in ((1e-9, 0.0), (1e-9, 0.999), (1.0, 0.5), (1.0, 0.999)):
        p = dict(board=board, T=T, u=u)
        r = e.search(board, player, last, T, None, u)
        edges, root = e.last_proof()
        assert_search(r, (edges, root), want, p, S, f"{n}x{n} crafted A T={T} u={u}")
        assert root == _capi.PROOF_WIN and r["action"] == win and r["pi"][win] == 1.0
        assert (np.count_nonzero(r["pi"]) == 1) if T < 1e-7 else (np.delete(r["pi"], win).max() < 1e-8)
        assert e.solver_stops() == 0                     # the winning move is a real terminal every time, never a stop
    e.close(); ev.close()


@pytest.mark.parametrize("n,k,persist", [(5, 4, None), (5, 4, "0"), (9, 5, None)], ids=["5x5-persistent", "5x5-lockstep", "9x9"])
def test_leaf_symmetry_on_the_fixture_net_equals_the_oracle(n, k, persist, monkeypatch):
    """random-symmetry leaf evaluation next to the solver, on a position where nothing gets proven: the search is then the plain
    one, which the oracle restates with the symmetry of every evaluation (orc_cfg.leaf_sym), bit for bit -- and it is not the
    search without the symmetry, so the de-mapping of the logits in the SOLVER kernels is what is compared"""
    _clean_env(monkeypatch, AZ_PERSIST=persist)
    p = positions(n, k)[1]
    o, net = orc.Oracle(n, k, S1, c_puct=C_PUCT, leaf_sym=True), orc.Net(n, build_weights(n))
    want = o.search(net, p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    e = engine(n, k, S1, 1)
    plain = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    e.set_leaf_symmetry(True)
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    edges, root = e.last_proof()
    assert (e.persistent() > 0) == (n == 5 and persist is None)
    assert not edges.any() and root == 0
    for key in ("N", "W", "P"):
        assert np.array_equal(r[key], want[key]), key
    assert int(r["action"]) == int(want["action"]) and np.array_equal(r["pi"], want["pi"])
    assert not np.array_equal(r["W"], plain["W"])
    e.close()


def test_leaf_symmetry_with_a_symmetric_net():
    """random-symmetry leaf evaluation next to the solver, with the one net whose answers no symmetry changes (constant
    logits): the search is the restatement's.  (With any other net the softmax is summed in another order under a symmetry,
    which az_net_eval cannot restate bit for bit.)"""
    n, k, S = 9, 5, 128
    board, player, last, win = sv.crafted_a(n, k)
    ev = NetEval(n, k, "uniform")
    want = sv.search(ev, n, k, S, board, player, last, None, True, C_PUCT)
    e = engine(n, k, S, 1, "uniform")
    e.set_leaf_symmetry(True)
    r = e.search(board, player, last, 1e-9, None, 0.3)
    assert_search(r, e.last_proof(), want, dict(board=board, T=1e-9, u=0.3), S, "leaf symmetry")
    assert r["action"] == win
    e.close(); ev.close()


@pytest.mark.parametrize("n,k,S", [(5, 4, 100), (9, 5, 200), (15, 5, 512)])
def test_crafted_b_is_a_proven_loss(n, k, S):
    board, player, last, ends = sv.crafted_b(n, k)
    ev = NetEval(n, k, "ends")
    info = {}
    want = sv.search(ev, n, k, S, board, player, last, None, True, C_PUCT, info=info)
    legal = board == 0
    assert want["root"] == sv.LOSS and (want["st"][legal] == sv.LOSS).all()
    e = engine(n, k, S, 1, "ends")
    p = dict(board=board, T=1.0, u=0.5)
    r = e.search(board, player, last, 1.0, None, 0.5)
    edges, root = e.last_proof()
    assert_search(r, (edges, root), want, p, S, f"{n}x{n} crafted B")
    assert root == _capi.PROOF_LOSS and np.array_equal(_capi.solver_counts(r["N"][legal], edges[legal]), r["N"][legal])
    assert (e.persistent() > 0) == (n == 5)
    assert e.solver_stops() == info["stops"] > 0          # once every move is refuted the simulations end on the proven edges
    e.close(); ev.close()


def test_crafted_b_value_and_resignation():
    """two arena games from crafted B (the second with the colours exchanged), both nets the same: the first ply's root is a
    proven LOSS, its value exactly -1, and with resignation on the mover resigns at that very ply"""
    n, k, S = 5, 4, 100
    board, player, last, _ = sv.crafted_b(n, k)
    sd, _ = weights(n, "ends")
    for resign in (False, True):
        e = engine(n, k, S, 2, "ends")
        e.load_weights(sd, 1)
        e.set_start_positions(board[None], [player], [last])
        if resign:
            e.set_resign(0.9)
        a = e.arena(2, seed0=5)
        proofs, values, rec = e.proofs(), e.values(), e.records()
        first = np.concatenate([[0], np.cumsum(a["nply"])])[:2]
        assert (proofs[first] == _capi.PROOF_LOSS).all() and (values[first] == -1.0).all()
        assert np.array_equal(rec["boards"][first[0]], board)
        if resign:
            assert a["nply"].tolist() == [1, 1] and a["results"].tolist() == [2, 1]
            assert ((a["actions"] >= 0).sum(axis=1) == 1).all()
        else:
            assert (a["nply"] >= 2).all() and a["results"].tolist() == [2, 1]     # the open line wins anyway
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. option off
# ---------------------------------------------------------------------------------------------------------------------
def test_option_off_again_is_byte_identical():
    n, k, S, G = 5, 4, 32, 6
    outs = []
    for toggle in (False, True):
        e = engine(n, k, S, 4, solver=False)
        if toggle:
            e.set_solver(True)
            e.search(*[positions(n, k)[3][key] for key in ("board", "player", "last")], 1.0, None, 0.5)
            e.set_solver(False)
            assert not e.solver()
            with pytest.raises(_capi.AzError):
                e.last_proof()
        p = positions(n, k)[3]
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        pers = e.persistent()
        c = e.selfplay(G, seed0=77)
        outs.append((r, e.records(), e.values(), e.games(), pers, e.persistent(), {key: c[key] for key in ("simulations", "expansions", "terminal_hits")}))
        if toggle:
            with pytest.raises(_capi.AzError):
                e.proofs()
        e.close()
    a, b = outs
    assert a[4] == b[4] > 0 and a[5] == b[5] > 0 and a[6] == b[6]            # the persistent kernel is back
    for key in a[0]:
        assert np.array_equal(a[0][key], b[0][key]) and np.asarray(a[0][key]).tobytes() == np.asarray(b[0][key]).tobytes(), key
    for key in a[1]:
        assert a[1][key].tobytes() == b[1][key].tobytes(), key
    assert a[2].tobytes() == b[2].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. deep engine
# ---------------------------------------------------------------------------------------------------------------------
def test_deep_engine():
    """S = 1100 > 1024: the DEEP instantiation of the tree step (sqrt table from HBM, 16-bit visit counts)"""
    n, k, S = 5, 4, 1100
    p = positions(n, k)[3]
    ev = NetEval(n, k, "seeded")
    want = sv.search(ev, n, k, S, p["board"], p["player"], p["last"], p["noise"], True, C_PUCT)
    e = engine(n, k, S, 1, deep=True)
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    assert_search(r, e.last_proof(), want, p, S, "deep 5x5")
    assert r["N"].sum() == S and want["st"].any()
    e.close(); ev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. az_search_batch = a loop of az_search
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(5, 4), (9, 5)])
def test_batch_equals_a_loop_of_searches(n, k):
    """eight positions on four slots: two waves"""
    ps = []
    for i in range(8):
        board, player, last = sv.random_position(n, k, (3, 8, 13, 17)[i % 4] if n == 5 else (4, 10, 20, 30)[i % 4], 40 + i)
        rs = np.random.RandomState(500 + i)
        ps.append(dict(board=board, player=player, last=last, noise=rs.dirichlet([0.3] * int((board == 0).sum())),
                       u=float(rs.random_sample()), T=(1.0, 0.5, 1e-9, 1.0)[i % 4]))
    e = engine(n, k, S1, 4)
    got = batch(e, ps)
    for i, (p, (rb, (eb, rootb))) in enumerate(zip(ps, got)):
        r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        edges, root = e.last_proof()
        for key in r:
            assert np.array_equal(r[key], rb[key]), (i, key)
        assert np.array_equal(edges, eb) and root == rootb, i
        assert not edges[p["board"] != 0].any()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. whole games
# ---------------------------------------------------------------------------------------------------------------------
def assert_games(e, ev, n, k, S, G, seed0, cap=None, what=""):
    rec, (nply, res), values, proofs = e.records(), e.games(), e.values(), e.proofs()
    off, proven = 0, 0
    for g in range(G):
        want = sv.selfplay_game(ev, n, k, S, seed0 + g, True, cap, np_full)
        L = int(nply[g])
        assert L == want["nply"] and int(res[g]) == want["result"], f"{what} game {g}: length / result"
        for key in REC_KEYS:
            assert np.array_equal(rec[key][off:off + L], want[key]), f"{what} game {g}: {key}"
        assert np.array_equal(values[off:off + L], want["values"]), f"{what} game {g}: values"
        assert np.array_equal(proofs[off:off + L], want["proofs"]), f"{what} game {g}: proofs"
        exact = want["proofs"] != 0
        assert np.isin(want["values"][exact], (-1.0, 0.0, 1.0)).all()
        proven += int(exact.sum())
        off += L
    assert off == len(values) == len(proofs)
    return proven


@pytest.mark.parametrize("n,k,S,G", [(5, 4, 100, 4), (9, 5, 64, 1)])
def test_whole_games_ply_by_ply(n, k, S, G):
    ev = NetEval(n, k, "seeded")
    e = engine(n, k, S, 4)
    c = e.selfplay(G, seed0=300)
    assert (e.persistent() > 0) == (n == 5) and c["simulations"] == S * c["plies"] and c["expansions"] + c["terminal_hits"] == c["simulations"]
    proven = assert_games(e, ev, n, k, S, G, 300, what=f"{n}x{n}")
    if n == 5:
        assert proven > 0
    e.close(); ev.close()


def test_whole_games_under_the_playout_cap():
    n, k, S, G, fast, permille = 5, 4, 100, 4, 24, 300
    ev = NetEval(n, k, "seeded")
    e = engine(n, k, S, 4)
    e.set_playout_cap(fast, permille / 1000.0, export_full_only=False)
    e.selfplay(G, seed0=300)
    assert_games(e, ev, n, k, S, G, 300, cap=(fast, permille), what="capped")
    e.close(); ev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. minimax on the GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,S", [(3, 3, 100), (4, 3, 300)])
def test_every_proven_record_is_the_minimax_value(n, k, S):
    G = 32
    e = engine(n, k, S, G)
    e.selfplay(G, seed0=900)
    rec, proofs, values = e.records(), e.proofs(), e.values()
    memo, proven = {}, 0
    for i in np.flatnonzero(proofs):
        want = sv.minimax(rec["boards"][i].copy(), int(rec["movers"][i]), n, k, memo)
        assert proofs[i] == want, (i, rec["boards"][i], proofs[i], want)
        assert values[i] == sv.VALUE[want]
        proven += 1
    assert proven > 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. arena
# ---------------------------------------------------------------------------------------------------------------------
def test_arena_plays_the_immediate_win():
    """a visited cell that makes the line is marked WIN at its first visit, the root is WIN from then on and every later
    simulation lands on it: N' holds nothing else, the ply plays it"""
    n, k, S, G = 5, 4, 64, 8
    e = engine(n, k, S, G)
    e.load_weights(build_weights(n, seed=4321), 1)
    a = e.arena(G, seed0=11)
    rec, proofs, values = e.records(), e.proofs(), e.values()
    assert len(proofs) == int(a["nply"].sum())
    seen = 0
    for i in range(len(proofs)):
        board, mover = rec["boards"][i], int(rec["movers"][i])
        imm = []
        for c in np.flatnonzero(board == 0):
            b2 = board.copy()
            b2[c] = mover
            if sv.wins_through(b2, int(c), n, k):
                imm.append(int(c))
        visited = [c for c in imm if rec["visits"][i][c] > 0]
        if visited:
            assert proofs[i] == _capi.PROOF_WIN and values[i] == 1.0 and int(rec["actions"][i]) == visited[0], (i, imm, visited)
            assert rec["pis"][i][visited[0]] == 1.0
            seen += 1
    assert seen > 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. launch paths
# ---------------------------------------------------------------------------------------------------------------------
def _episode(n, k, S, G, capped):
    e = engine(n, k, S, 4)
    if capped:
        e.set_playout_cap(S // 4, 0.4, export_full_only=False)
    e.selfplay(G, seed0=1234)
    out = (e.records(), e.values(), e.proofs(), e.games(), e.solver_stops(), e.persistent())
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def default_episode(n, k, S, G, capped):
    return _episode(n, k, S, G, capped)


@pytest.mark.parametrize("switch", ["AZ_PERSIST", "AZ_GRAPH", "AZ_COMPACT"])
@pytest.mark.parametrize("n,k,S,G", [(5, 4, 48, 6), (9, 5, 32, 5)])
def test_launch_paths_give_identical_episodes(n, k, S, G, switch, monkeypatch):
    """AZ_PERSIST=0: the lock-step kernels against the persistent one (5x5).  AZ_COMPACT=0 on an episode under the playout cap,
    where the compaction is the three-way partition of k_refill."""
    capped = switch == "AZ_COMPACT"
    _clean_env(monkeypatch)
    want = default_episode(n, k, S, G, capped)
    assert (want[5] > 0) == (n == 5 and not capped)
    monkeypatch.setenv(switch, "0")
    got = _episode(n, k, S, G, capped)
    assert got[5] == (0 if switch == "AZ_PERSIST" else want[5]) and got[4] == want[4]
    for key in want[0]:
        assert np.array_equal(got[0][key], want[0][key]), (switch, key)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert all(np.array_equal(x, y) for x, y in zip(got[3], want[3]))


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _refused(fn, *args):
    with pytest.raises(_capi.AzError) as ex:
        fn(*args)
    assert "(-1)" in str(ex.value), str(ex.value)          # AZ_ERR_INVALID


def test_refused_combinations_in_both_orders():
    n, k, S = 5, 4, 32
    p = positions(n, k)[1]
    others = (("subtree reuse", lambda e: e.set_subtree_reuse(True), lambda e: e.set_subtree_reuse(False)),
              ("virtual loss", lambda e: e.set_virtual_loss(4), lambda e: e.set_virtual_loss(1)),
              ("forced playouts", lambda e: e.set_forced_playouts(2.0), lambda e: e.set_forced_playouts(0.0)),
              ("gumbel", lambda e: e.set_gumbel(8), lambda e: e.set_gumbel(0)))
    e = engine(n, k, S, 2, solver=False)
    for name, on, off in others:
        e.set_solver(True)
        _refused(on, e)                                      # the solver first
        e.set_solver(False)
        on(e)
        _refused(e.set_solver, True)                         # the other option first
        assert not e.solver()
        off(e)
    e.set_solver(True)
    _refused(lambda: e.search_callback(p["board"], p["player"], p["last"], 1.0, lambda c, pl, la: (np.full(n * n, 1.0 / (n * n), np.float32), 0.0)))
    assert e.solver()
    # the engine still works, with the solver on
    ev = NetEval(n, k, "seeded")
    want = sv.search(ev, n, k, S, p["board"], p["player"], p["last"], p["noise"], True, C_PUCT)
    r = e.search(p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
    assert_search(r, e.last_proof(), want, p, S, "after the refusals")
    e.close(); ev.close()
    s = az.Engine(n, k, S, 2, synthetic=True, log_table=orc.numpy_log_table(S))
    _refused(s.set_solver, True)
    assert s.search(p["board"], p["player"], p["last"], 1.0, None, 0.5)["N"].sum() == S
    s.close()


def test_the_batched_external_evaluator_is_refused_in_both_orders():
    """the choice stated in include/az_engine.h: az_set_external_evaluator and the solver do not combine"""
    import torch
    n, k, S = 5, 4, 16
    e = engine(n, k, S, 2)
    planes = torch.zeros((2, 4, n, n), dtype=torch.float32, device="cuda")
    policy = torch.zeros((2, n * n), dtype=torch.float32, device="cuda")
    value = torch.zeros(2, dtype=torch.float32, device="cuda")
    args = (planes.data_ptr(), policy.data_ptr(), value.data_ptr(), 2, lambda net, count: None)
    _refused(e.set_external_evaluator, *args)
    e.set_solver(False)
    e.set_external_evaluator(*args)
    _refused(e.set_solver, True)
    e.clear_external_evaluator()
    e.set_solver(True)
    p = positions(n, k)[0]
    assert e.search(p["board"], p["player"], p["last"], 1.0, None, 0.5)["N"].sum() == S
    e.close()
