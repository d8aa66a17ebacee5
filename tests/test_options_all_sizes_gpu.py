"""Every search option and every net kernel shape on every board size the all-sizes tests visit (3, 4, 6, 7, 8, 10..14; 5, 9
and 15 have their dedicated files): engine == oracle bit for bit (np.array_equal, no tolerances), or == the same engine with the
option off where the oracle has no such notion (the evaluation cache).

The kernels are templates on the board size and their geometry changes with it in steps: cells per lane of a tree row
(TreeGeo<N>::CPL: 1 up to 8x8 -- where a row fills all 64 lanes --, 2 for 9..11, 3 for 12 and 13, 4 from 14), boards per trunk
workgroup (NetGeo<N>::G: 4 below 8x8, 2 for 8..11, 1 from 12), games per workgroup of the persistent kernel (2 up to 5x5, 1 at 6x6
and 7x7, none above) and the tile subsets of k_search<.., TS = true> (folded away at 3x3, disjoint at 4x4, one shared tile at 5x5).
Which case launches which instantiation:

  throughput shapes        k_fc<G, 2, 4>, the fused trunks over 42 / 21 / 83 workgroups with a ragged last board group, and the
                           tile-split trunks (k_tile, k_tile_res<N, 0..3>) on the short last pass
  virtual loss             k_step_vl<N> (synthetic and net), duplicate pending leaves at every CPL
  subtree reuse            k_move<N> / k_reuse compaction; on the small sizes the persistent kernel with ROWE = n*n and the
                           tile-subset variant k_search<N, 2, false, true, RES> for both nets
  evaluation cache         k_root_cache<N>, cache_lookup / cache_hit_store / cache_insert in k_step and inside k_search
  arena                    two nets, one game per workgroup of the persistent kernel on the small sizes
  search_batch             k_set_positions<N>, k_gather_roots<N> on every 64-cell word of a row, two lanes, three waves
  deep                     the DEEP k_step<N> and k_step_vl<N> with the in-flight bytes [B][R][RW]
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_all_sizes_gpu import SIZES, _positions

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.net import fold_resnet_state_dict
from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict, synthetic_state_dict

SMALL = [(3, 3), (4, 3), (6, 4), (7, 4)]                 # the sizes of SIZES that the persistent kernel serves
SMALL_AND_5 = [(3, 3), (4, 3), (5, 4), (6, 4), (7, 4)]   # 5x5 too: the three tile-subset geometries side by side
RECORD_KEYS = ("actions", "boards", "movers", "lasts", "visits", "pis", "z")
SEARCH_KEYS = ("N", "W", "P", "pi")


def _persist_gp(n):
    return 2 if n <= 5 else (1 if n <= 7 else 0)


def _weights(n, model, seed=None):
    """(state dict for Engine.load_weights, the oracle's net)"""
    if model == "resnet":
        sd = synthetic_resnet_state_dict(n) if seed is None else synthetic_resnet_state_dict(n, seed)
        return sd, orc.Net(n, resnet_tensors=fold_resnet_state_dict(sd))
    sd = synthetic_state_dict(n) if seed is None else synthetic_state_dict(n, seed)
    return sd, orc.Net(n, sd)


def _oracle_games(o, onet, n, G, seed0, cut=0):
    """the oracle's games seed0 .. seed0 + G - 1 (its scratch is per thread: one Oracle serves many threads)"""
    def one(g):
        noise, us = orc.selfplay_tape(seed0 + g, n, maxply=cut or None)
        return o.selfplay_game(onet, noise, us, maxply=cut or None)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(one, range(G)))


def _totals(games):
    tot = dict(expansions=0, terminal_hits=0, depth_sum=0, sims=0, root_evals=0, dup_sims=0, plies=0)
    for r in games:
        for key in r["counters"]:
            tot[key] += r["counters"][key]
        tot["plies"] += r["nply"]
    return tot


def _assert_games(e, games, what, cut=0):
    """the engine's last episode against the oracle's games, record by record"""
    rec = e.records(); nply, res = e.games()
    assert len(nply) == len(games)
    off = 0
    for g, r in enumerate(games):
        L = int(nply[g]); sl = slice(off, off + L)
        assert L == r["nply"] and int(res[g]) == r["result"], f"{what}: game {g}: length or result"
        for key in RECORD_KEYS:
            assert np.array_equal(rec[key][sl], r[key]), f"{what}: game {g}: {key} differs from the oracle"
        off += L
    assert off == len(rec["actions"])
    return rec


def _assert_work(c, tot, what):
    got = (c["expansions"], c["terminal_hits"], c["depth_sum"], c["duplicate_leaves"], c["simulations"], c["root_evals"], c["plies"])
    want = (tot["expansions"], tot["terminal_hits"], tot["depth_sum"], tot["dup_sims"], tot["sims"], tot["root_evals"], tot["plies"])
    assert got == want, f"{what}: expansions, terminal_hits, depth_sum, duplicate_leaves, simulations, root_evals, plies {got} != {want}"


def _assert_search(r, ro, what):
    for key in SEARCH_KEYS:
        assert np.array_equal(r[key], ro[key]), f"{what}: {key} differs from the oracle"
    assert int(r["action"]) == int(ro["action"]), f"{what}: action"


def _same_records(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{what}: {key}"


def _nearly_full(n, k, empty, rs):
    """The filling colour(r, c) = 1 + ((r // 2 + c) % 2): its longest run in any direction is 2, so no position on the way has a
    winner for k >= 3 and one further stone makes a run of 3 at most.  `empty` cells are left out so that the stone counts stay
    those of alternating play, and the rest is played interleaved; the oracle's rules confirm that the position is undecided."""
    cells = np.arange(n * n)
    colour = 1 + ((cells // n // 2 + cells % n) % 2)
    xs, os_ = list(rs.permutation(cells[colour == 1])), list(rs.permutation(cells[colour == 2]))
    d = len(xs) - len(os_)
    assert d in (0, 1)
    a = empty // 2 + (empty % 2 and d)            # X stones left out; afterwards #X - #O is 0 or 1 again
    xs, os_ = xs[a:], os_[empty - a:]
    assert len(xs) - len(os_) in (0, 1)
    acts = [int(c) for pair in zip(xs, os_) for c in pair] + ([int(xs[-1])] if len(xs) > len(os_) else [])
    rc, term, board, pl, res = orc.Oracle(n, k, 1).replay(acts)
    assert rc == 0 and res == 0 and not term.any() and int((board == 0).sum()) == empty
    return board, int(pl), acts[-1]


def _random_positions(rs, n, k, count):
    """undecided positions reached by legal play (the oracle's rules decide)"""
    o = orc.Oracle(n, k, 1)
    nn = n * n
    out = []
    while len(out) < count:
        acts = [int(a) for a in rs.permutation(nn)[:int(rs.randint(0, nn))]]
        rc, term, board, pl, res = o.replay(acts)
        if rc == 0 and res == 0 and not term.any() and (board == 0).any():
            out.append((board.copy(), int(pl), acts[-1] if acts else -1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# A. net kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", SIZES)
def test_throughput_fc_and_many_workgroup_trunks_bit_exact(n, k, monkeypatch):
    """83 slots, 2 * 83 + 34 positions: three passes of az_net_eval.  fc_t (az_kernels.hip) chooses the FC shape from the lane's
    item count, (83 + 15) / 16 = 6 row tiles > 4, not from the boards of the pass: ALL three passes run the throughput shape
    k_fc<G, 2, 4> (the latency shape k_fc<G, 1, 1> is what the 9-slot engines of test_forward_both_models_bit_exact run).  What
    the short last pass changes is the trunk: with AZ_SPLIT_MAX unset its 34 boards <= 64 take the tile-split kernels (k_tile /
    k_tile_res) over all 83 slots, 49 of them idle; the full passes, and every pass under AZ_SPLIT_MAX=0, take the fused trunk
    over ceil(83 / G) workgroups whose last board group is ragged for G = 2 and G = 4."""
    o = orc.Oracle(n, k, 1)
    slots, cnt = 83, 2 * 83 + 34
    boards, players, lasts = _positions(np.random.RandomState(1100 + n), n, cnt)
    planes = [o.encode(boards[i], int(players[i]), int(lasts[i])) for i in range(cnt)]
    for model in ("plain", "resnet"):
        sd, onet = _weights(n, model)
        with ThreadPoolExecutor(max_workers=8) as ex:
            want = list(ex.map(onet.eval, planes))
        for split in ("0", None):
            if split is None:
                monkeypatch.delenv("AZ_SPLIT_MAX", raising=False)
            else:
                monkeypatch.setenv("AZ_SPLIT_MAX", split)
            e = az.Engine(n, k, 4, slots, model=model)
            assert e.lanes() == 1
            e.load_weights(sd, 0)
            logits, P, v = e.net_eval(boards, players, lasts)
            e.close()
            for i, (ol, oP, ov) in enumerate(want):
                what = f"{model} AZ_SPLIT_MAX={split} n={n} board {i} (pass {i // slots})"
                assert np.array_equal(logits[i].view(np.uint32), ol.view(np.uint32)), f"{what}: logits"
                assert np.array_equal(P[i].view(np.uint32), oP.view(np.uint32)), f"{what}: P"
                assert v[i:i + 1].view(np.uint32)[0] == np.array([ov], np.float32).view(np.uint32)[0], f"{what}: value"


# ---------------------------------------------------------------------------------------------------------------------
# B.1 virtual loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", SIZES)
def test_virtual_loss_complete_synthetic_games(n, k):
    L, S, G = 32, 48, 3
    e = az.Engine(n, k, S, 3, synthetic=True, log_table=orc.numpy_log_table(S))
    e.set_virtual_loss(L)
    c = e.selfplay(G, seed0=21000 + 10 * n)
    games = _oracle_games(orc.Oracle(n, k, S, synthetic=True, virtual_loss=L), None, n, G, 21000 + 10 * n)
    _assert_games(e, games, f"{n}x{n} virtual loss {L}")
    _assert_work(c, _totals(games), f"{n}x{n} virtual loss {L}")
    assert c["simulations"] == S * c["plies"]
    e.close()


NEARLY_FULL_SIZES = [(n, k) for n, k in SIZES if k >= 4] + [(15, 5)]
NEARLY_FULL_NET = (12, 14)              # the real net as well: CPL 3 with one board per trunk workgroup, and CPL 4


@pytest.mark.parametrize("n,k", NEARLY_FULL_SIZES)
def test_virtual_loss_duplicate_leaves_on_nearly_full_boards(n, k):
    """2, 3, 5, 6 and 4 empty cells, 64 simulations in batches of 5 and of 32: the tree runs out of open leaves, so the simulations
    of a batch end on terminal leaves (the full board) and on leaves that are already pending.  The oracle's own expansion count
    (root included) says so: at most S / 2 wherever the tree is smaller than the batches -- every position in batches of 32 (the
    first batch finds `empty` open leaves, the second at most empty * (empty - 1): measured 3 to 29), and 2, 3 or 4 empty cells
    in batches of 5 (a tree of 5, 16 or 41 positions that can be expanded: measured 3, 7 to 10, 16 to 23).  Batches of 5 on 5 or 6
    empty cells are compared like the others but cannot meet that condition: 13 batches walk a tree of 206 or 1237 positions and
    the oracle expands 34 to 65 of them."""
    S, T = 64, 0.8
    rs = np.random.RandomState(21500 + n)
    pos = [(_nearly_full(n, k, empty, rs), rs.dirichlet([0.3] * empty), float(rs.random_sample())) for empty in (2, 3, 5, 6, 4)]
    for synthetic in ((True, False) if n in NEARLY_FULL_NET else (True,)):
        sd, onet = (None, None) if synthetic else _weights(n, "plain")
        for L in (5, 32):
            e = az.Engine(n, k, S, 2, synthetic=synthetic, log_table=orc.numpy_log_table(S))
            if not synthetic:
                e.load_weights(sd, 0)
            e.set_virtual_loss(L)
            o = orc.Oracle(n, k, S, synthetic=synthetic, virtual_loss=L)
            for (board, pl, last), noise, u in pos:
                ro = o.search(onet, board, pl, last, T, noise, u)
                what = f"{n}x{n} synthetic={synthetic} L={L}, {len(noise)} empty cells"
                print(f"{what}: the oracle expanded {ro['nexp']} leaves in {S} simulations")
                if L == 32 or len(noise) <= 4:
                    assert ro["nexp"] <= S // 2, f"{what}: {ro['nexp']} expansions: not a position that forces duplicates"
                r = e.search(board, pl, last, T, noise, u)
                _assert_search(r, ro, what)
                assert int(r["N"].sum()) == S
            e.close()


@pytest.mark.parametrize("n,k", SIZES)
def test_virtual_loss_real_net_games_cut_at_5_plies(n, k):
    """the logits row through k_step_vl's softmax at every CPL"""
    L, S, G, cut = 8, 48, 3, 5
    sd, onet = _weights(n, "plain")
    e = az.Engine(n, k, S, 3, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    e.set_virtual_loss(L)
    c = e.selfplay(G, seed0=21800 + 10 * n, max_plies=cut)
    games = _oracle_games(orc.Oracle(n, k, S, virtual_loss=L), onet, n, G, 21800 + 10 * n, cut)
    _assert_games(e, games, f"{n}x{n} virtual loss {L}, net")
    _assert_work(c, _totals(games), f"{n}x{n} virtual loss {L}, net")
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# B.2 subtree reuse
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", SIZES)
def test_subtree_reuse_complete_synthetic_games_with_refill(n, k):
    S, G = 48, 5
    e = az.Engine(n, k, S, 3, synthetic=True, log_table=orc.numpy_log_table(S))
    e.set_subtree_reuse(True)
    c = e.selfplay(G, seed0=22000 + 10 * n)
    games = _oracle_games(orc.Oracle(n, k, S, synthetic=True, reuse=True), None, n, G, 22000 + 10 * n)
    _assert_games(e, games, f"{n}x{n} reuse")
    tot = _totals(games)
    _assert_work(c, tot, f"{n}x{n} reuse")
    assert all((r["visits"].sum(axis=1) == S).all() for r in games)        # pi is still a distribution over S visits
    assert c["root_evals"] < c["plies"] and c["simulations"] < S * c["plies"]          # roots were retained and topped up
    e.close()


REUSE_C_PUCT = 0.3       # with the default 2.0 and the flat priors of a seeded net nearly nothing is carried from ply to ply


def _assert_carried(tot, S, what):
    """from the oracle alone: the retained subtrees really carry visits"""
    print(f"{what}: the oracle ran {tot['sims']} simulations for {tot['plies']} plies of {S}: {tot['sims'] / (S * tot['plies']):.3f}")
    assert tot["sims"] < 0.9 * S * tot["plies"], f"{what}: {tot['sims']} of {S * tot['plies']} simulations: nothing is carried"


# size: (seed of synthetic_state_dict, seed0).  Three games of five plies are a small sample and how much a seeded net concentrates
# its visits differs from size to size (the default net at 10x10 carries under 5 %), so net and games are chosen, from the oracle's
# output alone, where the oracle tops up at most 87 % of S per ply; _assert_carried holds them to the bar.  That bar is about the
# oracle and these inputs only: if it fails after a change to synthetic_state_dict or to the self-play tape, pick net seeds and
# seed0 values anew from the oracle's figures -- it says nothing about the engine.
REUSE_CUT_CASES = {8: (None, 22483), 10: (7, 22503), 11: (None, 22516), 12: (7, 22520), 13: (None, 22530), 14: (7, 22540)}


@pytest.mark.parametrize("n,k", [s for s in SIZES if s not in SMALL])
def test_subtree_reuse_real_net_carries_visits(n, k):
    S, G, cut = 48, 3, 5
    wseed, seed0 = REUSE_CUT_CASES[n]
    sd, onet = _weights(n, "plain", wseed)
    e = az.Engine(n, k, S, 3, c_puct=REUSE_C_PUCT, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    e.set_subtree_reuse(True)
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    games = _oracle_games(orc.Oracle(n, k, S, c_puct=REUSE_C_PUCT, reuse=True), onet, n, G, seed0, cut)
    tot = _totals(games)
    _assert_carried(tot, S, f"{n}x{n}")
    _assert_games(e, games, f"{n}x{n} reuse, net")
    _assert_work(c, tot, f"{n}x{n} reuse, net")
    e.close()


@pytest.mark.parametrize("model", ["plain", "resnet"])
@pytest.mark.parametrize("n,k", SMALL_AND_5)
def test_subtree_reuse_small_boards_both_kernels_both_nets(n, k, model, monkeypatch):
    """Complete games on the lock-step pipeline and in the persistent kernel (retained rows loaded into the LDS tree, the whole
    tree written back), with an odd slot count (a workgroup with a single game) and an even one (both tile subsets of
    k_search<.., TS = true> get their turn), and once more with the evaluation cache on top."""
    S, G = 48, (5 if n <= 5 else 4)
    seed0 = 22700 + 10 * n
    sd, onet = _weights(n, model)
    games = _oracle_games(orc.Oracle(n, k, S, c_puct=REUSE_C_PUCT, reuse=True), onet, n, G, seed0)
    tot = _totals(games)
    _assert_carried(tot, S, f"{n}x{n} {model}")
    for persist, slots, cache in (("0", 3, 0), ("0", 4, 0), ("1", 3, 0), ("1", 4, 0), ("1", 4, 1 << 12)):
        monkeypatch.setenv("AZ_PERSIST", persist)
        e = az.Engine(n, k, S, slots, c_puct=REUSE_C_PUCT, model=model, log_table=orc.numpy_log_table(S))
        e.load_weights(sd, 0)
        e.set_subtree_reuse(True)
        e.set_eval_cache(cache)
        c = e.selfplay(G, seed0=seed0)
        what = f"{n}x{n} {model} AZ_PERSIST={persist} {slots} slots cache={cache}"
        assert e.persistent() == (_persist_gp(n) if persist == "1" else 0), what
        _assert_games(e, games, what)
        _assert_work(c, tot, what)
        assert (c["cache_lookups"] > 0) == (cache > 0) and c["cache_hits"] <= c["cache_lookups"]
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# B.3 evaluation cache
# ---------------------------------------------------------------------------------------------------------------------
CACHE_WORK = ("games", "plies", "records", "simulations", "expansions", "root_evals", "terminal_hits", "depth_sum")


def _cache_episodes(n, k, S, slots, G, seed0, cut, sd, model, entries, games, what, gp=None):
    """The episode with the cache off, with it on, and again with it on: identical records, identical to the oracle's, the same
    work; the repeated episode finds at least half of its positions.  -> counters of (off, on, again)"""
    out = []
    for ent in (0, entries):
        e = az.Engine(n, k, S, slots, model=model, log_table=orc.numpy_log_table(S))
        e.load_weights(sd, 0)
        e.set_eval_cache(ent)
        for rep in range(2 if ent else 1):
            c = e.selfplay(G, seed0=seed0, max_plies=cut)
            assert gp is None or e.persistent() == gp, what
            out.append((_assert_games(e, games, f"{what} cache={ent} episode {rep}"), c))
        e.close()
    (r0, c0), (r1, c1), (r2, c2) = out
    _same_records(r0, r1, f"{what}: cache on"); _same_records(r0, r2, f"{what}: cache on, again")
    for key in CACHE_WORK:
        assert c0[key] == c1[key] == c2[key], f"{what}: {key}"
    assert c0["cache_lookups"] == 0 and c0["cache_hits"] == 0
    for c in (c1, c2):                    # (trunk_boards is not compared: the engine derives it from hits, expansions and root_evals)
        assert c["cache_lookups"] == c["expansions"] + c["root_evals"], what      # every evaluation is looked up first
        assert 0 <= c["cache_hits"] <= c["cache_lookups"], what
    print(f"{what}: hits {c1['cache_hits']} then {c2['cache_hits']} of {c2['cache_lookups']} lookups")
    assert c2["cache_hits"] >= 0.5 * c2["cache_lookups"], f"{what}: the repeated episode hit {c2['cache_hits']} of {c2['cache_lookups']}"
    return c0, c1, c2


def _cache_one_slot(n, k, S, G, seed0, cut, sd, model, entries, games, what):
    """One slot: one lookup and one insertion at a time, so the hits are a function of the episode and the counter identities
    are exact.  -> counters of (first, repeated episode)"""
    e = az.Engine(n, k, S, 1, model=model, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    e.set_eval_cache(entries)
    cs = []
    for rep in range(2):
        c = e.selfplay(G, seed0=seed0, max_plies=cut)
        _assert_games(e, games[:G], f"{what} one slot, episode {rep}")
        assert c["cache_lookups"] == c["expansions"] + c["root_evals"], what      # this one carries the weight: counted in the kernels
        # holds by construction -- the engine computes trunk_boards from this very expression -- and only pins its definition
        assert c["trunk_boards"] == c["expansions"] + c["root_evals"] - c["cache_hits"], what
        cs.append(c)
    e.close()
    return cs


@pytest.mark.parametrize("n,k", SIZES)
def test_eval_cache_changes_nothing_on_every_size(n, k):
    S, G, seed0 = 24, 3, 23000 + 10 * n
    cut = 0 if n <= 7 else 5
    entries = 1 if n == 12 else 1 << 14           # 12x12 (CPL = 3): the smallest table, 1024 entries, overwritten all the time
    sd, onet = _weights(n, "plain")
    games = _oracle_games(orc.Oracle(n, k, S), onet, n, G, seed0, cut)
    _cache_episodes(n, k, S, 3, G, seed0, cut, sd, "plain", entries, games, f"{n}x{n}")
    c1, c2 = _cache_one_slot(n, k, S, 2, seed0, cut, sd, "plain", 1 << 16, games, f"{n}x{n}")
    assert c1["cache_hits"] < c1["cache_lookups"]             # the first root at the least is new
    assert c2["cache_hits"] > c1["cache_hits"] and c2["cache_hits"] >= 0.5 * c2["cache_lookups"]


@pytest.mark.parametrize("model", ["plain", "resnet"])
@pytest.mark.parametrize("n,k", SMALL_AND_5)
def test_eval_cache_small_boards_both_kernels_both_nets(n, k, model, monkeypatch):
    """cache_lookup / cache_hit_store / cache_insert inside the persistent kernel, and k_root_cache + k_step on the lock-step
    pipeline: complete games, an even and an odd slot count."""
    S, G, seed0 = 24, 5, 23300 + 10 * n
    sd, onet = _weights(n, model)
    games = _oracle_games(orc.Oracle(n, k, S), onet, n, G, seed0)
    for persist in ("0", "1"):
        monkeypatch.setenv("AZ_PERSIST", persist)
        for slots in (4, 3):
            _cache_episodes(n, k, S, slots, G, seed0, 0, sd, model, 1 << 14, games, f"{n}x{n} {model} AZ_PERSIST={persist} {slots} slots",
                            gp=_persist_gp(n) if persist == "1" else 0)
        c1, c2 = _cache_one_slot(n, k, S, 2, seed0, 0, sd, model, 1 << 16, games, f"{n}x{n} {model} AZ_PERSIST={persist}")
        assert c2["cache_hits"] > c1["cache_hits"] and c2["cache_hits"] >= 0.5 * c2["cache_lookups"]


# ---------------------------------------------------------------------------------------------------------------------
# B.4 arena
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", SIZES)
def test_arena_two_nets_game_by_game(n, k):
    S, G = (16, 4) if n <= 8 else (8, 2)
    seed0 = 24000 + 10 * n
    (a, oa), (b, ob) = _weights(n, "plain"), _weights(n, "plain", seed=7)
    e = az.Engine(n, k, S, 3, log_table=orc.numpy_log_table(S))
    e.load_weights(a, 0); e.load_weights(b, 1)
    r = e.arena(G, seed0=seed0, temperature_table=orc.arena_T_table(n * n))
    assert e.persistent() == min(_persist_gp(n), 1)        # a workgroup's games must share one net: one game per workgroup
    e.close()
    o = orc.Oracle(n, k, S)
    with ThreadPoolExecutor(max_workers=4) as ex:
        want = list(ex.map(lambda g: o.arena_game(oa, ob, g, np.random.RandomState(seed0 + g).random_sample(n * n)), range(G)))
    w = l = d = 0
    for g, ro in enumerate(want):
        assert int(r["nply"][g]) == ro["nply"] and int(r["results"][g]) == ro["result"], f"{n}x{n} game {g}"
        assert np.array_equal(r["actions"][g][:ro["nply"]], ro["actions"]), f"{n}x{n} game {g}: moves"
        w += ro["result"] == 1; l += ro["result"] == 2; d += ro["result"] == 3
    assert (r["wins"], r["losses"], r["draws"], r["total"]) == (w, l, d, G)


# ---------------------------------------------------------------------------------------------------------------------
# B.5 search_batch
# ---------------------------------------------------------------------------------------------------------------------
BATCH_TEMPS = [1.0, 0.5, 1e-8, 0.05, 1e-7, 2.0, 0.3]       # two of them on the float32 path (<= 1e-7)
BATCH_NET = (8, 11, 13)                                     # the real net too: CPL 1 with a full 64-cell row, CPL 2, CPL 3


def _batch_positions(n, k, count, rs):
    nn = n * n
    pos = [(np.zeros(nn, np.uint8), 1, -1)]
    for b in (64, 128, 192):                 # the only stones, and the last move, on either side of a 64-cell word boundary
        if b < nn:
            for first, second in ((b - 1, b), (b, b - 1)):
                board = np.zeros(nn, np.uint8); board[first] = 1; board[second] = 2
                pos.append((board, 1, second))
    board = np.zeros(nn, np.uint8); board[nn - 1] = 1
    pos.append((board, 2, nn - 1))
    if k >= 4:
        pos += [_nearly_full(n, k, empty, rs) for empty in (2, 3, 5, 6)]
    return pos + _random_positions(rs, n, k, count - len(pos))


@pytest.mark.parametrize("n,k", SIZES)
def test_search_batch_three_waves_on_two_lanes(n, k):
    S, slots, count = 40, 16, 37
    rs = np.random.RandomState(25000 + n)
    pos = _batch_positions(n, k, count, rs)
    assert len(pos) == count
    noise = [rs.dirichlet([0.3] * int((b == 0).sum())) for b, _, _ in pos]
    us = [float(rs.random_sample()) for _ in pos]
    Ts = [BATCH_TEMPS[i % len(BATCH_TEMPS)] for i in range(count)]
    for synthetic in ((True, False) if n in BATCH_NET else (True,)):
        sd, onet = (None, None) if synthetic else _weights(n, "plain")
        o = orc.Oracle(n, k, S, synthetic=synthetic)
        with ThreadPoolExecutor(max_workers=16) as ex:
            want = list(ex.map(lambda i: o.search(onet, pos[i][0], pos[i][1], pos[i][2], Ts[i], noise[i], us[i]), range(count)))
        e = az.Engine(n, k, S, slots, synthetic=synthetic, engines=2, log_table=orc.numpy_log_table(S))
        assert e.lanes() == 2
        if not synthetic:
            e.load_weights(sd, 0)
        r = e.search_batch(np.stack([p[0] for p in pos]), [p[1] for p in pos], [p[2] for p in pos], Ts, noise, us)
        c = e.counters()
        e.close()
        for i in range(count):
            _assert_search({key: r[key][i] for key in SEARCH_KEYS + ("action",)}, want[i], f"{n}x{n} synthetic={synthetic} position {i}")
        assert c["simulations"] == count * S and c["root_evals"] == count and c["plies"] == count


# ---------------------------------------------------------------------------------------------------------------------
# B.6 deep engines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("n,k", SIZES)
def test_deep_synthetic_games_cut_at_3_plies(n, k, L):
    S, G, cut, seed0 = 1040, 2, 3, 26000 + 10 * n
    e = az.Engine(n, k, S, 2, synthetic=True, log_table=orc.numpy_log_table(S), deep=True)
    e.set_virtual_loss(L)
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    assert e.persistent() == 0
    games = _oracle_games(orc.Oracle(n, k, S, synthetic=True, virtual_loss=L), None, n, G, seed0, cut)
    _assert_games(e, games, f"{n}x{n} deep L={L}")
    _assert_work(c, _totals(games), f"{n}x{n} deep L={L}")
    assert c["simulations"] == S * c["plies"]
    e.close()


@pytest.mark.parametrize("n,k", [(8, 5), (12, 5)])
def test_deep_real_net_single_search(n, k):
    S = 1030
    sd, onet = _weights(n, "plain")
    rs = np.random.RandomState(26500 + n)
    board, pl, last = _random_positions(rs, n, k, 1)[0]
    noise = rs.dirichlet([0.3] * int((board == 0).sum()))
    e = az.Engine(n, k, S, 1, log_table=orc.numpy_log_table(S), deep=True)
    e.load_weights(sd, 0)
    r = e.search(board, pl, last, 1.0, noise, 0.37)
    e.close()
    _assert_search(r, orc.Oracle(n, k, S).search(onet, board, pl, last, 1.0, noise, 0.37), f"{n}x{n} deep S={S}")
    assert int(r["N"].sum()) == S
