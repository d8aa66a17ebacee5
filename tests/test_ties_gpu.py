"""PUCT tie-breaking on every copy of the selection: when two children share the maximal score the reference takes the one that
comes first in row-major legal order (mcts.py:70-74, max returns the first maximal element).  The evaluators here are the
constant nets of tests/ties.py -- a few discrete prior levels and one value for EVERY position -- so scores tie all the time
and that rule decides the whole search.  tests/golden/tree_ties_{n}x{k}.npz holds what the Python reference itself computed
with these evaluators, and how many of its selections had two or more maximal children (at the root and below it: both are
non-zero in every case that can have them, asserted in tests/test_oracle_golden.py).

Which test holds which copy of the rule:

  callback seam     az_search_callback: k_step<N> fed priors from the host        test_callback_seam_*, test_callback_tables_*
  k_step<N>         lock-step pipeline (AZ_PERSIST=0 where the persistent kernel
                    would serve), fused and tile-split trunks                     test_lock_step_*, test_search_batch_* (8x8 and up),
                                                                                  test_selfplay_* (AZ_PERSIST=0, 9x9, 15x15), test_properties_*
  k_search          persistent LDS-tree kernel, one cell per lane                 test_persistent_*, test_search_batch_* (7x7),
                                                                                  test_selfplay_small_boards_*
  DEEP k_step<N>    sqrt from HBM, more than 1024 simulations                     test_deep_*
  k_step_vl<N>      N + in-flight, W - in-flight (also DEEP, and batches of one)  test_virtual_loss_*

Fixture sizes and cells per lane of a tree row (TreeGeo<N>::CPL): 3x3, 7x7, 8x8 (64 cells: the wave exactly) 1; 9x9 2; 13x13 3;
15x15 4.  From 9x9 on cells j and j + 64 share a lane, and the `mirror` pattern puts the deciding tie between two such cells.
Everything is compared bit for bit (np.array_equal); the oracle's results are computed once per size and shared.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_options_all_sizes_gpu import (_assert_games, _assert_work, _nearly_full, _oracle_games, _same_records,
                                              _totals)
from tests.ties import TIE_SIZES, constant_resnet_tensors, constant_state_dict, levels_of
from tests.util import load

import alphazero_piskvorky_amd as az

MAX_S = 400               # the searches of the ordinary engines; the fixture's deeper cases are for test_deep_*
PERSIST_S_7x7 = 120       # (S + 1) * 49 edges of 16 B beside the net image in 160 KB of LDS: 120 simulations fit, 160 do not


@functools.lru_cache(maxsize=None)
def _cases(n, k):
    z = load(f"tree_ties_{n}x{k}.npz")
    out = []
    for i in range(len(z["seed"])):
        c = {key: z[key][i] for key in ("board", "levels", "P", "N", "W", "prior", "pi")}
        c.update(i=i, n=n, k=k, player=int(z["player"][i]), last=int(z["last"][i]), S=int(z["S"][i]), c_puct=float(z["c_puct"][i]),
                 T=float(z["T"][i]), vbias=float(z["vbias"][i]), v=float(z["v"][i]), action=int(z["action"][i]),
                 pattern=str(z["pattern"][i]))
        rs = np.random.RandomState(int(z["seed"][i]))
        c["noise"] = rs.dirichlet([0.3] * int((c["board"] == 0).sum())) if z["noise"][i] else None
        c["u"] = float(rs.random_sample())
        c["what"] = f"{n}x{n} case {i} ({c['pattern']}, vbias {c['vbias']}, S {c['S']}, c_puct {c['c_puct']})"
        out.append(c)
    return out


def _sd(c):
    return constant_state_dict(c["n"], c["levels"], c["vbias"])


def _oracle_search(c, S=None, L=0):
    S = S or c["S"]
    o = orc.Oracle(c["n"], c["k"], S, c_puct=c["c_puct"], virtual_loss=L)
    return o.search(orc.Net(c["n"], _sd(c)), c["board"], c["player"], c["last"], c["T"], c["noise"], c["u"])


@functools.lru_cache(maxsize=None)
def _oracle(n, k):
    """the sequential oracle on every case of the size, once"""
    with ThreadPoolExecutor(max_workers=16) as ex:
        return list(ex.map(_oracle_search, _cases(n, k)))


def _groups(cases):
    """an engine is built for one S and one c_puct: case indices by (S, c_puct)"""
    g = {}
    for c in cases:
        g.setdefault((c["S"], c["c_puct"]), []).append(c)
    return g


def _engine(c, S=None, **kw):
    S = S or c["S"]
    return az.Engine(c["n"], c["k"], S, kw.pop("slots", 1), c_puct=c["c_puct"], log_table=orc.numpy_log_table(S), **kw)


def _search(e, c):
    return e.search(c["board"], c["player"], c["last"], c["T"], c["noise"], c["u"])


def _assert_fixture(r, c, ro, what):
    """the reference's own numbers bit for bit; pi (a float32 of the build's exp and log table) against the oracle's"""
    assert np.array_equal(r["N"], c["N"]), f"{what}: visit counts differ from the reference's"
    assert int(r["N"].sum()) == c["S"]
    assert np.array_equal(r["W"], c["W"]), f"{what}: W differs from the reference's"
    assert np.array_equal(r["P"], c["prior"]), f"{what}: priors differ from the reference's"
    assert int(r["action"]) == c["action"], f"{what}: action"
    assert np.array_equal(r["pi"], ro["pi"]), f"{what}: pi differs from the oracle's"


def _assert_oracle(r, ro, what):
    for key in ("N", "W", "P", "pi"):
        assert np.array_equal(r[key], ro[key]), f"{what}: {key} differs from the oracle"
    assert int(r["action"]) == int(ro["action"]), f"{what}: action"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the callback seam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", TIE_SIZES)
def test_callback_seam_against_the_reference(n, k):
    cases = [c for c in _cases(n, k) if c["S"] <= MAX_S]
    want = _oracle(n, k)
    for (S, c_puct), group in _groups(cases).items():
        e = _engine(group[0])
        for c in group:
            r = e.search_callback(c["board"], c["player"], c["last"], c["T"], lambda cells, pl, la: (c["P"], c["v"]), c["noise"], c["u"])
            _assert_fixture(r, c, want[c["i"]], c["what"] + " callback")
        e.close()


def test_callback_tables_with_zeros_and_not_normalised():
    """'used as priors exactly as given, no masking, no renormalisation' (include/az_engine.h): a table with exact zeros and
    one that sums to 15.125, recorded from the reference's MCTS.run (no net has them as its softmax).  pi is the
    reference's float32 of numpy's exp and log: the 1e-6 of tests/test_oracle_golden.py."""
    n, k = 9, 5
    z = load(f"tree_ties_{n}x{k}.npz")
    assert (z["raw_P"][0] == 0).any() and abs(float(z["raw_P"][1].sum()) - 1.0) > 1.0
    for i in range(len(z["raw_seed"])):
        S, P, v = int(z["raw_S"][i]), z["raw_P"][i], float(z["raw_v"][i])
        assert int(z["raw_tied_root"][i]) > 0 and int(z["raw_tied_below"][i]) > 0
        u = float(np.random.RandomState(int(z["raw_seed"][i])).random_sample())
        e = az.Engine(n, k, S, 1, c_puct=float(z["raw_c_puct"][i]), log_table=orc.numpy_log_table(S))
        r = e.search_callback(z["raw_board"][i], int(z["raw_player"][i]), int(z["raw_last"][i]), float(z["raw_T"][i]),
                              lambda cells, pl, la: (P, v), None, u)
        e.close()
        what = f"raw table {i}"
        assert np.array_equal(r["N"], z["raw_N"][i]) and int(r["N"].sum()) == S, f"{what}: visit counts"
        assert np.array_equal(r["W"], z["raw_W"][i]), f"{what}: W"
        assert np.array_equal(r["P"], z["raw_prior"][i]), f"{what}: priors are not the given ones"
        assert int(r["action"]) == int(z["raw_action"][i]), f"{what}: action"
        np.testing.assert_allclose(r["pi"], z["raw_pi"][i], rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 2. lock-step k_step, 3. persistent k_search
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["0", None])
@pytest.mark.parametrize("n,k", TIE_SIZES)
def test_lock_step_against_the_reference(n, k, split, monkeypatch):
    monkeypatch.setenv("AZ_PERSIST", "0")
    if split is None:
        monkeypatch.delenv("AZ_SPLIT_MAX", raising=False)
    else:
        monkeypatch.setenv("AZ_SPLIT_MAX", split)
    cases = [c for c in _cases(n, k) if c["S"] <= MAX_S]
    want = _oracle(n, k)
    for (S, c_puct), group in _groups(cases).items():
        e = _engine(group[0])
        for c in group:
            e.load_weights(_sd(c), 0)
            r = _search(e, c)
            assert e.persistent() == 0
            _assert_fixture(r, c, want[c["i"]], c["what"] + f" k_step AZ_SPLIT_MAX={split}")
            _assert_oracle(r, want[c["i"]], c["what"] + f" k_step AZ_SPLIT_MAX={split}")
        e.close()


@pytest.mark.parametrize("n,k", [(3, 3), (7, 4)])
def test_persistent_kernel_against_the_reference(n, k, monkeypatch):
    monkeypatch.delenv("AZ_PERSIST", raising=False)
    cases = [c for c in _cases(n, k) if c["S"] <= (PERSIST_S_7x7 if n == 7 else MAX_S)]
    assert len(cases) >= 6
    want = _oracle(n, k)
    for (S, c_puct), group in _groups(cases).items():
        e = _engine(group[0])
        for c in group:
            e.load_weights(_sd(c), 0)
            r = _search(e, c)
            assert e.persistent() > 0, f"{c['what']}: not the persistent kernel"
            _assert_fixture(r, c, want[c["i"]], c["what"] + " k_search")
            _assert_oracle(r, want[c["i"]], c["what"] + " k_search")
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. deep k_step
# ---------------------------------------------------------------------------------------------------------------------
DEEP_S = 1100


def test_deep_3x3_against_the_reference():
    cases = [c for c in _cases(3, 3) if c["S"] > MAX_S]
    assert sorted(c["pattern"] for c in cases) == ["three", "uniform"] and all(c["S"] == DEEP_S for c in cases)
    for c in cases:
        ro = _oracle_search(c)
        e = _engine(c, deep=True)
        e.load_weights(_sd(c), 0)
        r = _search(e, c)
        assert e.persistent() == 0
        e.close()
        _assert_fixture(r, c, ro, c["what"] + " deep")
        _assert_oracle(r, ro, c["what"] + " deep")


def test_deep_9x9_against_the_oracle():
    """the uniform and the three-level net of the fixture (cases 0 and 5: their positions, nets and draws) with 1100 simulations"""
    cases = [_cases(9, 5)[i] for i in (0, 5)]
    assert [c["pattern"] for c in cases] == ["uniform", "three"]
    with ThreadPoolExecutor(max_workers=2) as ex:
        want = list(ex.map(lambda c: _oracle_search(c, S=DEEP_S), cases))
    for c, ro in zip(cases, want):
        e = _engine(c, S=DEEP_S, deep=True)
        e.load_weights(_sd(c), 0)
        r = _search(e, c)
        e.close()
        _assert_oracle(r, ro, c["what"] + f" deep S={DEEP_S}")
        assert int(r["N"].sum()) == DEEP_S


# ---------------------------------------------------------------------------------------------------------------------
# 5. k_step_vl
# ---------------------------------------------------------------------------------------------------------------------
VL_SIZES = [(7, 4), (9, 5), (15, 5)]
VL_LEAVES = (2, 8, 32)


def _vl_cases(n, k):
    """uniform with both signs of the value, three levels, and from 9x9 the in-lane ties"""
    cs = _cases(n, k)
    pick = [0, 1, 5] + ([10] if n >= 9 else [])
    assert [cs[i]["pattern"] for i in pick] == ["uniform", "uniform", "three"] + (["mirror"] if n >= 9 else [])
    return [cs[i] for i in pick]


@pytest.mark.parametrize("n,k", VL_SIZES)
def test_virtual_loss_batches_against_the_oracle(n, k):
    """On an open board a batch does NOT collide under ties: the in-flight visit of the first simulation lowers that edge's
    score below its tied siblings', so the next simulation takes the next cell in order, and the oracle expands S leaves in S
    simulations on every fixture case at these sizes (the engine's duplicate_leaves must then be 0).  Batches collide once
    they are larger than the open leaves: the same uniform net on boards with 5 and 3 empty cells and batches of 8 and 32.
    There the root has fewer children than the batch has simulations and none of them is expanded before the batch ends, so
    the first batch already sends a simulation to a pending leaf: duplicate_leaves > 0 follows from the rule alone."""
    cases = _vl_cases(n, k)
    jobs = [(c, L) for c in cases for L in VL_LEAVES]
    with ThreadPoolExecutor(max_workers=16) as ex:
        want = dict(zip([(c["i"], L) for c, L in jobs], ex.map(lambda j: _oracle_search(j[0], L=j[1]), jobs)))
    for L in VL_LEAVES:
        for (S, c_puct), group in _groups(cases).items():
            e = _engine(group[0])
            e.set_virtual_loss(L)
            for c in group:
                e.load_weights(_sd(c), 0)
                r = _search(e, c)
                ro = want[(c["i"], L)]
                _assert_oracle(r, ro, c["what"] + f" L={L}")
                assert int(r["N"].sum()) == S
                if ro["nexp"] == S + 1:               # every simulation of the oracle expanded a leaf
                    assert e.counters()["duplicate_leaves"] == 0, c["what"] + f" L={L}"
            e.close()
    # the uniform net where batches must collide
    S, T = 64, 0.8
    rs = np.random.RandomState(41000 + n)
    sd = constant_state_dict(n, levels_of("uniform", n), -0.5)
    onet = orc.Net(n, sd)
    pos = [(_nearly_full(n, k, empty, rs), float(rs.random_sample())) for empty in (5, 3)]
    for L in (8, 32):
        e = az.Engine(n, k, S, 1, log_table=orc.numpy_log_table(S))
        e.load_weights(sd, 0)
        e.set_virtual_loss(L)
        o = orc.Oracle(n, k, S, virtual_loss=L)
        for (board, pl, last), u in pos:
            ro = o.search(onet, board, pl, last, T, None, u)
            what = f"{n}x{n} uniform net, {int((board == 0).sum())} empty cells, L={L}"
            assert L > int((board == 0).sum()) and ro["nexp"] < S + 1       # see above: the first batch already collides
            r = e.search(board, pl, last, T, None, u)
            _assert_oracle(r, ro, what)
            assert e.counters()["duplicate_leaves"] > 0, what
        e.close()


@pytest.mark.parametrize("n,k", TIE_SIZES)
def test_virtual_loss_kernel_with_batches_of_one_against_the_reference(n, k, monkeypatch):
    """AZ_VL_FORCE=1: k_step_vl for L = 1, which must be the sequential search"""
    monkeypatch.setenv("AZ_VL_FORCE", "1")
    cases = [c for c in _cases(n, k) if c["S"] <= MAX_S]
    want = _oracle(n, k)
    for (S, c_puct), group in _groups(cases).items():
        e = _engine(group[0])
        e.set_virtual_loss(1)
        for c in group:
            e.load_weights(_sd(c), 0)
            r = _search(e, c)
            assert e.persistent() == 0           # the persistent kernel never serves the batched search
            _assert_fixture(r, c, want[c["i"]], c["what"] + " k_step_vl L=1")
        e.close()


def test_virtual_loss_deep_9x9_against_the_oracle():
    c, L = _cases(9, 5)[10], 8
    assert c["pattern"] == "mirror"
    ro = _oracle_search(c, S=DEEP_S, L=L)
    e = _engine(c, S=DEEP_S, deep=True)
    e.load_weights(_sd(c), 0)
    e.set_virtual_loss(L)
    r = _search(e, c)
    e.close()
    _assert_oracle(r, ro, c["what"] + f" deep S={DEEP_S} L={L}")
    assert int(r["N"].sum()) == DEEP_S


# ---------------------------------------------------------------------------------------------------------------------
# 6. az_search_batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(7, 4), (15, 5)])
def test_search_batch_equals_the_single_searches(n, k, monkeypatch):
    """All positions of one (S, c_puct) -- what an engine is built for -- in one call, once with every net of the group (a call has
    one net): equal to the single searches of the same engine, and the net's own case equal to the reference."""
    monkeypatch.delenv("AZ_PERSIST", raising=False)
    cases = [c for c in _cases(n, k) if c["S"] <= MAX_S]
    want = _oracle(n, k)
    for (S, c_puct), group in _groups(cases).items():
        e = _engine(group[0], slots=2, engines=2)            # two lanes of one slot: a batch of three or four is two waves
        assert e.lanes() == 2
        for c in group:
            e.load_weights(_sd(c), 0)
            for noisy in (False, True):                      # root noise is on or off for a whole call
                batch = [d for d in group if (d["noise"] is not None) == noisy]
                if not batch:
                    continue
                r = e.search_batch(np.stack([d["board"] for d in batch]), [d["player"] for d in batch], [d["last"] for d in batch],
                                   [d["T"] for d in batch], [d["noise"] for d in batch] if noisy else None, [d["u"] for d in batch])
                if n == 7:
                    assert (e.persistent() > 0) == (S <= PERSIST_S_7x7), f"{c['what']}: persistent {e.persistent()}"
                for j, d in enumerate(batch):
                    got = {key: r[key][j] for key in ("N", "W", "P", "pi", "action")}
                    if d is c:
                        _assert_fixture(got, d, want[d["i"]], d["what"] + " in a batch")
                    single = _search(e, d)
                    _assert_oracle(got, single, d["what"] + f" with the net of case {c['i']}: batch against the single search")
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. whole self-play games
# ---------------------------------------------------------------------------------------------------------------------
def _selfplay(n, k, S, G, seed0, sd, onet, what, cut=0, c_puct=2.0, reuse=False, model="plain", **kw):
    games = _oracle_games(orc.Oracle(n, k, S, c_puct=c_puct, reuse=reuse), onet, n, G, seed0, cut)
    e = az.Engine(n, k, S, kw.pop("slots", 3), c_puct=c_puct, model=model, log_table=orc.numpy_log_table(S), **kw)
    e.load_weights(sd, 0)
    e.set_subtree_reuse(reuse)
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    _assert_games(e, games, what, cut)
    _assert_work(c, _totals(games), what)
    return e, games, c


@pytest.mark.parametrize("persist", ["0", "1"])
def test_selfplay_3x3_to_the_end(persist, monkeypatch):
    monkeypatch.setenv("AZ_PERSIST", persist)
    n, k, S, G = 3, 3, 200, 8
    results = set()
    for pattern, vbias in (("uniform", 0.0), ("three", -0.5), ("checker", 0.25)):
        sd = constant_state_dict(n, levels_of(pattern, n, seed=7103), vbias)
        e, games, c = _selfplay(n, k, S, G, 31000, sd, orc.Net(n, sd), f"3x3 {pattern} vbias={vbias} AZ_PERSIST={persist}")
        assert (e.persistent() > 0) == (persist == "1")
        e.close()
        assert c["terminal_hits"] > 0
        results |= {g["result"] for g in games}
    assert results == {1, 2, 3}, f"outcomes {results}: wins of both sides and draws are wanted"


@pytest.mark.parametrize("persist", ["0", "1"])
def test_selfplay_small_boards_7x7_to_the_end(persist, monkeypatch):
    monkeypatch.setenv("AZ_PERSIST", persist)
    n, k, S, G = 7, 4, 48, 4
    sd = constant_state_dict(n, levels_of("three", n, seed=7107), -0.5)
    e, games, c = _selfplay(n, k, S, G, 31100, sd, orc.Net(n, sd), f"7x7 three levels AZ_PERSIST={persist}")
    assert (e.persistent() > 0) == (persist == "1")
    e.close()
    assert all(g["result"] != 0 for g in games)


@pytest.mark.parametrize("n,k,pattern,vbias", [(9, 5, "mirror", -0.5), (15, 5, "mirror", 0.0), (15, 5, "uniform", -0.5)])
def test_selfplay_large_boards_two_lanes_with_refill(n, k, pattern, vbias):
    S, G, cut = 64, 5, 4
    sd = constant_state_dict(n, levels_of(pattern, n), vbias)
    e, games, c = _selfplay(n, k, S, G, 31200 + n, sd, orc.Net(n, sd), f"{n}x{n} {pattern} vbias={vbias}", cut=cut, slots=4, engines=2)
    assert e.lanes() == 2 and G > 4
    e.close()


def test_selfplay_resnet_9x9():
    n, k, S, G, cut = 9, 5, 64, 5, 4
    t = constant_resnet_tensors(n, levels_of("mirror", n), -0.5)
    e, games, c = _selfplay(n, k, S, G, 31300, t, orc.Net(n, resnet_tensors=t), "9x9 ResidualBlock mirror", cut=cut, slots=4,
                            engines=2, model="resnet")
    e.close()


@pytest.mark.parametrize("n,k", [(7, 4), (8, 5), (9, 5), (13, 5), (15, 5)])
def test_selfplay_subtree_reuse(n, k):
    """k_reuse / k_move with tied counts.  Every evaluation of a constant net is the same, so WHICH of several tied cells a
    selection below the root takes changes the root's counts only through terminal leaves; a retained subtree makes the
    order below the root the next ply's visit counts, at every number of cells per lane.  Flat priors carry little from ply
    to ply (the oracle tops up 1128 or 1132 of 24 * 48 simulations): the bar is only that something is carried and that no
    root but the first is evaluated again."""
    S, G, cut = 48, 4, 6
    sd = constant_state_dict(n, levels_of("three", n, seed=7100 + n), -0.5)
    e, games, c = _selfplay(n, k, S, G, 31400 + n, sd, orc.Net(n, sd), f"{n}x{n} reuse", cut=cut, c_puct=0.3, reuse=True)
    e.close()
    tot = _totals(games)
    assert tot["sims"] < S * tot["plies"] and c["root_evals"] == G < c["plies"]


# ---------------------------------------------------------------------------------------------------------------------
# 8. properties that do not lean on the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _episode(n, k, S, G, cut, sd, seed0, prepare=None):
    e = az.Engine(n, k, S, 3, log_table=orc.numpy_log_table(S))
    e.load_weights(sd, 0)
    if prepare:
        prepare(e)
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    rec = e.records()
    e.close()
    return rec, c


@pytest.mark.parametrize("n,k", [(7, 4), (9, 5), (15, 5)])
def test_properties_leaf_symmetry_and_cache_change_nothing(n, k):
    """Every dihedral symmetry of a constant table over the whole board is -- for the uniform net -- the same table, so the
    records under random-symmetry leaf evaluation are those without it; and the evaluation cache never changes a record."""
    S, G, cut = 48, 4, 5
    sd = constant_state_dict(n, levels_of("uniform", n), -0.5)
    plain, c0 = _episode(n, k, S, G, cut, sd, 31500 + n)
    sym, _ = _episode(n, k, S, G, cut, sd, 31500 + n, lambda e: e.set_leaf_symmetry(True))
    _same_records(plain, sym, f"{n}x{n} uniform net, leaf symmetry on")
    for pattern in ("uniform", "three"):
        sd = constant_state_dict(n, levels_of(pattern, n, seed=7100 + n), -0.5)
        off, c0 = _episode(n, k, S, G, cut, sd, 31600 + n)
        on, c1 = _episode(n, k, S, G, cut, sd, 31600 + n, lambda e: e.set_eval_cache(1 << 12))
        _same_records(off, on, f"{n}x{n} {pattern} net, evaluation cache on")
        assert c0["cache_lookups"] == 0 and c1["cache_lookups"] > 0
        for key in ("plies", "simulations", "expansions", "terminal_hits", "depth_sum"):
            assert c0[key] == c1[key], f"{n}x{n} {pattern}: {key}"


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("n,k", [(7, 4), (9, 5), (15, 5)])
def test_properties_emulated_trunks_are_exact_on_constant_nets(n, k, mode, monkeypatch):
    """All products of a constant net's trunk are exactly zero: the fp32-emulating trunks have nothing to round, and visit
    counts, W and pi are those of the float32 trunk (and so the reference's)."""
    monkeypatch.setenv("AZ_PERSIST", "0")
    cases = [c for c in _cases(n, k) if c["S"] <= MAX_S]
    want = _oracle(n, k)
    for (S, c_puct), group in _groups(cases).items():
        e = _engine(group[0])
        for c in group:
            e.set_trunk_mode("f32")
            e.load_weights(_sd(c), 0)
            r32 = _search(e, c)
            e.set_trunk_mode(mode)
            r = _search(e, c)
            assert e.trunk_mode() == mode
            _assert_oracle(r, r32, c["what"] + f" {mode} against the float32 trunk")
            _assert_fixture(r, c, want[c["i"]], c["what"] + f" {mode}")
        e.close()
