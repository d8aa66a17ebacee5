"""The Gumbel root search, the parts that need no GPU: the Gumbel tape against numpy's own RandomState, az_gumbel_schedule and
az_gumbel_target against the rule restated in tests/gumbel.py, the argument checks of the Python seams, and the yardstick
itself -- the numpy search of tests/gumbel.py with the option off is Oracle.search, bit for bit."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import gumbel
from tests.util import ROOT, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.mcts import MCTS, check_gumbel
from alphazero_piskvorky_amd.self_play import SelfPlayManager

NEW = ("az_set_gumbel", "az_get_gumbel", "az_gumbel_schedule", "az_gumbel_target", "az_gumbel_vmix", "az_rng_selfplay_tape_gumbel")


def test_symbols_are_exported_declared_and_listed():
    L = _capi.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        header = f.read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s


# ---------------------------------------------------------------------------------------------------------------------
# the tape
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_plies,seed", [(3, 0, 5), (5, 0, 123456), (15, 4, 2 ** 32 + 9)])
def test_tape_is_randomstate_gumbel_bit_for_bit(n, max_plies, seed):
    """per ply p: gumbel(size = nn - p), then random_sample(); numpy's legacy gumbel is the scalar -log(-log(1 - U))"""
    noise, u = _capi.selfplay_tape_gumbel(seed, n, max_plies)
    want_n, want_u = gumbel.selfplay_tape(seed & 0xFFFFFFFF, n, max_plies or None)
    assert noise.dtype == np.float64 and noise.tobytes() == want_n.tobytes()
    assert u.tobytes() == want_u.tobytes()
    assert (noise < 0).any() and (noise > 1).any()              # not a Dirichlet sample


def test_tape_refuses_bad_arguments():
    L = _capi.lib()
    buf = np.zeros(400, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.az_rng_selfplay_tape_gumbel(1, 0, 0, p, p) == -1 and L.az_rng_selfplay_tape_gumbel(1, 16, 0, p, p) == -1
    assert L.az_rng_selfplay_tape_gumbel(1, 3, 0, None, p) == -1 and L.az_rng_selfplay_tape_gumbel(1, 3, 0, p, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------------------------
KS = (1, 2, 3, 5, 7, 16, 64)
SS = (1, 7, 8, 16, 33, 64, 400, 1100)


def test_schedule_equals_the_restatement():
    for k in KS:
        for S in SS:
            got = _capi.gumbel_schedule(k, S)
            assert got.dtype == np.int32 and np.array_equal(got, gumbel.schedule(k, S)), (k, S)
    assert _capi.gumbel_schedule(16, 64).tolist() == [0] * 16 + [1] * 8 + [2] * 8 + [3] * 4 + [4] * 4 + [5] * 4 + [6] * 4 + \
        [7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14]
    assert _capi.gumbel_schedule(0, 4).tolist() == [0, 1, 2, 3]
    for bad in ((-1, 4), (4, 0), (4, 65535)):
        with pytest.raises(ValueError):
            _capi.gumbel_schedule(*bad)


def test_playing_the_gate_always_finds_a_child_and_leaves_the_schedules_visits():
    """the gate N == seq[t] played on random scores with random q: every simulation has a selectable child, and the visits it
    leaves are the schedule's multiset whatever the scores were"""
    rs = np.random.RandomState(7)
    for k in KS:
        for S in SS:
            seq = _capi.gumbel_schedule(k, S)
            legal = k + int(rs.randint(0, 5))                   # more legal cells than candidates
            h = rs.gumbel(size=legal) + rs.normal(size=legal)
            N = np.zeros(legal, np.int64)
            for t in range(S):
                sc = h + (50.0 + N.max()) * rs.uniform(-1, 1, legal)
                cand = N == seq[t]
                assert cand.any(), (k, S, t)
                N[int(np.argmax(np.where(cand, sc, -np.inf)))] += 1
            assert sorted(N[N > 0].tolist()) == gumbel.schedule_visits(k, S), (k, S)
    assert gumbel.schedule_visits(16, 64) == [1] * 8 + [3] * 4 + [7, 7, 15, 15]


# ---------------------------------------------------------------------------------------------------------------------
# az_gumbel_target = the rule
# ---------------------------------------------------------------------------------------------------------------------
def random_row(rs, i):
    """one root row: kind 0 a halving-like row, 1 one legal cell, 2 every visit on one child, 3 equal scores among the most
    visited (the lowest wins), 4 a large count"""
    kind = i % 5
    count = 1 if kind == 1 else int(rs.randint(2, 226)) if kind != 4 else int(rs.randint(129, 226))
    logits = (rs.normal(size=count) * 3).astype(np.float32)
    e = np.exp(logits.astype(np.float64) - logits.max())
    prior = (e / e.sum()).astype(np.float32)
    g = rs.gumbel(size=count)
    S = int(rs.choice([1, 16, 32, 64, 400]))
    N = np.zeros(count, np.int32)
    if kind == 2 or count == 1:
        N[int(rs.randint(count))] = S
    else:
        cand = rs.choice(count, size=min(count, 16), replace=False)
        for c, v in zip(cand, reversed(gumbel.schedule_visits(len(cand), S))):
            N[c] = v
    W = (N * rs.uniform(-0.95, 0.95, count)).astype(np.float64)
    if kind == 3 and (N == N.max()).sum() >= 2:
        top = np.flatnonzero(N == N.max())
        logits[top] = logits[top[0]]
        g[top] = g[top[0]]
        W[top] = W[top[0]]
    return logits, g, N, W, prior, np.float32(rs.uniform(-1, 1))


@functools.lru_cache(maxsize=None)
def rows():
    rs = np.random.RandomState(20261019)
    return tuple(random_row(rs, i) for i in range(300))


def test_gumbel_target_equals_the_rule_on_random_rows():
    ties = single = onechild = unvisited = big = 0
    for logits, g, N, W, P, v0 in rows():
        for cv, cs in ((50.0, 1.0), (0.0, 0.1), (20.0, 3.0)):
            want_pi, want_a, want_vm = gumbel.target(logits, g, N, W, P, v0, cv, cs)
            pi, a = _capi.gumbel_target(logits, g, N, W, P, v0, cv, cs)
            assert a == want_a, (N, a, want_a)
            assert pi.dtype == np.float32 and gumbel.within_one_float32_step(pi, want_pi)
            assert abs(float(pi.astype(np.float64).sum()) - 1.0) < 1e-6
        assert _capi.gumbel_vmix(N, W, P, v0) == want_vm                    # exact: the same pairwise order
        top = np.flatnonzero(N == N.max())
        ties += len(top) > 1
        single += len(N) == 1
        onechild += int((N > 0).sum() == 1)
        unvisited += int((N == 0).any())
        big += len(N) > 128
    assert len(rows()) == 300 and ties > 50 and single >= 60 and onechild >= 100 and unvisited > 150 and big >= 60, \
        (ties, single, onechild, unvisited, big)


def test_equal_scores_take_the_lowest_cell_and_unvisited_children_get_v_mix():
    logits = np.array([0.5, 0.5, 0.5, -1.0], np.float32)
    g = np.array([0.25, 0.25, 0.25, 3.0])
    N, W = np.array([2, 2, 2, 0], np.int32), np.array([1.0, 1.0, 1.0, 0.0])
    P = np.array([0.3, 0.3, 0.3, 0.1], np.float32)
    pi, a = _capi.gumbel_target(logits, g, N, W, P, 0.2)
    assert a == 0                                                # three equal scores among N == max N; cell 3 (N = 0) is no candidate
    # v_mix = (0.2 + (6 / 0.9) * 0.45) / 7 with the float32 priors widened
    p = float(np.float32(0.3))
    vm = (float(np.float32(0.2)) + (6.0 / (p + p + p)) * (p * 0.5 + p * 0.5 + p * 0.5)) / 7.0
    assert _capi.gumbel_vmix(N, W, P, 0.2) == vm
    y = np.array([0.5 + 52.0 * 0.5] * 3 + [-1.0 + 52.0 * vm])
    e = np.exp(y - y.max())
    assert gumbel.within_one_float32_step(pi, e / e.sum())


def test_gumbel_target_refuses_bad_arguments():
    ok = ([0.0, 1.0], [0.1, 0.2], [3, 1], [1.0, 0.0], [0.5, 0.5], 0.0)
    _capi.gumbel_target(*ok)
    for cv, cs in ((-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (50.0, 0.0), (50.0, -1.0), (50.0, float("inf"))):
        with pytest.raises(ValueError):
            _capi.gumbel_target(*ok, cv, cs)
    with pytest.raises(ValueError):
        _capi.gumbel_target([0.0, 1.0], [0.1, 0.2], [0, 0], [0.0, 0.0], [0.5, 0.5], 0.0)      # no visit at all
    with pytest.raises(ValueError):
        _capi.gumbel_target([0.0, 1.0], [0.1, 0.2], [3, -1], [1.0, 0.0], [0.5, 0.5], 0.0)
    with pytest.raises(ValueError):
        _capi.gumbel_target([0.0], [0.1, 0.2], [3, 1], [1.0, 0.0], [0.5, 0.5], 0.0)
    with pytest.raises(ValueError):
        _capi.gumbel_target([], [], [], [], [], 0.0)
    assert np.isnan(_capi.gumbel_vmix([0, 0], [0.0, 0.0], [0.5, 0.5], 0.0))


def test_setters_refuse_a_null_engine():
    L = _capi.lib()
    m, cv, cs = C.c_int(7), C.c_double(7.0), C.c_double(7.0)
    assert L.az_set_gumbel(None, 16, 50.0, 1.0) == -1
    assert L.az_get_gumbel(None, C.byref(m), C.byref(cv), C.byref(cs)) == -1 and m.value == 7 and cv.value == cs.value == 7.0


# ---------------------------------------------------------------------------------------------------------------------
# the Python seams
# ---------------------------------------------------------------------------------------------------------------------
def test_check_gumbel():
    assert check_gumbel(None) is None
    assert check_gumbel({}) == {"m": 16, "c_visit": 50.0, "c_scale": 1.0} == _capi.GUMBEL_DEFAULTS
    assert check_gumbel({"m": 4, "c_scale": 0.5}) == {"m": 4, "c_visit": 50.0, "c_scale": 0.5}
    for bad in ({"m": 0}, {"m": 65}, {"m": -1}, {"c_visit": -1.0}, {"c_visit": float("nan")}, {"c_visit": float("inf")},
                {"c_scale": 0.0}, {"c_scale": float("inf")}, {"c_scale": float("nan")}, {"k": 2}):
        with pytest.raises(ValueError):
            check_gumbel(bad)
    # every refused combination
    for kw in (dict(subtree_reuse=True), dict(virtual_loss=4), dict(forced_playouts={"k": 2.0, "prune": True}), dict(evaluator=object())):
        with pytest.raises(ValueError):
            check_gumbel({"m": 16}, **kw)
        assert check_gumbel(None, **kw) is None
    assert az.self_play.check_gumbel is check_gumbel


def test_seams_validate_and_refuse_the_combinations():
    g = {"m": 8}
    assert SelfPlayManager(None, "cuda:0", gumbel=g).gumbel == {"m": 8, "c_visit": 50.0, "c_scale": 1.0}
    assert SelfPlayManager(None, "cuda:0").gumbel is None
    for kw in (dict(subtree_reuse=True), dict(virtual_loss=2), dict(forced_playouts={"k": 2.0})):
        with pytest.raises(ValueError):
            SelfPlayManager(None, "cuda:0", gumbel=g, **kw)
    from alphazero_piskvorky_amd.controller import BatchPolicyValueFn
    ev = BatchPolicyValueFn.__new__(BatchPolicyValueFn)
    with pytest.raises(ValueError):
        SelfPlayManager(None, "cuda:0", gumbel=g, evaluator=ev)
    fn = lambda state: None
    with pytest.raises(ValueError):
        MCTS(fn, 10, 2.0, gumbel=g)                              # a plain callable returns priors, not logits
    assert MCTS(fn, 10, 2.0).gumbel is None


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick: the numpy search with the option off is the oracle's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,S", [(5, 4, 64), (9, 5, 32)])
def test_restatement_with_the_option_off_is_oracle_search(n, k, S):
    """5x5 with the fixture's trained net (logits, P, v from the oracle's Net.eval), 9x9 with the synthetic evaluator"""
    if n == 5:
        net, o = orc.Net(5, weights_from_fixture(5, "ckpt_saved")), orc.Oracle(n, k, S)
        ev = lambda b, p, l: net.eval(o.encode(b, p, l))
    else:
        net, o = None, orc.Oracle(n, k, S, synthetic=True)
        ev = lambda b, p, l: (np.zeros(n * n, np.float32),) + o.synth_eval(b, p, l)
    for stones, seed in ((0, 1), (6, 2), (11, 3)):
        board, player, last = gumbel.random_position(n, k, stones, seed)
        rs = np.random.RandomState(seed + 100)
        for noise in (rs.dirichlet([0.3] * int((board == 0).sum())), None):
            for T in (1.0, 1e-9):
                u = rs.random_sample()
                want = o.search(net, board, player, last, T, noise, u)
                got = gumbel.search_move(ev, n, k, S, board, player, last, T, noise, u, m=0)
                assert np.array_equal(got["N"], want["N"]) and np.array_equal(got["W"], want["W"]) and np.array_equal(got["P"], want["P"])
                assert got["action"] == want["action"] and np.array_equal(got["pi"], want["pi"]) and got["N"].sum() == S


def test_restatement_the_option_changes_the_tree_keeps_the_priors_and_follows_the_schedule():
    n, k, S, m = 5, 4, 32, 16
    net, o = orc.Net(5, weights_from_fixture(5, "ckpt_saved")), orc.Oracle(n, k, S)
    ev = lambda b, p, l: net.eval(o.encode(b, p, l))
    board, player, last = gumbel.random_position(n, k, 6, 2)
    g = np.random.RandomState(5).gumbel(size=19)
    off = gumbel.search(ev, n, k, S, board, player, last)
    on = gumbel.search(ev, n, k, S, board, player, last, g=g, m=m)
    assert on["N"].sum() == off["N"].sum() == S and not np.array_equal(on["N"], off["N"]) and np.array_equal(on["P"], off["P"])
    assert sorted(on["N"][on["N"] > 0].tolist()) == gumbel.schedule_visits(16, S)
    # the restatement's own teeth: the wrong gate and sigma without max N give other trees
    assert not np.array_equal(gumbel.search(ev, n, k, S, board, player, last, g=g, m=m, mutate="ge")["N"], on["N"])
    r = gumbel.search_move(ev, n, k, S, board, player, last, 1.0, g, 0.5, m=m)
    assert abs(float(r["pi"].astype(np.float64).sum()) - 1.0) < 1e-6 and (r["pi"][board != 0] == 0).all() and board[r["action"]] == 0
    assert r["N"][r["action"]] == r["N"].max()
