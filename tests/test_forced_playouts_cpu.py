"""Forced playouts and policy target pruning, the parts that need no GPU: az_forced_prune against the rule restated in
tests/forced.py, the argument checks of the C-ABI and the Python seams, and the yardstick itself -- the numpy search of
tests/forced.py with the rule off is Oracle.search, bit for bit."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import forced
from tests.util import ROOT

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.mcts import MCTS, check_forced_playouts
from alphazero_piskvorky_amd.self_play import SelfPlayManager

NEW = ("az_set_forced_playouts", "az_get_forced_playouts", "az_forced_prune")


def test_symbols_are_exported_declared_and_listed():
    L = _capi.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        header = f.read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s


# ---------------------------------------------------------------------------------------------------------------------
# az_forced_prune = the rule
# ---------------------------------------------------------------------------------------------------------------------
def random_row(rs, nn, total, kind):
    """one root row as a search could leave it: a few children hold most visits, many hold the handful the forced rule gives.
    kind 1: the two most visited children tie; kind 2: a second child as good as the first, so that score(c, N_c) >= target"""
    count = int(rs.randint(2, nn + 1))
    prior = rs.dirichlet([0.3] * count).astype(np.float32)
    weights = rs.dirichlet([0.15] * count)
    N = rs.multinomial(total, weights).astype(np.int32)
    if total >= 8:
        small = rs.choice(count, size=min(count, 3), replace=False)       # children with exactly 0 and 1 visits
        for i, c in enumerate(small):
            if c != int(np.argmax(N)):
                N[int(np.argmax(N))] += N[c] - (i % 2)
                N[c] = i % 2
    if kind == 1 and count >= 3 and total >= 2:
        a, b, c = np.argsort(-N, kind="stable")[:3]
        s = int(N[a] + N[b])
        N[a] = N[b] = s // 2
        N[c] += s - 2 * (s // 2)
    W = (N * rs.uniform(-0.9, 0.9, count)).astype(np.float64)
    if kind == 2 and count >= 2 and N.sum() > 0:
        c = int(np.argsort(-N, kind="stable")[1])
        if N[c] > 0:
            W[c] = float(N[c])                                             # Q_c = 1: above any target the first child can set
    if N.sum() == 0:
        N[0] = 1
    return N, W, prior


@functools.lru_cache(maxsize=None)
def rows():
    rs = np.random.RandomState(20261019)
    out = []
    for nn in (9, 25, 81, 225):
        for total in (1, 32, 400, 5000):
            for i in range(20):
                out.append((nn, total) + random_row(rs, nn, total, i % 3))
    return tuple(out)


def test_forced_prune_equals_the_rule_on_random_rows():
    removed_rows = emptied = kept_by_score = ties = with0 = with1 = 0
    for k in (2.0, 0.5, 16.0):
        for nn, total, N, W, P in rows():
            want = forced.prune(k, 2.0, N, W, P)
            got, removed = _capi.forced_prune(k, 2.0, N, W, P)
            assert got.dtype == np.int32 and np.array_equal(got, want), (k, nn, total, N, want, got)
            assert removed == int(N.sum() - want.sum()) >= 0
            star = int(np.argmax(N))
            assert got[star] == N[star] and (got <= N).all() and (got[N == 0] == 0).all() and not (got == 1)[N > 1].any()
            if k == 2.0:
                removed_rows += removed > 0
                emptied += int(((got == 0) & (N > 1)).sum() > 0)
                ties += int((N == N.max()).sum() > 1)
                with0 += int((N == 0).any()); with1 += int((N == 1).any())
                sq = np.sqrt(N.sum() + 1e-8)
                score = lambda c: W[c] / N[c] + ((2.0 * float(P[c])) * sq) / (1 + N[c])
                kept_by_score += int(any(c != star and N[c] > 0 and score(c) >= score(star) for c in range(len(N))))
    assert len(rows()) == 320
    # the rows exercise every branch of the rule
    assert removed_rows > 50 and emptied > 10 and kept_by_score > 10 and ties > 20 and with0 > 50 and with1 > 50, \
        (removed_rows, emptied, kept_by_score, ties, with0, with1)


def test_forced_prune_by_hand():
    """three children, total 100, sq = 10 (+ 5e-10): c* = child 0 with score 0.5 + 2 * 0.5 * sq / 61 = 0.6639...; child 1
    (N 30, Q 0.2, P 0.3: F = ceil(sqrt(60)) = 8, lo = 22) scores 0.2 + 6 / (1 + m) < target from m = 12 on, so N' = lo = 22;
    child 2 (N 10, Q -0.5, P 0.2: F = ceil(sqrt(40)) = 7, lo = 3) scores below the target at every m >= 3: N' = 3"""
    got, removed = _capi.forced_prune(2.0, 2.0, [60, 30, 10], [30.0, 6.0, -5.0], [0.5, 0.3, 0.2])
    assert got.tolist() == [60, 22, 3] and removed == 15
    assert forced.prune(2.0, 2.0, [60, 30, 10], [30.0, 6.0, -5.0], [0.5, 0.3, 0.2]).tolist() == [60, 22, 3]
    # target 0.5 + 17 / 97 = 0.675...; child 1 (Q 0, score 1 / (1 + m)) is below it from m = 1 on and a child left with a single
    # playout loses it; child 2 had only one, which the same score keeps (m = 0 scores 1.0); child 3 (Q -1) loses its one
    got, removed = _capi.forced_prune(2.0, 2.0, [96, 2, 1, 1], [48.0, 0.0, 0.0, -1.0], [0.85, 0.05, 0.05, 0.05])
    assert got.tolist() == [96, 0, 1, 0] and removed == 3
    assert forced.prune(2.0, 2.0, [96, 2, 1, 1], [48.0, 0.0, 0.0, -1.0], [0.85, 0.05, 0.05, 0.05]).tolist() == [96, 0, 1, 0]


# ---------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_forced_prune_refuses_bad_arguments():
    ok = ([3, 1], [1.0, 0.0], [0.5, 0.5])
    for k in (0.0, -1.0, 16.5, float("nan")):
        with pytest.raises(ValueError):
            _capi.forced_prune(k, 2.0, *ok)
    with pytest.raises(ValueError):
        _capi.forced_prune(2.0, 2.0, [0, 0], [0.0, 0.0], [0.5, 0.5])          # no visit at all
    with pytest.raises(ValueError):
        _capi.forced_prune(2.0, 2.0, [3, -1], [1.0, 0.0], [0.5, 0.5])
    with pytest.raises(ValueError):
        _capi.forced_prune(2.0, 2.0, [3, 1], [1.0], [0.5, 0.5])
    with pytest.raises(ValueError):
        _capi.forced_prune(2.0, 2.0, [], [], [])
    L = _capi.lib()
    out = np.zeros(2, np.int32)
    assert L.az_forced_prune(2.0, 2.0, 2, None, None, None, out.ctypes.data_as(C.c_void_p)) == -1


def test_setters_refuse_a_null_engine():
    L = _capi.lib()
    k, p = C.c_double(7.0), C.c_int(7)
    assert L.az_set_forced_playouts(None, 2.0, 1) == -1
    assert L.az_get_forced_playouts(None, C.byref(k), C.byref(p)) == -1 and k.value == 7.0 and p.value == 7


def test_check_forced_playouts():
    assert check_forced_playouts(None) is None
    assert check_forced_playouts({"k": 2}) == {"k": 2.0, "prune": True}
    assert check_forced_playouts({"k": 16, "prune": 0}) == {"k": 16.0, "prune": False}
    for bad in ({}, {"prune": True}, {"k": 0}, {"k": -2.0}, {"k": 16.1}, {"k": float("nan")}, {"k": 2, "prunes": True}):
        with pytest.raises(ValueError):
            check_forced_playouts(bad)
    assert az.self_play.check_forced_playouts is check_forced_playouts


def test_seams_validate_and_refuse_subtree_reuse():
    m = SelfPlayManager(None, "cuda:0", forced_playouts={"k": 2.0})
    assert m.forced_playouts == {"k": 2.0, "prune": True} and SelfPlayManager(None, "cuda:0").forced_playouts is None
    with pytest.raises(ValueError):
        SelfPlayManager(None, "cuda:0", subtree_reuse=True, forced_playouts={"k": 2.0})
    with pytest.raises(ValueError):
        SelfPlayManager(None, "cuda:0", forced_playouts={"k": 20.0})
    fn = lambda state: None
    assert MCTS(fn, 10, 2.0, forced_playouts={"k": 4, "prune": False}).forced_playouts == {"k": 4.0, "prune": False}
    assert MCTS(fn, 10, 2.0).forced_playouts is None
    with pytest.raises(ValueError):
        MCTS(fn, 10, 2.0, forced_playouts={"k": 0.0})


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick: the numpy search with the rule off is the oracle's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,S,L", [(5, 4, 64, 1), (9, 5, 64, 1), (15, 5, 64, 1), (9, 5, 64, 4), (5, 4, 42, 4), (5, 4, 1100, 1)])
def test_helper_with_the_rule_off_is_oracle_search(n, k, S, L):
    """visits, W, priors and action; with L > 1 the oracle's virtual-loss batches (42 = ten batches of four and one of two)"""
    o = orc.Oracle(n, k, S, synthetic=True, virtual_loss=0 if L == 1 else L)
    for stones, seed in ((0, 1), (6, 2), (11, 3)):
        board, player, last = forced.random_position(n, k, stones, seed)
        rs = np.random.RandomState(seed + 100)
        for noise in (rs.dirichlet([0.3] * int((board == 0).sum())), None):
            for T in (1.0, 1e-9):
                u = rs.random_sample()
                want = o.search(None, board, player, last, T, noise, u)
                got = forced.search_move(o.synth_eval, n, k, S, board, player, last, T, noise, u, 0.0, L=L)
                assert np.array_equal(got["N"], want["N"]) and np.array_equal(got["W"], want["W"]) and np.array_equal(got["P"], want["P"])
                assert got["action"] == want["action"] and got["N"].sum() == S


def test_helper_forcing_changes_the_tree_and_keeps_the_budget():
    n, k, S = 5, 4, 64
    o = orc.Oracle(n, k, S, synthetic=True)
    board, player, last = forced.random_position(n, k, 6, 2)
    noise = np.random.RandomState(5).dirichlet([0.3] * 19)
    off = forced.search(o.synth_eval, n, k, S, board, player, last, noise, 0.0)
    on = forced.search(o.synth_eval, n, k, S, board, player, last, noise, 2.0)
    assert on["N"].sum() == off["N"].sum() == S and not np.array_equal(on["N"], off["N"]) and np.array_equal(on["P"], off["P"])
    # without noise the rule is off whatever k says
    assert np.array_equal(forced.search(o.synth_eval, n, k, S, board, player, last, None, 2.0)["N"],
                          forced.search(o.synth_eval, n, k, S, board, player, last, None, 0.0)["N"])
