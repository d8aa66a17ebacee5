"""MCTS-Solver (az_set_solver), the parts that need no GPU: the numpy restatement in tests/solver.py with the option off is
Oracle.search bit for bit; with it on every status it proves is the brute-force minimax value; az_solver_counts is the rule's N';
the crafted positions prove what they are meant to; and the Python seams validate the option."""
import ctypes as C
import functools
import os
import re
import zlib

import numpy as np
import pytest

from oracle import oracle as orc
from tests import solver as sv
from tests.util import ROOT

from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.evaluator import ModelEvaluator
from alphazero_piskvorky_amd.mcts import MCTS, check_solver
from alphazero_piskvorky_amd.self_play import SelfPlayManager

NEW = ("az_set_solver", "az_get_solver", "az_last_proof", "az_selfplay_proofs", "az_solver_counts", "az_solver_stops")


def test_symbols_are_exported_declared_and_listed():
    L = _capi.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        header = f.read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s
    assert (_capi.PROOF_UNKNOWN, _capi.PROOF_WIN, _capi.PROOF_LOSS, _capi.PROOF_DRAW) == (sv.UNKNOWN, sv.WIN, sv.LOSS, sv.DRAW) == (0, 1, 2, 3)
    for name, val in (("AZ_PROOF_UNKNOWN", 0), ("AZ_PROOF_WIN", 1), ("AZ_PROOF_LOSS", 2), ("AZ_PROOF_DRAW", 3)):
        assert re.search(r"\b%s = %d\b" % (name, val), header), name


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick: the numpy search with the option off is the oracle's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(5, 4), (9, 5)])
def test_restatement_with_the_option_off_is_oracle_search(n, k):
    S = 64
    o = orc.Oracle(n, k, S, synthetic=True)
    for stones, seed in ((0, 1), (6, 2), (11, 3)):
        board, player, last = sv.random_position(n, k, stones, seed)
        rs = np.random.RandomState(seed + 100)
        for noise in (rs.dirichlet([0.3] * int((board == 0).sum())), None):
            for T in (1.0, 1e-9):
                u = rs.random_sample()
                want = o.search(None, board, player, last, T, noise, u)
                got = sv.search_move(o.synth_eval, n, k, S, board, player, last, T, noise, u, solver=False)
                assert np.array_equal(got["N"], want["N"]) and np.array_equal(got["W"], want["W"]) and np.array_equal(got["P"], want["P"])
                assert got["action"] == want["action"] and got["N"].sum() == S
                assert got["root"] == sv.UNKNOWN and not got["st"].any() and np.array_equal(got["Np"], got["N"])


# ---------------------------------------------------------------------------------------------------------------------
# soundness: every proven status is the minimax value
# ---------------------------------------------------------------------------------------------------------------------
def hashed_eval(n):
    """a position-hashed random evaluator: priors and value drawn from a RandomState seeded by the position"""
    def evaluate(board, player, last):
        rs = np.random.RandomState(zlib.crc32(bytes(board) + bytes([int(player)])))
        return rs.dirichlet([0.5] * (n * n)).astype(np.float32), float(np.float32(rs.uniform(-0.9, 0.9)))
    return evaluate


MINIMAX_CASES = ((3, 3, 0, 100), (3, 3, 2, 100), (3, 3, 4, 100), (4, 3, 4, 300), (4, 4, 6, 300))


@functools.lru_cache(maxsize=None)
def minimax_run(n, k, stones, S):
    """(searches, proven roots, proven root edges, wrong statuses) over the seeds 0..5 and the two evaluators"""
    memo, searches, roots, edges, wrong = {}, 0, 0, 0, []
    for seed in range(6):
        board, player, last = sv.random_position(n, k, stones, seed)
        for name, ev in (("uniform", sv.constant_eval(n)), ("hashed", hashed_eval(n))):
            r = sv.search(ev, n, k, S, board, player, last)
            searches += 1
            if r["root"] != sv.UNKNOWN:
                roots += 1
                if r["root"] != sv.minimax(board.copy(), player, n, k, memo):
                    wrong.append((seed, name, "root"))
            for a in np.flatnonzero(r["st"]):
                edges += 1
                if r["st"][a] != sv.minimax_edge(board, player, int(a), n, k, memo):
                    wrong.append((seed, name, int(a)))
            # the root's own status is the rule applied to its row
            assert r["root"] == sv.node_status(r["st"], board == 0), (seed, name)
            assert r["N"].sum() == S
    return searches, roots, edges, tuple(wrong)


@pytest.mark.parametrize("n,k,stones,S", MINIMAX_CASES)
def test_every_proven_status_is_the_minimax_value(n, k, stones, S):
    searches, roots, edges, wrong = minimax_run(n, k, stones, S)
    assert searches == 12 and not wrong, wrong
    print(f"{n}x{n} k={k} stones={stones} S={S}: {roots} of {searches} roots and {edges} root edges proven")
    if (n, k, stones) in ((3, 3, 4), (4, 3, 4)):
        assert roots > 0 and edges > 0          # these two cases keep the test from being vacuous


# ---------------------------------------------------------------------------------------------------------------------
# az_solver_counts = the rule
# ---------------------------------------------------------------------------------------------------------------------
def test_solver_counts_equals_the_rule_on_random_rows():
    rs = np.random.RandomState(20261019)
    kinds = dict(nothing=0, win=0, survivor=0, no_survivor=0, all_loss=0)
    for trial in range(400):
        count = int(rs.randint(1, 226))
        N = rs.multinomial(int(rs.choice([1, 32, 400, 5000])), rs.dirichlet([0.15] * count)).astype(np.int32)
        mode = trial % 5
        if mode == 0:
            st = np.zeros(count, np.int8)
        elif mode == 1:
            st = rs.randint(0, 4, count).astype(np.int8)
            st[rs.randint(count)] = sv.WIN
        elif mode == 2:                                         # LOSS edges and a visited survivor
            st = rs.choice([0, 2, 3], count).astype(np.int8)
            st[int(np.argmax(N))] = sv.UNKNOWN
        elif mode == 3:                                         # LOSS edges, every edge that is not LOSS unvisited
            st = rs.choice([0, 2, 3], count).astype(np.int8)
            st[N > 0] = sv.LOSS
        else:
            st = np.full(count, sv.LOSS, np.int8)
        want = sv.solver_counts(N, st)
        got = _capi.solver_counts(N, st)
        assert got.dtype == np.int32 and np.array_equal(got, want), (trial, N, st, want, got)
        if (st == sv.WIN).any():
            kinds["win"] += 1
            assert np.array_equal(got, np.where(st == sv.WIN, N, 0))
        elif (st == sv.LOSS).all():
            kinds["all_loss"] += 1
            assert np.array_equal(got, N)
        elif not (st == sv.LOSS).any():
            kinds["nothing"] += 1
            assert np.array_equal(got, N)
        elif ((st != sv.LOSS) & (N > 0)).any():
            kinds["survivor"] += 1
            assert not got[st == sv.LOSS].any() and np.array_equal(got[st != sv.LOSS], N[st != sv.LOSS])
        else:
            kinds["no_survivor"] += 1
            assert np.array_equal(got, N)
    assert min(kinds.values()) >= 20, kinds


def test_solver_counts_by_hand():
    assert _capi.solver_counts([5, 3, 2], [0, 0, 0]).tolist() == [5, 3, 2]
    assert _capi.solver_counts([5, 3, 2], [2, 1, 3]).tolist() == [0, 3, 0]
    assert _capi.solver_counts([5, 3, 2, 1], [1, 0, 1, 2]).tolist() == [5, 0, 2, 0]
    assert _capi.solver_counts([5, 3, 2], [2, 0, 3]).tolist() == [0, 3, 2]
    assert _capi.solver_counts([5, 3, 0], [2, 2, 0]).tolist() == [5, 3, 0]          # the only survivor has no visit
    assert _capi.solver_counts([5, 3, 2], [2, 2, 2]).tolist() == [5, 3, 2]


def test_solver_counts_refuses_bad_arguments():
    for bad in (([], []), ([1, 2], [0]), ([1, -1], [0, 0]), ([1, 1], [0, 4]), ([1, 1], [0, -1])):
        with pytest.raises(ValueError):
            _capi.solver_counts(*bad)
    L = _capi.lib()
    out = np.zeros(2, np.int32)
    assert L.az_solver_counts(2, None, None, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.az_set_solver(None, 1) == -1 and L.az_get_solver(None) == -1
    assert L.az_last_proof(None, 0, None, None, None) == -1 and L.az_solver_stops(None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the crafted positions
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted_a_tree(n, k, S):
    board, player, last, win = sv.crafted_a(n, k)
    info = {}
    return sv.search(sv.constant_eval(n), n, k, S, board, player, last, info=info), info


@functools.lru_cache(maxsize=None)
def crafted_b_tree(n, k, S):
    board, player, last, ends = sv.crafted_b(n, k)
    lg = np.zeros(n * n, np.float32)
    lg[list(ends)] = 6.0
    return sv.search(sv.constant_eval(n, lg), n, k, S, board, player, last)


@pytest.mark.parametrize("n,k,S", [(5, 4, 64), (9, 5, 128), (15, 5, 256)])
def test_crafted_a_the_single_winning_cell(n, k, S):
    board, player, last, win = sv.crafted_a(n, k)
    r, info = crafted_a_tree(n, k, S)
    assert r["root"] == sv.WIN and np.flatnonzero(r["st"]).tolist() == [win] and r["st"][win] == sv.WIN
    # every cell before the winning one got its single visit, every simulation from the discovery on lands on the winning cell
    before = int((board[:win] == 0).sum())
    assert r["N"][win] == S - before == info["terminals"] and info["stops"] == 0
    legal = board == 0
    assert sv.solver_counts(r["N"][legal], r["st"][legal]).sum() == r["N"][win]
    # at T -> 0 pi is exactly one-hot and every u plays the winning cell; at T = 1 the unchanged temperature path leaves an
    # emptied cell what it leaves an unvisited one today, log(0 + 1e-8): a share of 1e-8 / N' of pi, below float32's spacing at 1
    for u in (0.0, 0.999):
        m = sv.search_move(sv.constant_eval(n), n, k, S, board, player, last, 1e-9, None, u)
        assert m["action"] == win and m["value"] == 1.0 and m["pi"][win] == 1.0 and m["pi"].sum() == 1.0
        assert np.count_nonzero(m["pi"]) == 1
    m = sv.search_move(sv.constant_eval(n), n, k, S, board, player, last, 1.0, None, 0.5)
    assert m["action"] == win and m["value"] == 1.0 and m["pi"][win] == 1.0 and np.delete(m["pi"], win).max() < 1e-8


@pytest.mark.parametrize("n,k,S,legal,proven", [(5, 4, 100, 19, True), (9, 5, 100, 73, False), (9, 5, 200, 73, True),
                                                (15, 5, 400, 217, False), (15, 5, 512, 217, True)])
def test_crafted_b_every_move_loses(n, k, S, legal, proven):
    board, player, last, ends = sv.crafted_b(n, k)
    assert int((board == 0).sum()) == legal
    r = crafted_b_tree(n, k, S)
    if not proven:
        assert r["root"] == sv.UNKNOWN and 0 < int((r["st"] == sv.LOSS).sum()) < legal
        return
    assert r["root"] == sv.LOSS and (r["st"][board == 0] == sv.LOSS).all()
    assert np.array_equal(sv.solver_counts(r["N"][board == 0], r["st"][board == 0]), r["N"][board == 0])
    lg = np.zeros(n * n, np.float32)
    lg[list(ends)] = 6.0
    m = sv.search_move(sv.constant_eval(n, lg), n, k, S, board, player, last, 1.0, None, 0.5)
    assert m["value"] == -1.0 and np.array_equal(m["Np"], m["N"])


# ---------------------------------------------------------------------------------------------------------------------
# the Python seams
# ---------------------------------------------------------------------------------------------------------------------
def test_check_solver_and_the_seams():
    assert check_solver(False) is False and check_solver(None) is False and check_solver(True) is True and check_solver(1) is True
    for kw in (dict(subtree_reuse=True), dict(virtual_loss=4), dict(forced_playouts={"k": 2.0, "prune": True}),
               dict(gumbel={"m": 16}), dict(evaluator=object())):
        with pytest.raises(ValueError):
            check_solver(True, **kw)
        assert check_solver(False, **kw) is False
    assert SelfPlayManager(None, "cuda:0", solver=True).solver is True and SelfPlayManager(None, "cuda:0").solver is False
    for kw in (dict(subtree_reuse=True), dict(virtual_loss=4), dict(forced_playouts={"k": 2.0}), dict(gumbel={"m": 16})):
        with pytest.raises(ValueError):
            SelfPlayManager(None, "cuda:0", solver=True, **kw)
    fn = lambda state: None
    assert MCTS(fn, 10, 2.0).solver is False and MCTS(fn, 10, 2.0).last_proof is None
    with pytest.raises(ValueError):
        MCTS(fn, 10, 2.0, solver=True)          # a plain callable is an outside evaluator
    assert ModelEvaluator(device="cuda:0", solver=True).solver is True and ModelEvaluator(device="cuda:0").solver is False
    with pytest.raises(ValueError):
        ModelEvaluator(device="cuda:0", solver=True, virtual_loss=4)
    with pytest.raises(ValueError):
        ModelEvaluator(device="cuda:0", solver=True, evaluators=True)
