"""az_search_batch / Engine.search_batch / MCTS.run_many: what can be checked without a GPU -- the C-ABI declares and
exports the entry point, a NULL engine is refused without a crash, the wrapper's shape checks run before the library is
called, and run_many draws from numpy's global RNG in the order a loop of run() does."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import ROOT

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi, games
from alphazero_piskvorky_amd.controller import PolicyValueFn
from alphazero_piskvorky_amd.mcts import MCTS


def test_entry_point_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        h = f.read()
    assert "int az_search_batch(az_engine *e, int slot, int count," in h
    assert "az_search_batch" in _capi.EXPORTS
    assert hasattr(_capi.lib(), "az_search_batch")          # ctypes resolves the symbol or raises AttributeError


def test_null_engine_is_refused_without_a_crash():
    b = np.zeros(25, np.uint8); p = np.ones(1, np.uint8); la = np.full(1, -1, np.int16)
    T = np.ones(1, np.float64); u = np.full(1, 0.5, np.float64)
    pi = np.full(25, 7.0, np.float32)
    rc = _capi.lib().az_search_batch(None, 0, 1, _capi._p(b), _capi._p(p), _capi._p(la), _capi._p(T), None, _capi._p(u),
                                     _capi._p(pi), None, None, None, None)
    assert rc == -1                                          # AZ_ERR_INVALID
    assert (pi == 7.0).all()


def _bare_engine(n=5):
    """the wrapper object without az_create: every ValueError below is raised before the library is reached"""
    e = az.Engine.__new__(az.Engine)
    e.n, e.nn, e.h = n, n * n, C.c_void_p()
    return e


def test_search_batch_shape_checks_raise_before_the_library_is_called():
    e = _bare_engine(5)
    B = np.zeros((3, 25), np.uint8); pl = [1, 2, 1]; la = [-1, -1, -1]
    with pytest.raises(ValueError, match="boards"):
        e.search_batch(np.zeros((3, 24), np.uint8), pl, la, 1.0)
    with pytest.raises(ValueError, match="boards"):
        e.search_batch(np.zeros((3, 5, 4), np.uint8), pl, la, 1.0)
    with pytest.raises(ValueError, match="boards"):
        e.search_batch(np.zeros(25, np.uint8), [1], [-1], 1.0)
    with pytest.raises(ValueError, match="players and lasts"):
        e.search_batch(B, [1, 2], la, 1.0)
    with pytest.raises(ValueError, match="players and lasts"):
        e.search_batch(B, pl, [-1] * 4, 1.0)
    with pytest.raises(ValueError, match="temperature"):
        e.search_batch(B, pl, la, [1.0, 0.5])
    with pytest.raises(ValueError, match="u must"):
        e.search_batch(B, pl, la, 1.0, u=[0.5, 0.5])
    with pytest.raises(ValueError, match="one array per position"):
        e.search_batch(B, pl, la, 1.0, noise=[np.ones(25)] * 2)
    B2 = B.copy(); B2[1, 3] = 1
    with pytest.raises(ValueError, match=r"noise\[1\] must have one entry per legal cell \(24\)"):
        e.search_batch(B2, pl, [-1, 3, -1], 1.0, noise=[np.ones(25)] * 3)
    # the [count, n, n] form passes the checks (and then reaches the library, which refuses the NULL engine)
    with pytest.raises(az.AzError, match=r"az_search_batch failed \(-1\)"):
        e.search_batch(np.zeros((3, 5, 5), np.uint8), pl, la, [1.0, 0.5, 1e-8], noise=[np.ones(25)] * 3, u=[0.1, 0.2, 0.3])


class _RecordingEngine:
    """stands in for both of MCTS's engines: records the (noise, u) pairs it is handed, returns a fixed legal answer"""

    def __init__(self, n):
        self.n, self.nn, self.calls = n, n * n, []

    def _answer(self, cells):
        a = int(np.flatnonzero(np.asarray(cells).reshape(-1) == 0)[0])
        pi = np.zeros(self.nn, np.float32); pi[a] = 1.0
        N = np.zeros(self.nn, np.int32); N[a] = 3
        return a, pi, N

    def search(self, cells, player, last, temperature, noise=None, u=0.5, slot=0):
        self.calls.append((None if noise is None else np.array(noise), float(u), float(temperature)))
        a, pi, N = self._answer(cells)
        return dict(action=a, pi=pi, N=N, W=np.zeros(self.nn), P=pi.copy())

    def search_batch(self, boards, players, lasts, temperature, noise=None, u=None, slot=0):
        boards = np.asarray(boards).reshape(-1, self.nn)
        out = dict(action=[], pi=[], N=[])
        for i in range(len(boards)):
            self.calls.append((None if noise is None else np.array(noise[i]), float(u[i]), float(temperature[i])))
            a, pi, N = self._answer(boards[i])
            out["action"].append(a); out["pi"].append(pi); out["N"].append(N)
        return {k: np.array(v) for k, v in out.items()}


def _states(n=5, k=4):
    rs = np.random.RandomState(4)
    out = []
    for stones in (0, 3, 25, 7, 24, 25, 1):          # two full boards, one of them in the middle of the list
        s = games.Gomoku(n, k)
        cells = np.zeros(n * n, np.uint8)
        where = rs.permutation(n * n)[:stones]
        cells[where] = 1 + (np.arange(stones) & 1)
        s.cells = cells
        s.current_player = "X" if stones % 2 == 0 else "O"
        s.last_action = None if stones == 0 else (int(where[-1]) // n, int(where[-1]) % n)
        out.append(s)
    return out


@pytest.mark.parametrize("add_noise", [False, True])
def test_run_many_draws_in_the_order_of_a_loop_of_run(add_noise):
    states = _states()
    temps = [1.0, 0.7, 0.5, 1e-8, 0.3, 0.2, 0.9]
    loop_eng, many_eng = _RecordingEngine(5), _RecordingEngine(5)
    m1 = MCTS(PolicyValueFn(None), num_simulations=8, c_puct=2.0)
    m1._eng = lambda n, k: loop_eng
    m2 = MCTS(PolicyValueFn(None), num_simulations=8, c_puct=2.0)
    m2._eng_batch = lambda n, k, count: many_eng
    np.random.seed(12)
    r1 = [m1.run(s, T, add_root_noise=add_noise) for s, T in zip(states, temps)]
    after1 = np.random.random_sample()
    np.random.seed(12)
    r2 = m2.run_many(states, temps, add_root_noise=add_noise)
    after2 = np.random.random_sample()
    assert after1 == after2                                   # the global RNG was advanced by exactly the same draws
    assert len(loop_eng.calls) == len(many_eng.calls) == 5    # the full boards reach no engine
    for (nz1, u1, T1), (nz2, u2, T2) in zip(loop_eng.calls, many_eng.calls):
        assert u1 == u2 and T1 == T2
        assert (nz1 is None and nz2 is None) if not add_noise else np.array_equal(nz1, nz2)
    assert len(r2) == len(states)
    for (pi1, a1), (pi2, a2) in zip(r1, r2):
        assert a1 == a2 and np.array_equal(pi1, pi2) and pi2.shape == (5, 5) and pi2.dtype == np.float32
    assert r2[2][1] is None and r2[5][1] is None and not r2[2][0].any()
    assert m2.last_visits.shape == (len(states), 5, 5) and not m2.last_visits[2].any() and m2.last_visits[0].sum() == 3


def test_run_many_refuses_mixed_board_sizes_and_bad_temperature_lists():
    m = MCTS(PolicyValueFn(None), num_simulations=8, c_puct=2.0)
    with pytest.raises(ValueError, match="differ in board size"):
        m.run_many([games.Gomoku(5, 4), games.Gomoku(9, 5)], 1.0)
    with pytest.raises(ValueError, match="temperature"):
        m.run_many([games.Gomoku(5, 4)] * 3, [1.0, 0.5])
    assert m.run_many([], 1.0) == []


def test_run_many_with_a_plain_callable_is_the_loop_of_run():
    calls = []
    m = MCTS(lambda s: (np.full((5, 5), 0.04, np.float32), 0.0), num_simulations=4, c_puct=2.0)
    m.run = lambda s, T, add_root_noise=False: (calls.append((s, float(T), add_root_noise)),
                                                setattr(m, "last_visits", np.ones((5, 5), np.int32)),
                                                (np.zeros((5, 5), np.float32), (0, 0)))[-1]
    states = _states()[:2]
    out = m.run_many(states, [1.0, 0.5], add_root_noise=True)
    assert [c[0] for c in calls] == states and [c[1] for c in calls] == [1.0, 0.5] and all(c[2] for c in calls)
    assert len(out) == 2 and m.last_visits.shape == (2, 5, 5) and m.last_visits.sum() == 50
