"""Candidate moves (az_set_candidates), the parts that need no GPU: az_candidate_mask against a brute-force Chebyshev mask, the
exported symbols and their argument checks, the restatement of tests/candidates.py against the oracle (its two yardsticks), the
seams' refusals -- and that the cases tests/test_candidates_gpu.py compares are not vacuous.

Yardsticks: the masked softmax with every cell a candidate is the oracle's P bit for bit, and the search with radius 0 has
Oracle.search's visit counts (and W, P, pi, action).  Non-vacuity: on every (size, position, radius) case with radius 1 or 2 and
at least one stone, the plain search puts a visit outside C or its root counts differ from the restatement's."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import candidates as cd
from tests import forced
from tests.util import ROOT, build_weights

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi, options
from alphazero_piskvorky_amd import train as train_mod
from alphazero_piskvorky_amd.evaluator import ModelEvaluator
from alphazero_piskvorky_amd.mcts import MCTS
from alphazero_piskvorky_amd.self_play import SelfPlayManager

NEW = ("az_set_candidates", "az_get_candidates", "az_candidate_mask")
S1 = 32


# ---------------------------------------------------------------------------------------------------------------------
# 1. the mask
# ---------------------------------------------------------------------------------------------------------------------
def _boards(n):
    nn = n * n
    rs = np.random.RandomState(100 + n)
    out = []
    for stones in (0, 1, 2, n, nn // 2, nn - 1, nn):
        b = np.zeros(nn, np.uint8)
        b[rs.permutation(nn)[:stones]] = rs.randint(1, 3, size=stones)
        out.append(b)
    mid = n // 2
    for r, c in ((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (0, mid), (mid, 0), (mid, n - 1), (n - 1, mid)):
        b = np.zeros(nn, np.uint8)
        b[r * n + c] = 1
        out.append(b)
    if n == 15:
        for cell in (63, 64, 127, 128, 191, 192, 224):             # the word boundaries of the 4 x 64-bit plane
            b = np.zeros(nn, np.uint8)
            b[cell] = 2
            out.append(b)
    return out


@pytest.mark.parametrize("n", range(3, 16))
def test_mask_equals_brute_force(n):
    for b in _boards(n):
        stones = int((b != 0).sum())
        for radius in range(1, n):
            got = _capi.candidate_mask(b, n, radius)
            assert got.dtype == np.uint8 and got.shape == (n * n,)
            assert np.array_equal(got.astype(bool), cd.candidate_mask(b, n, radius)), (n, stones, radius)
            if stones == 0:
                assert got.all()
            elif stones == n * n:
                assert not got.any()
            else:
                assert got.any() and not got[b != 0].any()
        assert np.array_equal(_capi.candidate_mask(b, n, n - 1).astype(bool), (b == 0) if stones else np.ones(n * n, bool))
        assert np.array_equal(_capi.candidate_mask(b, n, 0).astype(bool), b == 0)      # off: the empty cells


def test_the_brute_force_mask_is_the_definition_cell_by_cell():
    """the numpy mask itself, against two nested loops on one board with stones at a corner, an edge and the middle"""
    n = 7
    b = np.zeros(n * n, np.uint8)
    b[[0, 3 * n + 6, 4 * n + 3]] = (1, 2, 1)
    for radius in (1, 2, 3):
        want = np.zeros(n * n, bool)
        for j in range(n * n):
            want[j] = b[j] == 0 and any(b[s] and max(abs(j // n - s // n), abs(j % n - s % n)) <= radius for s in range(n * n))
        assert np.array_equal(cd.candidate_mask(b, n, radius), want)
    # no wrap across a row's end: (4, 0) follows the stone at (3, 6) in cell order and is 6 columns away from it
    assert not cd.candidate_mask(b, n, 1)[4 * n] and not _capi.candidate_mask(b, n, 1)[4 * n]
    assert cd.candidate_mask(b, n, 1)[2 * n + 5] and cd.candidate_mask(b, n, 1)[1 * n + 1]


# ---------------------------------------------------------------------------------------------------------------------
# 2. symbols and arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    L = _capi.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        header = f.read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes is not None
    for name in ("set_candidates", "candidates"):
        assert callable(getattr(az.Engine, name))
    assert callable(_capi.candidate_mask) and callable(_capi.check_candidates)


def test_layouts_are_unchanged():
    assert len(_capi.az_counters._fields_) == 21 and len(_capi.az_config._fields_) == 12 and len(_capi.az_selfplay_args._fields_) == 7


def test_null_and_out_of_range_arguments_are_refused():
    L = _capi.lib()
    b = np.zeros(25, np.uint8)
    m = np.zeros(25, np.uint8)
    bp, mp = b.ctypes.data, m.ctypes.data
    assert L.az_candidate_mask(5, bp, 1, mp) == 0
    for bad in ((2, bp, 1, mp), (16, bp, 1, mp), (5, None, 1, mp), (5, bp, 1, None), (5, bp, -1, mp), (5, bp, 5, mp)):
        assert L.az_candidate_mask(*bad) == -1, bad
    b[3] = 3
    assert L.az_candidate_mask(5, bp, 1, mp) == -1                 # a cell holds 0, 1 or 2
    assert L.az_set_candidates(None, 1) == -1 and L.az_get_candidates(None, None) == -1
    for bad in ((np.zeros(24, np.uint8), 5, 1), (np.zeros(25, np.uint8), 5, 5), (np.zeros(25, np.uint8), 5, -1)):
        with pytest.raises(ValueError):
            _capi.candidate_mask(*bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the two yardsticks, and non-vacuity
# ---------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net(n, k):
    if n not in _NETS:
        onet = orc.Net(n, build_weights(n))
        _NETS[n] = (onet, cd.net_evaluator(n, k, onet))
    return _NETS[n]


@pytest.mark.parametrize("n,k", cd.SIZES)
def test_the_masked_softmax_over_all_cells_is_the_oracles(n, k):
    o = orc.Oracle(n, k, 1)
    onet, _ = net(n, k)
    for p in cd.positions(n, k):
        logits, P, _ = onet.eval(o.encode(p["board"], p["player"], p["last"]))
        got = cd.masked_softmax(logits, np.ones(n * n, bool))
        assert got.dtype == np.float32 and np.array_equal(got, P)
        # ... and over the legal cells it is another vector as soon as a stone is on the board
        if (p["board"] != 0).any():
            legal = cd.masked_softmax(logits, p["board"] == 0)
            assert not np.array_equal(legal, P) and not legal[p["board"] != 0].any() and abs(float(legal.sum()) - 1.0) < 1e-5


def test_the_canonical_wave_sum():
    """lane partials in ascending cell order, then the butterfly: by hand on four lanes' worth of cells"""
    vals = np.zeros(225, np.float32)
    vals[[3, 67, 131, 35]] = np.float32([1.0, 2.0 ** -24, 2.0 ** -24, 1.0])
    # lane 3 adds 1 + 2^-24 (rounds to 1) + 2^-24 (rounds to 1); then lane 3 + lane 35 = 2
    assert cd.wave_sum(vals, np.flatnonzero(vals), np.float32) == np.float32(2.0)
    assert cd.wave_sum(vals.astype(np.float64), np.flatnonzero(vals), np.float64) == 2.0 + 2.0 ** -23


@pytest.mark.parametrize("n,k", cd.SIZES)
def test_with_radius_0_the_restatement_is_the_oracles_search(n, k):
    o = orc.Oracle(n, k, S1, c_puct=cd.C_PUCT)
    onet, ev = net(n, k)
    for i, p in enumerate(cd.positions(n, k)):
        for noise in (None, p["noise"]):
            want = o.search(onet, p["board"], p["player"], p["last"], p["T"], noise, p["u"])
            got = cd.search_move(ev, n, k, S1, p["board"], p["player"], p["last"], p["T"], noise, p["u"])
            for key in ("N", "W", "P", "pi"):
                assert np.array_equal(got[key], want[key]), (n, i, noise is not None, key)
            assert got["action"] == want["action"]


def test_with_radius_0_the_synthetic_restatement_is_the_oracles_search():
    n, k = 9, 5
    o = orc.Oracle(n, k, S1, c_puct=cd.C_PUCT, synthetic=True)
    for p in cd.positions(n, k):
        want = o.search(None, p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        got = cd.search_move(cd.synth_evaluator(n, k), n, k, S1, p["board"], p["player"], p["last"], p["T"], p["noise"], p["u"])
        assert all(np.array_equal(got[key], want[key]) for key in ("N", "W", "P", "pi")) and got["action"] == want["action"]


@pytest.mark.parametrize("n,k", [(9, 5), (15, 5)])
def test_the_cases_are_not_vacuous(n, k):
    """radius 1 and 2 on the 1-, 6- and 11-stone positions: the plain search has a visit outside C, or other root counts than
    the restatement; and the set is a proper subset of the legal cells"""
    _, ev = net(n, k)
    for i, p in enumerate(cd.positions(n, k)):
        if not (p["board"] != 0).any():
            continue
        plain = cd.search(ev, n, k, S1, p["board"], p["player"], p["last"], p["noise"])
        for radius in (1, 2):
            info = {}
            on = cd.search(ev, n, k, S1, p["board"], p["player"], p["last"], p["noise"], radius=radius, info=info)
            C = cd.candidate_mask(p["board"], n, radius)
            outside = int(plain["N"][~C].sum())
            assert on["N"].sum() == plain["N"].sum() == S1
            assert 0 < info["cand"] == int(C.sum()) < int((p["board"] == 0).sum()), (n, i, radius)
            assert not on["N"][~C].any() and not on["P"][~C].any()
            assert outside > 0 or not np.array_equal(on["N"], plain["N"]), (n, i, radius)


def test_the_rule_acts_below_the_root_and_through_the_normalisation():
    """on the empty board every cell is a root candidate, and radius 1 still changes the search; radius n-1 changes a 6-stone
    search through the priors alone"""
    n, k = 9, 5
    _, ev = net(n, k)
    p0, p6 = cd.positions(n, k)[0], cd.positions(n, k)[2]
    plain = cd.search(ev, n, k, S1, p0["board"], p0["player"], p0["last"], p0["noise"])
    on = cd.search(ev, n, k, S1, p0["board"], p0["player"], p0["last"], p0["noise"], radius=1)
    assert not (np.array_equal(plain["N"], on["N"]) and np.array_equal(plain["W"], on["W"]))
    plain = cd.search(ev, n, k, S1, p6["board"], p6["player"], p6["last"], p6["noise"])
    on = cd.search(ev, n, k, S1, p6["board"], p6["player"], p6["last"], p6["noise"], radius=n - 1)
    assert not np.array_equal(plain["P"], on["P"])
    assert not (np.array_equal(plain["N"], on["N"]) and np.array_equal(plain["W"], on["W"]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the seams
# ---------------------------------------------------------------------------------------------------------------------
def test_check_candidates():
    assert _capi.check_candidates(None) is None and _capi.check_candidates(False) is None
    assert _capi.check_candidates({"radius": 2}) == {"radius": 2} and _capi.check_candidates({"radius": np.int64(14)}) == {"radius": 14}
    for bad in ({}, {"radius": 0}, {"radius": -1}, {"radius": 15}, {"radius": 1.5}, {"radius": True}, {"radius": "2"}, {"r": 2},
                {"radius": 2, "on": True}, 2, [2], True):
        with pytest.raises(ValueError):
            _capi.check_candidates(bad)


def test_the_fourth_table_refuses_each_new_pair_and_passes_each_member_alone():
    partners = ("subtree_reuse", "gumbel", "solver", "selection", "evaluator")
    assert {frozenset(r[:2]) for r in options.CANDIDATE_CONFLICTS} == {frozenset(("candidates", x)) for x in partners}
    assert len(options.CANDIDATE_CONFLICTS) == len(partners) and len(options.SELECTION_CONFLICTS) == 3
    for a, b, message in options.CANDIDATE_CONFLICTS:
        with pytest.raises(ValueError, match=re.escape(message)):
            options.check_combination({a, b})
        with pytest.raises(ValueError, match=re.escape(message)):
            options.check_combination({a, b}, of="candidates")
        options.check_combination({a})
        options.check_combination({b})
        options.check_combination({a, b}, of="playout_cap")
    with pytest.raises(ValueError, match="threat_search needs solver"):
        options.check_combination({"candidates", "threat_search"})
    options.check_combination({"candidates", "virtual_loss", "leaf_symmetry", "playout_cap", "forced_playouts"})
    assert options.switched_on(candidates=None) == set() and options.switched_on(candidates={"radius": 1}) == {"candidates"}


class _NoEngine:
    """stands where a seam would build an engine: nothing may reach it"""
    def __getattr__(self, name):
        raise AssertionError(f"the seam touched an engine ({name})")


def test_the_seams_refuse_bad_keys_ranges_and_pairs_before_an_engine_exists(monkeypatch):
    def fn(state):
        raise AssertionError("never evaluated")
    from alphazero_piskvorky_amd.controller import PolicyValueFn
    monkeypatch.setattr("alphazero_piskvorky_amd.mcts.Engine", _NoEngine)
    monkeypatch.setattr("alphazero_piskvorky_amd.self_play.Engine", _NoEngine)
    monkeypatch.setattr("alphazero_piskvorky_amd.evaluator.Engine", _NoEngine)
    native = PolicyValueFn.__new__(PolicyValueFn)                        # stands for make_policy_value_fn(controller)
    for bad in ({"radius": 0}, {"radius": 15}, {"radius": 1.0}, {"reach": 2}, {}):
        with pytest.raises(ValueError):
            MCTS(native, 16, 2.0, candidates=bad)
        with pytest.raises(ValueError):
            SelfPlayManager(None, "cuda:0", candidates=bad)
        with pytest.raises(ValueError):
            ModelEvaluator(candidates=bad)
    good = {"radius": 2}
    assert MCTS(native, 16, 2.0, candidates=good).candidates == good and MCTS(native, 16, 2.0).candidates is None
    with pytest.raises(ValueError, match="own net"):
        MCTS(fn, 16, 2.0, candidates=good)                               # a plain callable is az_search_callback's evaluator
    for other, match in ((dict(gumbel={"m": 4}), "Gumbel"), (dict(solver=True), "solver"), (dict(selection={"fpu": 0.2}), "selection rule")):
        with pytest.raises(ValueError, match=match):
            MCTS(native, 16, 2.0, candidates=good, **other)
    m = SelfPlayManager(None, "cuda:0", candidates=good, virtual_loss=4, forced_playouts={"k": 2.0}, playout_cap={"fast_sims": 8},
                        leaf_symmetry=True)
    assert m.candidates == good
    for other, match in ((dict(subtree_reuse=True), "subtree_reuse"), (dict(gumbel={"m": 4}), "Gumbel"), (dict(solver=True), "solver"),
                         (dict(selection={"fpu": 0.2}), "selection rule")):
        with pytest.raises(ValueError, match=match):
            SelfPlayManager(None, "cuda:0", candidates=good, **other)
    m.candidates = {"radius": 99}                                        # the options are plain attributes: checked again per episode
    with pytest.raises(ValueError):
        m._check_options()
    for other, match in ((dict(solver=True), "solver"), (dict(selection={"fpu": 0.2}), "selection rule"), (dict(evaluators=True), "own net")):
        with pytest.raises(ValueError, match=match):
            ModelEvaluator(candidates=good, **other)
    assert ModelEvaluator(candidates=good).candidates == good


class _StubEngine:
    """records what bring_candidates does to it"""
    def __init__(self):
        self.radius, self.calls = 0, []

    def candidates(self):
        return self.radius

    def set_candidates(self, radius):
        self.calls.append(radius)
        self.radius = radius


def test_bring_candidates_goes_off_before_and_on_after():
    e = _StubEngine()
    options.bring_candidates(e, None, before=True); options.bring_candidates(e, None, before=False)
    assert e.calls == []                                                  # off stays off: the engine is not touched
    options.bring_candidates(e, {"radius": 2}, before=True)
    assert e.calls == []
    options.bring_candidates(e, {"radius": 2}, before=False)
    assert e.calls == [2]
    options.bring_candidates(e, {"radius": 2}, before=True); options.bring_candidates(e, {"radius": 2}, before=False)
    assert e.calls == [2]                                                 # the same option again: nothing to do
    options.bring_candidates(e, {"radius": 1}, before=True)
    assert e.calls == [2, 0]                                              # another one: off first ...
    options.bring_candidates(e, {"radius": 1}, before=False)
    assert e.calls == [2, 0, 1]                                           # ... then on
    options.bring_candidates(e, None, before=True)
    assert e.calls[-1] == 0 and e.candidates() == 0                       # a seam without the option brings a cached engine back
    options.bring_candidates(e, None, before=False)
    assert len(e.calls) == 4


def test_train_main_parses_the_flag(monkeypatch):
    seen = {}
    monkeypatch.setattr(train_mod, "run", lambda *a, **kw: seen.update(kw))
    monkeypatch.setattr("sys.argv", ["train", "--candidate-radius", "2"])
    train_mod.main()
    assert seen["candidates"] == {"radius": 2}
    monkeypatch.setattr("sys.argv", ["train"])
    train_mod.main()
    assert seen["candidates"] is None
