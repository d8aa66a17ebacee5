"""The selection rule (az_set_selection), the parts that need no GPU: the exported symbols, the two tables against their formulas,
the restatement of tests/selection.py against Oracle.search with the rule off, the argument checks of the seams, train's flags
-- and that the cases tests/test_selection_gpu.py compares are not vacuous.

Non-vacuity, counted by test_the_cases_are_not_vacuous: over the 72 single searches of the GPU file (3 sizes x 3 positions x with
and without noise x 4 parameter sets, S = 64, c_puct = 3) the restatement's root visits differ from the plain search's in every
one; the selections whose argmax differs from the plain rule's on the same tree state number 4 to 62 at the root and 2 to 91
below it per search (2894 and 3082 in all, of 72 x 64 root selections).  The nine un-noised (a) searches visit 11, 2, 14 (5x5),
42, 45, 1 (9x9) and 45, 1, 1 (15x15) distinct root children where the plain rule visits 4, 17, 12, 10, 27, 11, 16, 13 and 11:
wide where the root's value is high, narrow where it is low, as the issue describes."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import forced
from tests import selection as sel
from tests.util import ROOT

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi, options
from alphazero_piskvorky_amd import train as train_mod
from alphazero_piskvorky_amd.evaluator import ModelEvaluator
from alphazero_piskvorky_amd.mcts import MCTS
from alphazero_piskvorky_amd.self_play import SelfPlayManager

NEW = ("az_set_selection", "az_get_selection", "az_selection_tables")
S1 = 64


def test_symbols_are_exported_declared_and_bound():
    L = _capi.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        header = f.read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s
    assert L.az_set_selection.argtypes is not None and L.az_get_selection.argtypes is not None
    for name in ("set_selection", "selection"):
        assert callable(getattr(az.Engine, name))
    assert callable(_capi.selection_tables)


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
def test_mass_table_is_the_square_root_exactly():
    _, mass = _capi.selection_tables(2.0, 19652.0, 0.0, 64)
    assert mass.dtype == np.float64 and mass.shape == (4097,)
    assert np.array_equal(mass, np.sqrt(np.arange(4097) / 4096.0))
    assert mass[0] == 0.0 and mass[4096] == 1.0


@pytest.mark.parametrize("S", [1, 64, 1024, 1100, 65534])
@pytest.mark.parametrize("c_puct,base,factor", [(2.0, 19652.0, 1.0), (3.0, 50.0, 1.0), (1.25, 1.0, 16.0), (4.0, 500.5, 0.3)])
def test_cpuct_table_is_the_formula_within_one_ulp(S, c_puct, base, factor):
    cp, _ = _capi.selection_tables(c_puct, base, factor, S)
    assert cp.dtype == np.float64 and cp.shape == (S + 2,)
    i = np.arange(S + 2, dtype=np.float64)
    want = c_puct + factor * np.log((i + base + 1.0) / base)
    assert np.all(np.abs(cp - want) <= np.spacing(want)), float(np.max(np.abs(cp - want) / np.spacing(want)))
    assert np.all(np.diff(cp) >= 0.0) and cp[0] >= c_puct


@pytest.mark.parametrize("c_puct", [2.0, 3.0, 0.1, 1e-3, 7.7])
def test_cpuct_table_is_c_puct_exactly_without_a_factor(c_puct):
    for base in (1.0, 50.0, 19652.0):
        cp, _ = _capi.selection_tables(c_puct, base, 0.0, 1100)
        assert np.all(cp == c_puct)


def test_selection_tables_refuses_bad_arguments():
    for bad in ((2.0, 0.5, 1.0, 64), (2.0, 50.0, -0.1, 64), (2.0, 50.0, 16.5, 64), (2.0, float("nan"), 1.0, 64),
                (2.0, float("inf"), 1.0, 64), (float("nan"), 50.0, 1.0, 64), (2.0, 50.0, 1.0, 0), (2.0, 50.0, 1.0, 65535)):
        with pytest.raises(ValueError):
            _capi.selection_tables(*bad)
    L = _capi.lib()
    assert L.az_selection_tables(2.0, 50.0, 1.0, 64, None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", sel.SIZES)
def test_with_the_rule_off_the_restatement_is_the_oracles_search(n, k):
    o = orc.Oracle(n, k, S1, c_puct=sel.C_PUCT, synthetic=True)
    for i, p in enumerate(sel.positions(n, k)):
        for noise in (None, p["noise"]):
            want = o.search(None, p["board"], p["player"], p["last"], p["T"], noise, p["u"])
            got = sel.search_move(o.synth_eval, n, k, S1, p["board"], p["player"], p["last"], p["T"], noise, p["u"], c_puct=sel.C_PUCT)
            for key in ("N", "W", "P", "pi"):
                assert np.array_equal(got[key], want[key]), (n, i, noise is not None, key)
            assert got["action"] == want["action"]
            plain = forced.search(o.synth_eval, n, k, S1, p["board"], p["player"], p["last"], noise, 0.0, sel.C_PUCT)
            assert all(np.array_equal(got[key], plain[key]) for key in ("N", "W", "P"))


def test_the_visited_mass_is_an_integer_sum_of_floors():
    P = np.array([0.5, 0.25, 2.0 ** -25, 1.0 - 2.0 ** -24, 0.1], np.float32)
    vis = np.array([True, True, True, True, False])
    assert sel.visited_mass(P, vis) == (1 << 23) + (1 << 22) + 0 + ((1 << 24) - 1)
    assert sel.visited_mass(P, ~vis) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 24))


def test_the_cases_are_not_vacuous():
    """every single search of the GPU file: other root visits than the plain search, and selections that differ from the plain
    rule's both at the root and below it (the module docstring has the counts)"""
    root = below = 0
    lo = [10 ** 9, 10 ** 9]
    for n, k in sel.SIZES:
        ev = orc.Oracle(n, k, 1, synthetic=True).synth_eval
        for i, p in enumerate(sel.positions(n, k)):
            for noise in (None, p["noise"]):
                off = forced.search(ev, n, k, S1, p["board"], p["player"], p["last"], noise, 0.0, sel.C_PUCT)
                for name, s in sel.SETS.items():
                    info = {}
                    on = sel.search(ev, n, k, S1, p["board"], p["player"], p["last"], noise, 0.0, sel.C_PUCT, sel=s, info=info)
                    assert on["N"].sum() == off["N"].sum() == S1
                    assert not np.array_equal(on["N"], off["N"]), (n, i, noise is not None, name)
                    assert info["root_diff"] > 0 and info["below_diff"] > 0, (n, i, noise is not None, name, info)
                    root += info["root_diff"]; below += info["below_diff"]
                    lo = [min(lo[0], info["root_diff"]), min(lo[1], info["below_diff"])]
    assert lo[0] >= 1 and lo[1] >= 1 and root > 72 and below > 72


def test_the_self_play_cases_are_not_vacuous():
    from tests.test_playout_cap_cpu import np_full
    for n, k, seed0, G in ((5, 4, 5300, 6), (9, 5, 5400, 3)):
        ev = orc.Oracle(n, k, 1, synthetic=True).synth_eval
        for cap in (None, (8, 500)):
            for g in range(G):
                on = sel.selfplay_game(ev, n, k, 32, seed0 + g, sel.SETS["c"], cap=cap, full_fn=np_full)
                off = sel.selfplay_game(ev, n, k, 32, seed0 + g, None, cap=cap, full_fn=np_full)
                assert on["root_diff"] > 0 and on["below_diff"] > 0, (n, cap, g)
                assert on["visits"].shape != off["visits"].shape or not np.array_equal(on["visits"], off["visits"]), (n, cap, g)


# ---------------------------------------------------------------------------------------------------------------------
# the third table and the seams
# ---------------------------------------------------------------------------------------------------------------------
def test_the_third_table_refuses_each_new_pair_and_passes_each_member_alone():
    assert len(options.SELECTION_CONFLICTS) == 3
    assert {frozenset(r[:2]) for r in options.SELECTION_CONFLICTS} == {frozenset(("selection", x)) for x in ("subtree_reuse", "solver", "gumbel")}
    for a, b, message in options.SELECTION_CONFLICTS:
        with pytest.raises(ValueError, match=re.escape(message)):
            options.check_combination({a, b})
        with pytest.raises(ValueError, match=re.escape(message)):
            options.check_combination({a, b}, of="selection")
        options.check_combination({a})
        options.check_combination({b})
        options.check_combination({a, b}, of="playout_cap")          # a rule that does not speak of the option asked about
    # the threat search falls with the solver it needs
    with pytest.raises(ValueError, match="threat_search needs solver"):
        options.check_combination({"selection", "threat_search"})
    # everything else combines
    options.check_combination({"selection", "virtual_loss", "leaf_symmetry", "playout_cap", "forced_playouts"})
    options.check_combination({"selection", "evaluator", "virtual_loss", "forced_playouts"})
    assert options.switched_on(selection=None) == set() and options.switched_on(selection=dict(sel.SETS["a"])) == {"selection"}


def test_check_selection():
    assert _capi.check_selection(None) is None and _capi.check_selection(False) is None
    assert _capi.check_selection({}) == _capi.check_selection(True) == dict(fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0)
    assert _capi.check_selection({"cpuct_factor": 1, "cpuct_base": 50}) == dict(fpu=0.2, fpu_root=0.0, cpuct_base=50.0, cpuct_factor=1.0)
    for bad in ({"fpu": -0.1}, {"fpu": 2.1}, {"fpu_root": 2.5}, {"fpu_root": float("nan")}, {"cpuct_base": 0.5}, {"cpuct_base": float("inf")},
                {"cpuct_factor": -1.0}, {"cpuct_factor": 16.5}, {"fpu": float("inf")}, {"k": 2.0}, {"fpu": 0.2, "on": True}, 0.2, [0.2]):
        with pytest.raises(ValueError):
            _capi.check_selection(bad)


class _NoEngine:
    """stands where a seam would build an engine: nothing may reach it"""
    def __getattr__(self, name):
        raise AssertionError(f"the seam touched an engine ({name})")


def _controller(n=5):
    import torch
    from alphazero_piskvorky_amd.controller import NeuralNetworkController
    from alphazero_piskvorky_amd.net import GomokuNet
    return NeuralNetworkController(GomokuNet(board_size=n), device=torch.device("cpu"))


def test_the_seams_refuse_bad_keys_ranges_and_pairs_before_an_engine_exists(monkeypatch):
    def fn(state):
        raise AssertionError("never evaluated")
    monkeypatch.setattr("alphazero_piskvorky_amd.mcts.Engine", _NoEngine)
    monkeypatch.setattr("alphazero_piskvorky_amd.self_play.Engine", _NoEngine)
    monkeypatch.setattr("alphazero_piskvorky_amd.evaluator.Engine", _NoEngine)
    for bad in ({"fpu": 3.0}, {"cpuct_base": 0.0}, {"cpuct_factor": 17.0}, {"fpu_root": -1.0}, {"reduction": 0.2}):
        with pytest.raises(ValueError):
            MCTS(fn, 16, 2.0, selection=bad)
        with pytest.raises(ValueError):
            SelfPlayManager(None, "cuda:0", selection=bad)
        with pytest.raises(ValueError):
            ModelEvaluator(selection=bad)
    good = dict(sel.SETS["c"])
    assert MCTS(fn, 16, 2.0, selection=good).selection == good
    assert MCTS(fn, 16, 2.0, selection={"fpu": 0.3}).selection == dict(fpu=0.3, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0)
    assert MCTS(fn, 16, 2.0).selection is None
    with pytest.raises(ValueError, match="Gumbel"):
        MCTS(fn, 16, 2.0, selection=good, gumbel={"m": 4})
    m = SelfPlayManager(None, "cuda:0", selection=good, virtual_loss=4, forced_playouts={"k": 2.0}, playout_cap={"fast_sims": 8})
    assert m.selection == good
    for other, match in ((dict(subtree_reuse=True), "subtree_reuse"), (dict(gumbel={"m": 4}), "Gumbel"), (dict(solver=True), "solver")):
        with pytest.raises(ValueError, match=match):
            SelfPlayManager(None, "cuda:0", selection=good, **other)
    m.selection = {"fpu": 9.0}                                           # the options are plain attributes: checked again per episode
    with pytest.raises(ValueError):
        m._check_options()
    with pytest.raises(ValueError, match="solver"):
        ModelEvaluator(selection=good, solver=True)
    assert ModelEvaluator(selection=good).selection == good


class _StubEngine:
    """records what bring_selection does to it"""
    def __init__(self, have=None):
        self.have = dict(_capi.SELECTION_DEFAULTS, on=False) if have is None else dict(have, on=True)
        self.calls = []

    def selection(self):
        return dict(self.have)

    def set_selection(self, fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0, on=True):
        self.calls.append(("set", on))
        self.have = dict(fpu=fpu, fpu_root=fpu_root, cpuct_base=cpuct_base, cpuct_factor=cpuct_factor, on=on) if on else dict(self.have, on=False)


def test_bring_selection_goes_off_before_and_on_after():
    a, c = dict(sel.SETS["a"]), dict(sel.SETS["c"])
    e = _StubEngine()
    options.bring_selection(e, None, before=True); options.bring_selection(e, None, before=False)
    assert e.calls == []                                                  # off stays off: the engine is not touched
    options.bring_selection(e, a, before=True)
    assert e.calls == []
    options.bring_selection(e, a, before=False)
    assert e.calls == [("set", True)] and e.selection() == dict(a, on=True)
    options.bring_selection(e, a, before=True); options.bring_selection(e, a, before=False)
    assert e.calls == [("set", True)]                                     # the same option again: nothing to do
    options.bring_selection(e, c, before=True)
    assert e.calls[-1] == ("set", False)                                  # another one: off first ...
    options.bring_selection(e, c, before=False)
    assert e.calls[-1] == ("set", True) and e.selection() == dict(c, on=True)     # ... then on
    options.bring_selection(e, None, before=True)
    assert e.calls[-1] == ("set", False) and not e.selection()["on"]      # a seam without the option brings a cached engine back
    n = len(e.calls)
    options.bring_selection(e, None, before=False)
    assert len(e.calls) == n


# ---------------------------------------------------------------------------------------------------------------------
# train's flags
# ---------------------------------------------------------------------------------------------------------------------
def test_train_flags():
    errors = []
    f = train_mod.selection_from_flags
    assert f(errors.append, None, None, None, None) is None and not errors
    assert f(errors.append, 0.2, None, None, None) == {"fpu": 0.2}
    assert f(errors.append, 0.3, 0.1, 50.0, 1.0) == {"fpu": 0.3, "fpu_root": 0.1, "cpuct_base": 50.0, "cpuct_factor": 1.0}
    assert f(errors.append, None, None, None, 1.0) == {"cpuct_factor": 1.0}
    assert f(errors.append, None, 0.1, 50.0, 1.0) == {"cpuct_factor": 1.0, "fpu_root": 0.1, "cpuct_base": 50.0}
    assert f(errors.append, 0.0, None, None, None) == {"fpu": 0.0} and not errors      # 0 is a value, not "not given"
    for lonely in ((None, 0.1, None, None), (None, None, 50.0, None), (None, 0.1, 50.0, None)):
        errors.clear()
        assert f(errors.append, *lonely) is None
        assert errors == ["--fpu-root and --cpuct-base need --fpu or --cpuct-factor"]
    # what the flags give is what the seams take
    assert _capi.check_selection(f(errors.append, None, None, 50.0, 1.0)) == dict(fpu=0.2, fpu_root=0.0, cpuct_base=50.0, cpuct_factor=1.0)


def test_train_main_parses_the_flags(monkeypatch):
    seen = {}
    monkeypatch.setattr(train_mod, "run", lambda *a, **kw: seen.update(kw))
    monkeypatch.setattr("sys.argv", ["train", "--fpu", "0.25", "--cpuct-factor", "1", "--cpuct-base", "100"])
    train_mod.main()
    assert seen["selection"] == {"fpu": 0.25, "cpuct_base": 100.0, "cpuct_factor": 1.0}
    monkeypatch.setattr("sys.argv", ["train"])
    train_mod.main()
    assert seen["selection"] is None
    monkeypatch.setattr("sys.argv", ["train", "--fpu-root", "0.1"])
    with pytest.raises(SystemExit):
        train_mod.main()
