"""options.py without a GPU: the conflict table read by one function, the order in which apply_options calls an engine's setters
(a stub engine that records them), and the command-line helper of train.py."""
import pytest

from alphazero_piskvorky_amd import options
from alphazero_piskvorky_amd.options import apply_options, check_combination, option_from_flags, switched_on


class StubEngine:
    """An engine's option setters and getters over a dict; `calls` is what apply_options did to it, in order."""
    nn = 25

    def __init__(self):
        self.state = dict(win_rule="freestyle", start=0, resign=0.0, cap=0, forced=0.0, gumbel=0, solver=False, threat=(0, 0))
        self.calls = []

    def _set(self, name, key, value):
        self.calls.append(name)
        self.state[key] = value

    def win_rule(self): return self.state["win_rule"]
    def start_positions(self): return self.state["start"]
    def resign(self): return {"threshold": self.state["resign"]}
    def playout_cap(self): return {"fast_sims": self.state["cap"]}
    def forced_playouts(self): return {"k": self.state["forced"]}
    def gumbel(self): return {"m": self.state["gumbel"]}
    def solver(self): return self.state["solver"]
    def threat_search(self): return self.state["threat"]

    def set_win_rule(self, rule):
        assert self.state["start"] == 0, "the rule changes while start positions validated under the other rule are set"
        self._set(f"win_rule {rule}", "win_rule", rule)

    def clear_start_positions(self): self._set("start off", "start", 0)
    def set_start_positions(self, boards, players, lasts, first=0): self._set(f"start on first={first}", "start", len(players))
    def set_resign(self, threshold, min_ply=0, playout=0.0): self._set("resign on" if threshold else "resign off", "resign", threshold)
    def set_playout_cap(self, fast_sims, full=0.25, export_full_only=True): self._set(f"cap {fast_sims} {export_full_only}", "cap", fast_sims)
    def set_forced_playouts(self, k, prune=True): self._set(f"forced {k}", "forced", k)
    def set_gumbel(self, m, c_visit=50.0, c_scale=1.0): self._set(f"gumbel {m}", "gumbel", m)

    def set_solver(self, on):
        assert on or self.state["threat"][0] == 0, "the solver goes off under the threat search that needs it"
        self._set(f"solver {bool(on)}", "solver", bool(on))

    def set_threat_search(self, max_depth=8, node_budget=256):
        assert max_depth == 0 or self.state["solver"], "the threat search goes on without the solver"
        self._set(f"threat {max_depth}", "threat", (max_depth, node_budget if max_depth else 0))


A = dict(win_rule="exact", start_positions=([[0] * 25], [1], [-1]), first=6, resign={"threshold": 0.9, "min_ply": 4, "playout": 0.1},
         playout_cap=None, forced_playouts=None, gumbel=None, solver=True, threat_search={"max_depth": 8, "node_budget": 256})
B = dict(win_rule="freestyle", start_positions=None, first=0, resign=None, playout_cap={"fast_sims": 10, "full": 0.25, "train_on_fast": True},
         forced_playouts=None, gumbel={"m": 64, "c_visit": 50.0, "c_scale": 1.0}, solver=False, threat_search=None)
OFF = dict(win_rule="freestyle", start_positions=None, first=0, resign=None, playout_cap=None, forced_playouts=None, gumbel=None,
           solver=False, threat_search=None)


def test_apply_options_orders_the_setters():
    e = StubEngine()
    assert apply_options(e, **OFF) is e and e.calls == []                 # a new engine with nothing asked for: no setter at all
    apply_options(e, **A)
    assert e.calls == ["win_rule exact", "start on first=6", "resign on", "solver True", "threat 8"]
    e.calls.clear()
    apply_options(e, **B)
    # start positions go before the rule changes, the threat search before the solver, and all of that before anything goes on
    assert e.calls == ["start off", "win_rule freestyle", "resign off", "threat 0", "solver False", "cap 10 False", "gumbel 25"]     # m clamped to n * n
    e.calls.clear()
    apply_options(e, **A)
    assert e.calls == ["win_rule exact", "cap 0 True", "gumbel 0", "start on first=6", "resign on", "solver True", "threat 8"]
    e.calls.clear()
    apply_options(e, **A)                                                 # again: what is set is set again, nothing is cleared
    assert e.calls == ["start on first=6", "resign on", "threat 8"]
    e.calls.clear()
    apply_options(e, **dict(OFF, forced_playouts={"k": 2.0, "prune": False}))
    assert e.calls == ["start off", "win_rule freestyle", "resign off", "threat 0", "solver False", "forced 2.0"]
    assert e.state == dict(win_rule="freestyle", start=0, resign=0.0, cap=0, forced=2.0, gumbel=0, solver=False, threat=(0, 0))


def test_the_table_is_read_by_one_function():
    names = {"subtree_reuse", "virtual_loss", "leaf_symmetry", "evaluator", "playout_cap", "forced_playouts", "gumbel", "solver"}
    assert all({a, b} <= names and a != b for a, b, _ in options.CONFLICTS)
    assert switched_on(subtree_reuse=False, virtual_loss=1, leaf_symmetry=None, gumbel=None, solver=False) == set()
    assert switched_on(subtree_reuse=True, virtual_loss=4, gumbel={}, solver=1, evaluator=object()) == {"subtree_reuse", "virtual_loss", "gumbel", "solver", "evaluator"}
    check_combination(set())
    check_combination({"playout_cap", "forced_playouts", "leaf_symmetry", "virtual_loss"})
    for a, b, message in options.CONFLICTS:
        with pytest.raises(ValueError) as err:
            check_combination({a, b})
        assert str(err.value) == message
        check_combination({a})
        check_combination({b})
    with pytest.raises(ValueError, match="needs solver"):
        check_combination({"threat_search"})
    check_combination({"threat_search", "solver"})
    # of: only the rules of one option
    with pytest.raises(ValueError, match="Gumbel root search does not combine with subtree_reuse"):
        check_combination({"evaluator", "subtree_reuse", "gumbel"}, "gumbel")
    check_combination({"evaluator", "subtree_reuse"}, "gumbel")


def test_option_from_flags():
    errors = []
    assert option_from_flags(errors.append, {"m": None, "c_visit": None}, "needs m") is None and not errors
    assert option_from_flags(errors.append, {"m": 16, "c_visit": None, "c_scale": 0.5}, "needs m") == {"m": 16, "c_scale": 0.5}
    assert option_from_flags(errors.append, {"m": None, "c_visit": 1.0}, "needs m") is None and errors == ["needs m"]
