"""ModelEvaluator seam (evaluator.py:14-122): all arena games run concurrently in the HIP engine with two
weight sets (candidate = X = slot 0, baseline = O = slot 1, odd games start with O).  With torch.distributed
initialised the games are split over the ranks in even-aligned blocks and the W/L/D tally is all-reduced, so every
rank returns the same result (and takes the same promotion decision)."""
import numpy as np
import torch

from . import constants as _c
from . import parallel
from ._capi import AZ_MAX_SIMULATIONS, Engine, check_candidates, check_rng, check_selection, check_threat_search, win_rule_name
from .controller import device_index, make_batch_policy_value_fn, merge_batch_evaluators, model_kind
from .mcts import check_solver, numpy_log_table
from .options import apply_options, bring_candidates, bring_selection, check_combination, switched_on
from .self_play import check_resign


def temperature_schedule(move: int) -> float:
    return _c.EVAL_TEMPERATURE * np.exp(-move / _c.EVAL_TEMPERATURE_SCHEDULE_HALFTIME)


class ModelEvaluator:
    def __init__(self, game_class=None, print_games=False, device=None, seed=None, virtual_loss=1, eval_cache=0,
                 start_positions=None, resign: dict = None, evaluators=None, solver: bool = False, win_rule: str = None,
                 threat_search: dict = None, selection: dict = None, candidates: dict = None, rng: str = None):
        self.game_class = game_class
        # where the arena's move uniforms come from: "numpy" (the default) or "philox", made on the GPU (az_set_rng)
        self.rng = check_rng(rng)
        # which game the arena plays: "freestyle" (constants.WIN_RULE's default) or "exact" (standard Gomoku; az_set_win_rule)
        self.win_rule = win_rule_name(_c.WIN_RULE if win_rule is None else win_rule)
        # opt-in: the arena's evaluations leave the engine (az_set_external_evaluator).  A (candidate, baseline) pair of
        # controller.BatchPolicyValueFn, one BatchPolicyValueFn that serves both nets by its `net` argument, or True = the
        # two controllers' own torch modules, wrapped at every evaluate().
        self.evaluators = evaluators if evaluators is None or evaluators is True else merge_batch_evaluators(evaluators)
        self.print_games = print_games
        self.device = device if device is not None else torch.device("cuda")
        self.seed = seed
        self.virtual_loss = virtual_loss      # opt-in search upgrades (mcts.py:17-22 TODO), see include/az_engine.h
        self.eval_cache = eval_cache
        # opt-in: (boards, players, lasts); games 2i and 2i+1 both start from position i mod count, the second with the
        # colours exchanged, so every position is played once from either side
        self.start_positions = start_positions
        # opt-in: dict(threshold, min_ply=0); an arena game ends as a loss of the mover once the search value of a ply falls
        # below -threshold.  No arena game is exempt: a `playout` share is accepted and has no effect here.
        self.resign = check_resign(resign)
        # opt-in MCTS-Solver in both sides' searches (az_set_solver).  Not with virtual_loss > 1 or outside evaluators.
        self.solver = check_solver(solver, virtual_loss=virtual_loss, evaluator=self.evaluators)
        # opt-in root threat search in both sides' searches, dict(max_depth=8, node_budget=256) or True (az_set_threat_search).
        # Needs solver=True.
        self.threat_search = check_threat_search(threat_search, self.solver)
        # opt-in selection rule in both sides' searches, dict(fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0)
        # (az_set_selection).  Not with solver.
        self.selection = check_selection(selection)
        check_combination(switched_on(selection=self.selection, solver=self.solver), "selection")
        # opt-in candidate moves in both sides' searches, dict(radius=r) (az_set_candidates).  Not with solver, selection or
        # evaluators.
        self.candidates = check_candidates(candidates)
        check_combination(switched_on(candidates=self.candidates, solver=self.solver, selection=self.selection,
                                      evaluator=self.evaluators), "candidates")
        self._engine = None

    def evaluate(self, candidate_controller, baseline_controller, num_games=20, debug=False):
        candidate_controller.net.eval()
        baseline_controller.net.eval()
        n = candidate_controller.net.board_size
        k = min(_c.WIN_LENGTH, n)
        S = _c.NUM_EVAL_SIMULATIONS
        import torch.distributed as td
        rank, world = (td.get_rank(), td.get_world_size()) if td.is_available() and td.is_initialized() else (0, 1)
        lo, hi = parallel.arena_block(num_games, rank, world)
        mine = hi - lo
        dev = torch.device("cuda", device_index(self.device))
        key = (n, k, S, max(mine, 1), model_kind(candidate_controller.net), self.virtual_loss, self.eval_cache)
        if self._engine is None or self._key != key:
            if self._engine is not None:
                self._engine.close()
            self._engine = Engine(n, k, S, max(1, min(mine, _c.CONCURRENT_GAMES)), c_puct=_c.EVAL_EXPLORATION_CONSTANT,
                                  device=device_index(self.device), log_table=numpy_log_table(S), model=key[4],
                                  deep=S > AZ_MAX_SIMULATIONS)
            self._engine.set_virtual_loss(self.virtual_loss)
            self._engine.set_eval_cache(self.eval_cache)
            self._key = key
        eng = self._engine
        if self.evaluators is None:
            eng.load_weights(candidate_controller.net.state_dict(), 0)
            eng.load_weights(baseline_controller.net.state_dict(), 1)
        elif self.evaluators is True:
            make_batch_policy_value_fn((candidate_controller.net, baseline_controller.net), self.device).attach(eng)
        elif not eng.external_evaluator():
            self.evaluators.attach(eng)
        T = np.array([float(temperature_schedule(m)) for m in range(n * n + 2)], dtype=np.float64)
        seed0 = self.seed if self.seed is not None else int(np.random.randint(0, 2 ** 31 - 1))
        if self.seed is None:
            seed0 = parallel.broadcast_seed(seed0, dev)
        self.win_rule = win_rule_name(self.win_rule)
        self.resign = check_resign(self.resign)
        self.solver = check_solver(self.solver, virtual_loss=self.virtual_loss, evaluator=self.evaluators)
        self.threat_search = check_threat_search(self.threat_search, self.solver)
        self.selection = check_selection(self.selection)
        check_combination(switched_on(selection=self.selection, solver=self.solver), "selection")
        self.candidates = check_candidates(self.candidates)
        check_combination(switched_on(candidates=self.candidates, solver=self.solver, selection=self.selection,
                                      evaluator=self.evaluators), "candidates")
        self.rng = check_rng(self.rng)
        # first=lo is even (parallel.arena_block): no pair of games from one start position is torn apart.  The arena has no
        # playout cap, forced playouts or Gumbel root search: its roots are not noised.
        bring_candidates(eng, self.candidates, before=True)
        bring_selection(eng, self.selection, before=True)
        apply_options(eng, win_rule=self.win_rule, start_positions=self.start_positions, first=lo, resign=self.resign,
                      playout_cap=None, forced_playouts=None, gumbel=None, solver=self.solver, threat_search=self.threat_search,
                      rng=self.rng)
        bring_selection(eng, self.selection, before=False)
        bring_candidates(eng, self.candidates, before=False)
        r = eng.arena(mine, seed0=seed0 + lo, temperature_table=T) if mine > 0 else {"wins": 0, "losses": 0, "draws": 0, "total": 0, "win_rate": 0.0}
        if world > 1:
            w, l, d = parallel.all_reduce_tally(r["wins"], r["losses"], r["draws"], dev, engine=eng)
            tot = w + l + d
            r = dict(r, wins=w, losses=l, draws=d, total=tot, win_rate=(w + 0.5 * d) / tot if tot else 0.0)   # evaluator.py:106-109
        if debug:
            print(f"[Evaluator]: Candidate Win Rate: {r['win_rate']:.2%} (W:{r['wins']} L:{r['losses']} D:{r['draws']})")
        self.last_result = r
        return r["win_rate"], {"wins": r["wins"], "losses": r["losses"], "draws": r["draws"], "total": r["total"],
                               "win_rate": r["win_rate"]}
