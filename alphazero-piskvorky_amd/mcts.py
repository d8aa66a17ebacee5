"""MCTS.run seam (mcts.py:87-183) over az_search: one position, the whole search on the GPU.

The reference's randomness comes from numpy's global legacy RNG in a fixed order per call --
np.random.dirichlet([alpha]*len(legal)) when add_root_noise, then one random_sample() inside
np.random.choice (mcts.py:114,177).  The shim makes the same two draws from the same global RNG and hands
them to the engine, so np.random.seed(s) reproduces the reference's choices."""
import numpy as np

from . import constants as _c
from ._capi import (AZ_MAX_SIMULATIONS, FORCED_K_MAX, GUMBEL_DEFAULTS, GUMBEL_M_MAX, Engine, check_candidates, check_selection, check_threat_search,
                    win_rule_name)
from .controller import BatchPolicyValueFn, PolicyValueFn, device_index, model_kind, weights_version
from .options import apply_options, bring_candidates, bring_selection, check_combination, switched_on


def numpy_log_table(S):
    """float32 log(N + 1e-8) exactly as mcts.py:161 evaluates it."""
    return np.log(np.arange(S + 1, dtype=np.float32) + 1e-8).astype(np.float32)


def check_forced_playouts(fp):
    """None, or the dict a seam takes: k in (0, 16] (KataGo: 2) and optional prune (default True: pi and the move are made
    from the pruned counts)."""
    if fp is None:
        return None
    extra = set(fp) - {"k", "prune"}
    if extra or "k" not in fp:
        raise ValueError(f"forced_playouts takes k and prune (k is required), got {sorted(fp)}")
    out = {"k": float(fp["k"]), "prune": bool(fp.get("prune", True))}
    if not 0.0 < out["k"] <= FORCED_K_MAX:
        raise ValueError(f"forced_playouts k must be in (0, {FORCED_K_MAX:g}], got {out['k']}")
    return out


def check_solver(solver, subtree_reuse=False, virtual_loss=1, forced_playouts=None, gumbel=None, evaluator=None):
    """bool(solver), the MCTS-Solver option of a seam (az_set_solver).  Raises ValueError for the combinations the engine refuses:
    subtree reuse, virtual-loss batching, forced playouts, the Gumbel root search and evaluators outside the engine."""
    if not solver:
        return False
    check_combination(switched_on(solver=True, subtree_reuse=subtree_reuse, virtual_loss=virtual_loss, forced_playouts=forced_playouts,
                                  gumbel=gumbel, evaluator=evaluator), "solver")
    return True


def check_gumbel(gumbel, subtree_reuse=False, virtual_loss=1, forced_playouts=None, evaluator=None):
    """None, or the dict a seam takes for the Gumbel root search (az_set_gumbel): m in 1..64 (default 16), c_visit >= 0 (50) and
    c_scale > 0 (1).  Raises ValueError for the combinations the engine refuses: subtree reuse, virtual-loss batching, forced
    playouts and an evaluator outside the engine (it returns priors, not logits)."""
    if gumbel is None:
        return None
    extra = set(gumbel) - set(GUMBEL_DEFAULTS)
    if extra:
        raise ValueError(f"gumbel takes m, c_visit and c_scale, got {sorted(gumbel)}")
    out = {"m": int(gumbel.get("m", GUMBEL_DEFAULTS["m"])), "c_visit": float(gumbel.get("c_visit", GUMBEL_DEFAULTS["c_visit"])),
           "c_scale": float(gumbel.get("c_scale", GUMBEL_DEFAULTS["c_scale"]))}
    if not 1 <= out["m"] <= GUMBEL_M_MAX:
        raise ValueError(f"gumbel m must be in 1..{GUMBEL_M_MAX}, got {out['m']}")
    if not (0.0 <= out["c_visit"] < float("inf")) or not (0.0 < out["c_scale"] < float("inf")):
        raise ValueError(f"gumbel needs c_visit >= 0 and c_scale > 0, both finite, got {out['c_visit']} and {out['c_scale']}")
    check_combination(switched_on(gumbel=out, subtree_reuse=subtree_reuse, virtual_loss=virtual_loss, forced_playouts=forced_playouts,
                                  evaluator=evaluator), "gumbel")
    return out


class MCTS:
    def __init__(self, policy_value_fn, num_simulations, c_puct, dirichlet_alpha=0.3, dirichlet_weight=0.25, virtual_loss=1,
                 forced_playouts=None, gumbel=None, solver=False, threat_search=None, selection=None, candidates=None):
        if not callable(policy_value_fn):
            raise TypeError("policy_value_fn must be callable: state -> (policy [n, n], value)")
        # make_policy_value_fn(controller): the leaves are evaluated inside the HIP engine.  Any other callable keeps the
        # reference's plugin seam (mcts.py:87-93): the tree stays on the GPU and every evaluation is one host round trip
        # (az_search_callback) -- compatible, not fast.
        # A BatchPolicyValueFn keeps the seam AND the speed: any torch net on the same GPU evaluates the leaves of all
        # searches together on device buffers (az_set_external_evaluator), run() and run_many() through az_search_batch.
        self._batched = isinstance(policy_value_fn, BatchPolicyValueFn)
        self._external = not self._batched and not isinstance(policy_value_fn, PolicyValueFn)
        self.policy_value_fn = policy_value_fn
        self.num_simulations = num_simulations
        self.c_puct = c_puct
        self.dirichlet_alpha = dirichlet_alpha
        self.dirichlet_weight = dirichlet_weight
        self.virtual_loss = virtual_loss      # opt-in: leaves per evaluation batch (az_set_virtual_loss); 1 = the reference's loop
        # opt-in: dict(k, prune=True), forced playouts and policy target pruning in the searches with add_root_noise
        # (az_set_forced_playouts); the others are untouched
        self.forced_playouts = check_forced_playouts(forced_playouts)
        # opt-in: dict(m=16, c_visit=50.0, c_scale=1.0), the Gumbel root search in the searches with add_root_noise (az_set_gumbel):
        # they draw np.random.gumbel(size=legal) where the others draw the Dirichlet sample.  Controller-backed evaluators only.
        self.gumbel = check_gumbel(gumbel, virtual_loss=virtual_loss, forced_playouts=self.forced_playouts,
                                   evaluator=policy_value_fn if (self._external or self._batched) else None)
        # opt-in: MCTS-Solver in every search (az_set_solver): proven wins, losses and draws; last_proof then holds the last
        # run()'s (edge statuses [n, n], root status), after run_many() one pair per state.  Controller-backed evaluators only.
        self.solver = check_solver(solver, virtual_loss=virtual_loss, forced_playouts=self.forced_playouts, gumbel=self.gumbel,
                                   evaluator=policy_value_fn if (self._external or self._batched) else None)
        # opt-in: dict(max_depth=8, node_budget=256) or True, the root threat search in front of every search (az_set_threat_search):
        # forced-four wins and forced blocks reach the solver as premarked root statuses.  Needs solver=True.
        self.threat_search = check_threat_search(threat_search, self.solver)
        # opt-in: dict(fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0), first-play urgency and visit-dependent c_puct
        # in every search (az_set_selection).  Not with gumbel or solver.
        self.selection = check_selection(selection)
        check_combination(switched_on(selection=self.selection, gumbel=self.gumbel, solver=self.solver), "selection")
        # opt-in: dict(radius=r), every search expands, noises and selects only the empty cells within r of a stone, the priors
        # normalised over them (az_set_candidates).  Controller-backed evaluators only; not with gumbel, solver or selection.
        self.candidates = check_candidates(candidates)
        check_combination(switched_on(candidates=self.candidates, gumbel=self.gumbel, solver=self.solver, selection=self.selection,
                                      evaluator=policy_value_fn if (self._external or self._batched) else None), "candidates")
        self.last_proof = None
        self._engine = None
        self._version = None
        self._batch_engine = None             # run_many's own engine; run() and its one-slot engine are untouched by it
        self._batch_version = None

    def _new_engine(self, n, k, slots, **evaluator):
        """an engine of this object's own with the searches' options; evaluator: device and model of the net that evaluates"""
        eng = Engine(n, k, self.num_simulations, slots, c_puct=self.c_puct, dirichlet_alpha=self.dirichlet_alpha,
                     dirichlet_weight=self.dirichlet_weight, log_table=numpy_log_table(self.num_simulations),
                     deep=self.num_simulations > AZ_MAX_SIMULATIONS, **evaluator)
        if not self._external:
            eng.set_virtual_loss(self.virtual_loss)
        # the rule is the state's (_ruled); games, and with them start positions, resignation and the playout cap, are not played here
        bring_candidates(eng, self.candidates, before=True)
        bring_selection(eng, self.selection, before=True)
        apply_options(eng, win_rule="freestyle", start_positions=None, first=0, resign=None, playout_cap=None,
                      forced_playouts=self.forced_playouts, gumbel=self.gumbel, solver=self.solver, threat_search=self.threat_search)
        bring_selection(eng, self.selection, before=False)
        return bring_candidates(eng, self.candidates, before=False)

    @staticmethod
    def _state_rule(state):
        """the win rule a state carries ("freestyle" | "exact"); a state object without the attribute plays the reference's game"""
        return win_rule_name(getattr(state, "win_rule", None))

    @staticmethod
    def _ruled(eng, rule):
        """the searches read the rule from the state, like board_size and win_length: a cached engine is set to it on reuse"""
        if getattr(eng, "_searched_rule", "freestyle") != rule:     # the engines here are this object's own: new ones are freestyle
            eng.set_win_rule(rule)
            eng._searched_rule = rule
        return eng

    def _root_noise(self, legal):
        """the draws of one noised root from numpy's global RNG: the Dirichlet sample, or Gumbel(0, 1) under gumbel=..."""
        if self.gumbel is not None:
            return np.random.gumbel(size=legal)
        return np.random.dirichlet([self.dirichlet_alpha] * legal)

    def _eng_external(self, n, k):
        if self._engine is None or (self._engine.n, self._engine.k) != (n, k):
            self._engine = self._new_engine(n, k, 1)
        return self._engine

    def _run_external(self, root_state, temperature, noise, u):
        from .games import Gomoku
        n, k, rule = root_state.board_size, root_state.win_length, self._state_rule(root_state)

        def evaluate(cells, player, last):
            g = Gomoku(n, k, rule)
            g.cells = cells
            g.current_player = _c.X if player == 1 else _c.O
            g.last_action = None if last < 0 else (last // n, last % n)
            return self.policy_value_fn(g)

        return self._ruled(self._eng_external(n, k), rule).search_callback(root_state.cells, root_state.player_code(), root_state.last_index(),
                                                        float(temperature), evaluate, noise, u)

    def _eng(self, n, k):
        ctrl = self.policy_value_fn.controller
        if self._engine is None or (self._engine.n, self._engine.k) != (n, k):
            self._engine = self._new_engine(n, k, 1, device=device_index(ctrl.device), model=model_kind(ctrl.net))
            self._version = None
        ver = weights_version(ctrl.net)
        if ver != self._version:
            self._engine.load_weights(ctrl.net.state_dict(), 0)
            self._version = ver
        return self._engine

    def run(self, root_state, temperature, add_root_noise=False):
        n = root_state.board_size
        legal = int((root_state.cells == 0).sum())
        if legal == 0:
            return np.zeros((n, n), dtype=np.float32), None            # mcts.py:152-153
        noise = self._root_noise(legal) if add_root_noise else None
        u = np.random.random_sample()
        if self._external:
            r = self._run_external(root_state, temperature, noise, u)
        elif self._batched:
            rb = self._ruled(self._eng_batch(n, root_state.win_length, 1), self._state_rule(root_state)).search_batch(
                np.asarray(root_state.cells, np.uint8).reshape(1, n * n), [root_state.player_code()], [root_state.last_index()],
                float(temperature), None if noise is None else [noise], [u])
            r = {key: val[0] for key, val in rb.items()}
        else:
            eng = self._ruled(self._eng(n, root_state.win_length), self._state_rule(root_state))
            r = eng.search(root_state.cells, root_state.player_code(), root_state.last_index(), float(temperature), noise, u)
            if self.solver:
                edges, root = eng.last_proof()
                self.last_proof = (edges.reshape(n, n), root)
        a = int(r["action"])
        self.last_visits = r["N"].reshape(n, n)
        return r["pi"].reshape(n, n), (a // n, a % n)

    # ---- many positions at once (az_search_batch) ----
    BATCH_MIN_SLOTS, BATCH_MAX_SLOTS = 64, 1024

    def _eng_batched_eval(self, n, k, count):
        """the engine of a BatchPolicyValueFn: no weights, the evaluator attached; slots as _eng_batch"""
        slots = 1 if count == 1 else self.BATCH_MIN_SLOTS
        while slots < min(count, self.BATCH_MAX_SLOTS):
            slots *= 2
        eng = self._batch_engine
        if eng is None or (eng.n, eng.k) != (n, k) or eng.slots < slots:
            if eng is not None:
                eng.close()
            eng = self._batch_engine = self._new_engine(n, k, slots, device=device_index(self.policy_value_fn.device))
            self.policy_value_fn.attach(eng)
        return eng

    def _eng_batch(self, n, k, count):
        """run_many's engine: slots = the next power of two >= count inside [64, 1024]; grows with a larger batch, never shrinks"""
        if self._batched:
            return self._eng_batched_eval(n, k, count)
        ctrl = self.policy_value_fn.controller
        slots = self.BATCH_MIN_SLOTS
        while slots < min(count, self.BATCH_MAX_SLOTS):
            slots *= 2
        eng = self._batch_engine
        if eng is None or (eng.n, eng.k) != (n, k) or eng.slots < slots:
            if eng is not None:
                eng.close()
            self._batch_engine = self._new_engine(n, k, slots, device=device_index(ctrl.device), model=model_kind(ctrl.net))
            self._batch_version = None
        ver = weights_version(ctrl.net)
        if ver != self._batch_version:
            self._batch_engine.load_weights(ctrl.net.state_dict(), 0)
            self._batch_version = ver
        return self._batch_engine

    def run_many(self, states, temperature, add_root_noise=False):
        """run() for every state of a list, searched together on the GPU: [(pi [n, n], move or None), ...].  Draws from
        numpy's global RNG in the order a loop of run() would -- per state the Dirichlet sample when add_root_noise, then
        one random_sample(); a state without a legal cell draws nothing -- so after np.random.seed(s) the result equals
        [run(s_i, T_i) for s_i in states].  temperature: a scalar or one value per state.  With a plain callable as the
        evaluator this IS that loop (az_search_callback: compatible, not fast)."""
        states = list(states)
        count = len(states)
        T = np.asarray(temperature, np.float64)
        if T.ndim == 0:
            T = np.full(count, float(T), np.float64)
        if T.shape != (count,):
            raise ValueError(f"temperature must be a scalar or have one entry per state ({count})")
        if count == 0:
            self.last_visits = np.zeros((0, 0, 0), np.int32)
            return []
        n, k = states[0].board_size, states[0].win_length
        if any((s.board_size, s.win_length) != (n, k) for s in states):
            raise ValueError("run_many: the states differ in board size or win length")
        rule = self._state_rule(states[0])
        if any(self._state_rule(s) != rule for s in states):
            raise ValueError("run_many: the states differ in their win rule")
        if self._external:
            out, visits = [], np.zeros((count, n, n), np.int32)
            for i, s in enumerate(states):
                out.append(self.run(s, T[i], add_root_noise))
                if out[-1][1] is not None:
                    visits[i] = self.last_visits
            self.last_visits = visits
            return out
        live, noise, us = [], [], []
        for i, s in enumerate(states):
            legal = int((s.cells == 0).sum())
            if legal == 0:
                continue                                                # mcts.py:152-153: nothing is drawn
            if add_root_noise:
                noise.append(self._root_noise(legal))
            us.append(np.random.random_sample())
            live.append(i)
        out = [(np.zeros((n, n), dtype=np.float32), None) for _ in range(count)]     # mcts.py:152-153 for the full boards
        visits = np.zeros((count, n, n), np.int32)
        if live:
            eng = self._ruled(self._eng_batch(n, k, len(live)), rule)
            r = eng.search_batch(np.stack([np.asarray(states[i].cells, np.uint8).reshape(n * n) for i in live]),
                                 [states[i].player_code() for i in live], [states[i].last_index() for i in live],
                                 T[live], noise if add_root_noise else None, us)
            for j, i in enumerate(live):
                a = int(r["action"][j])
                out[i] = (r["pi"][j].reshape(n, n), (a // n, a % n))
                visits[i] = r["N"][j].reshape(n, n)
            if self.solver:
                edges, roots = eng.last_proof()
                proof = [None] * count
                for j, i in enumerate(live):
                    proof[i] = (edges[j].reshape(n, n), int(roots[j]))
                self.last_proof = proof
        self.last_visits = visits
        return out
