"""SelfPlayManager seam (self_play.py:24-159): the whole episode runs in the HIP engine, one engine per GPU,
games sharded over the ranks of torch.distributed when it is initialised, records exchanged once at episode end."""
from collections.abc import Callable

import numpy as np
import torch

from . import constants as _c
from . import parallel
from ._capi import check_candidates, check_rng, check_selection, check_threat_search, AZ_AUG_REFERENCE4, AZ_MAX_SIMULATIONS, REUSE_MAX_SIMULATIONS, Engine, playout_cap_permille, resign_permille, win_rule_name
from .controller import BatchPolicyValueFn, device_index, model_kind
from .mcts import check_forced_playouts, check_gumbel, check_solver, numpy_log_table
from .options import apply_options, bring_candidates, bring_selection, check_combination, switched_on


def default_temperature_schedule(move: int) -> float:
    norm = 1 + _c.TEMPERATURE_BASELINE
    return (np.exp(-move / _c.TEMPERATURE_SCHEDULE_HALFTIME) + _c.TEMPERATURE_BASELINE) / norm


def resign_stats(result, cross_ply, exempt, movers) -> dict:
    """What an episode says about its resignation threshold, per game: result (AZ_RES_*, 0 = cut), cross_ply (first ply
    whose search value crossed, -1 = none), exempt (the game was played out whatever its values) and movers (the side to
    move at cross_ply, 1 / 2; ignored where cross_ply < 0).
      resigned                games that ended by resignation: crossed, not exempt, lost by the side that crossed (a move
                              that ends the game itself takes precedence, and then the mover has won or drawn)
      exempt                  games that were played out
      exempt_crossed          ... of which some ply crossed: they would have resigned
      false_positives         ... of which the side that crossed did NOT lose in the end
      false_positive_rate     false_positives / exempt_crossed, None without an exempt game that crossed"""
    result, cross_ply = np.asarray(result, np.int64), np.asarray(cross_ply, np.int64)
    exempt, movers = np.asarray(exempt, bool), np.asarray(movers, np.int64)
    if not (result.shape == cross_ply.shape == exempt.shape == movers.shape and result.ndim == 1):
        raise ValueError("result, cross_ply, exempt and movers must be one-dimensional and of one length")
    crossed = cross_ply >= 0
    if not np.isin(movers[crossed], (1, 2)).all():
        raise ValueError("movers must be 1 or 2 wherever a ply crossed")
    lost = crossed & (result == 3 - movers)
    ec = crossed & exempt
    fp = int((ec & ~lost).sum())
    return {"games": int(len(result)), "resigned": int((lost & ~exempt).sum()), "exempt": int(exempt.sum()),
            "exempt_crossed": int(ec.sum()), "false_positives": fp,
            "false_positive_rate": fp / int(ec.sum()) if ec.any() else None}


def check_resign(resign):
    """None, or the dict a seam takes: threshold in (0, 1], optional min_ply >= 0 and playout share in [0, 1]."""
    if resign is None:
        return None
    extra = set(resign) - {"threshold", "min_ply", "playout"}
    if extra or "threshold" not in resign:
        raise ValueError(f"resign takes threshold, min_ply and playout (threshold is required), got {sorted(resign)}")
    out = {"threshold": float(resign["threshold"]), "min_ply": int(resign.get("min_ply", 0)),
           "playout": float(resign.get("playout", 0.0))}
    if not 0.0 < out["threshold"] <= 1.0:
        raise ValueError(f"resign threshold must be in (0, 1], got {out['threshold']}")
    if out["min_ply"] < 0:
        raise ValueError(f"resign min_ply must be >= 0, got {out['min_ply']}")
    resign_permille(out["playout"])
    return out


def check_playout_cap(cap, num_simulations=None):
    """None, or the dict a seam takes: fast_sims >= 1 (at most num_simulations when that is given), optional share `full` of
    the plies that get the full search (default 0.25) and train_on_fast (default False: only full plies become examples)."""
    if cap is None:
        return None
    extra = set(cap) - {"fast_sims", "full", "train_on_fast"}
    if extra or "fast_sims" not in cap:
        raise ValueError(f"playout_cap takes fast_sims, full and train_on_fast (fast_sims is required), got {sorted(cap)}")
    out = {"fast_sims": int(cap["fast_sims"]), "full": float(cap.get("full", 0.25)),
           "train_on_fast": bool(cap.get("train_on_fast", False))}
    if out["fast_sims"] < 1 or (num_simulations is not None and out["fast_sims"] > num_simulations):
        raise ValueError(f"playout_cap fast_sims must be 1..num_simulations"
                         f"{'' if num_simulations is None else f' = {num_simulations}'}, got {out['fast_sims']}")
    playout_cap_permille(out["full"])
    return out


def _mix32(x):
    """murmur3's 32-bit finaliser on a uint32 array (az_resign_mix)"""
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B); x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35); x ^= x >> np.uint32(16)
    return x


def playout_cap_full_plies(seed0, nply, ply0, full) -> np.ndarray:
    """bool per record, game-major then ply like Engine.records(): the ply was FULL by the rule of az_set_playout_cap
    (az_playout_cap_full, restated on arrays).  seed0: seed of the first game; nply[g]: plies game g searched; ply0[g]: the
    absolute ply it started at (0 from the empty board); full: the share of full plies."""
    nply, ply0 = np.asarray(nply, np.int64), np.broadcast_to(np.asarray(ply0, np.int64), np.shape(nply))
    game = np.repeat(np.arange(len(nply), dtype=np.int64), nply)
    ply = np.arange(int(nply.sum()), dtype=np.int64) - np.repeat(np.cumsum(nply) - nply, nply) + ply0[game]
    key = ((int(seed0) + game) & 0xFFFFFFFF).astype(np.uint32)
    inner = _mix32(((ply + 0x9E3779B9) & 0xFFFFFFFF).astype(np.uint32))
    return (_mix32(key ^ inner) % np.uint32(1000)).astype(np.int64) < playout_cap_permille(full)


def playout_cap_stats(sims, full) -> dict:
    """What an episode says about its playout cap: sims, the simulations of every record (Engine.sims()), and full, whether the
    record's ply was FULL by the hash (playout_cap_full_plies; with fast_sims = num_simulations the simulations cannot tell).
    The records, those of full plies -- what the export filter lets through --, and the mean simulations per ply (the cost of
    the episode's searches, num_simulations without a cap)."""
    sims, full = np.asarray(sims, np.int64), np.asarray(full, bool)
    if sims.shape != full.shape or sims.ndim != 1:
        raise ValueError("sims and full must be one-dimensional and of one length")
    return {"records": int(len(sims)), "full_records": int(full.sum()),
            "mean_sims_per_ply": float(sims.mean()) if len(sims) else None}


class SelfPlayManager:
    def __init__(self, controller, device, mcts_params: dict = None,
                 temperature_schedule: Callable[[int], float] = default_temperature_schedule,
                 concurrent_games: int = None, augmentation: int = AZ_AUG_REFERENCE4, seed: int = None,
                 engines_per_gpu: int = None, subtree_reuse: bool = False, gather_to: int = None,
                 eval_cache: int = 0, virtual_loss: int = 1, trunk: str = "f32", leaf_symmetry: bool = False,
                 start_positions=None, resign: dict = None, evaluator: BatchPolicyValueFn = None,
                 playout_cap: dict = None, forced_playouts: dict = None, gumbel: dict = None, solver: bool = False,
                 win_rule: str = None, threat_search: dict = None, selection: dict = None, candidates: dict = None,
                 rng: str = None):
        self.controller = controller
        # where the engine's random numbers come from: "numpy" (the default; RandomState(seed + game) streams made on host cores,
        # the reference's numbers) or "philox" (a counter-based stream made on the GPU with no host thread: throughput runs;
        # az_set_rng).  Combines with every option.
        self.rng = rng
        # which game is played: "freestyle" (constants.WIN_RULE's default, the reference's: a run of WIN_LENGTH or more wins) or
        # "exact" (standard Gomoku: exactly WIN_LENGTH, an overline wins nothing; az_set_win_rule).  Combines with every option.
        # Whether exact-rule self-play trains a stronger standard-rule net has not been measured.
        self.win_rule = win_rule_name(_c.WIN_RULE if win_rule is None else win_rule)
        # opt-in: a controller.BatchPolicyValueFn evaluates every leaf instead of the engine's own net kernels (any torch
        # net on the same GPU; az_set_external_evaluator).  Not with subtree_reuse or leaf_symmetry; eval_cache and trunk
        # have no effect while it is set.
        if evaluator is not None and not isinstance(evaluator, BatchPolicyValueFn):
            raise TypeError("evaluator must be a controller.BatchPolicyValueFn (make_batch_policy_value_fn)")
        self.evaluator = evaluator
        self.device = device
        self.mcts_params = mcts_params or {"num_simulations": 100}
        # opt-in playout cap randomisation: dict(fast_sims, full=0.25, train_on_fast=False); only the share `full` of the plies
        # gets num_simulations and root noise and becomes training examples, the rest is searched with fast_sims and moves
        # the game along (az_set_playout_cap).  Not with subtree_reuse or an external evaluator.
        self.playout_cap = playout_cap
        self.last_playout_cap_stats = None    # playout_cap_stats() of this rank's games of the last episode (None while the cap is off)
        # opt-in forced playouts and policy target pruning: dict(k, prune=True); every noised root (with a playout cap: the full
        # plies') guarantees its children visits by the square root of their prior, and pi is made from the counts without
        # them (az_set_forced_playouts).  Not with subtree_reuse.  The records keep the raw visits and neither W nor the
        # priors, so the pruned share cannot be recomputed from them: the manager reports no statistics of it
        # (tools/forced_playouts_gain.py measures it on searched positions).
        self.forced_playouts = forced_playouts
        # opt-in Gumbel root search: dict(m=16, c_visit=50.0, c_scale=1.0); every noised root (with a playout cap: the full plies')
        # samples m Gumbel-top candidates, searches them by sequential halving and records pi = softmax(logits + sigma(completed
        # Q)) (az_set_gumbel); the engine fills the game tapes with Gumbel draws.  Not with subtree_reuse, virtual_loss > 1,
        # forced_playouts or an external evaluator.
        self.gumbel = gumbel
        # opt-in MCTS-Solver: every search keeps proven wins, losses and draws in its tree; pi never spreads mass over refuted
        # moves while a better one is known, a proven root records an exact value (az_set_solver).  Not with subtree_reuse,
        # virtual_loss > 1, forced_playouts, gumbel or an external evaluator.  Whether it trains a stronger net per GPU hour
        # has not been measured.
        self.solver = solver
        # opt-in root threat search, dict(max_depth=8, node_budget=256) or True: an exact forced-four search on every root before
        # the simulations, its proven wins and forced blocks premarked for the solver (az_set_threat_search).  Needs solver=True.
        # Whether it trains a stronger net per GPU hour has not been measured.
        self.threat_search = threat_search
        # opt-in selection rule: dict(fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0); an unvisited child is worth its
        # parent's value less fpu * sqrt(visited prior mass) instead of 0, and c_puct grows with the parent's count
        # (az_set_selection).  Not with subtree_reuse, gumbel or solver.  Whether it trains a stronger net per GPU hour has not
        # been measured (tools/selection_gain.py measures throughput, game length and how wide the roots get).
        self.selection = selection
        # opt-in candidate moves: dict(radius=r); every search expands, noises and selects only the empty cells within Chebyshev
        # distance r of a stone (every cell on an empty board), the priors normalised over them (az_set_candidates).  Not with
        # subtree_reuse, gumbel, solver, selection or an outside evaluator.  Whether it trains a stronger net per GPU hour has not
        # been measured (tools/candidates_gain.py measures throughput and the shape of the searches).
        self.candidates = candidates
        self.temperature_schedule = temperature_schedule
        self.concurrent_games = concurrent_games or _c.CONCURRENT_GAMES
        self.augmentation = augmentation      # 4 = the reference's rotations (self_play.py:94-108), 8 = full dihedral group, 1 = none
        self.seed = seed
        self.engines_per_gpu = engines_per_gpu      # None: az_config.engines = 0, the library chooses
        self.subtree_reuse = subtree_reuse    # opt-in search upgrade (mcts.py:17-22 TODO); off = the reference's fresh root every move
        self.eval_cache = eval_cache          # opt-in: positions kept in the device evaluation cache (mcts.py:17,22 TODO); results unchanged
        self.virtual_loss = virtual_loss      # opt-in: leaves per search and evaluation batch (mcts.py:17-22 TODO); 1 = sequential like the reference
        self.trunk = trunk                    # opt-in: "bf16x3" / "f16x2" = fp32-emulating conv trunks on the 16-bit matrix cores (tolerance, not bit-exact)
        self.leaf_symmetry = leaf_symmetry    # opt-in: every net evaluation sees a pseudo-random dihedral symmetry of the position (README.md:61,82)
        self.start_positions = start_positions    # opt-in: (boards, players, lasts); game g continues position g mod count instead of starting on the empty board
        # opt-in: dict(threshold, min_ply=0, playout=0.0); a game ends as a loss of the mover once the search value of a ply
        # falls below -threshold, except in the share `playout` of the games, which measure the false positives
        self.resign = resign
        self.last_resign_stats = None         # resign_stats() of this rank's games of the last episode (None while resignation is off)
        self.gather_to = gather_to            # multi-rank: None = every rank receives all records (all-gather); r = only rank r does
        self.last_counters = None
        self._engine = None
        self._check_options()

    def _check_options(self):
        """Every option in its checked form, and ValueError for a bad value or a combination the engine would refuse: at
        construction, and again before every episode (the options are plain attributes)."""
        self.win_rule = win_rule_name(self.win_rule)
        self.resign = check_resign(self.resign)
        self.playout_cap = check_playout_cap(self.playout_cap, self.mcts_params.get("num_simulations", 100))
        self.forced_playouts = check_forced_playouts(self.forced_playouts)
        self.gumbel = check_gumbel(self.gumbel)
        self.solver = check_solver(self.solver)
        self.threat_search = check_threat_search(self.threat_search)
        self.selection = check_selection(self.selection)
        self.candidates = check_candidates(self.candidates)
        self.rng = check_rng(self.rng)
        check_combination(switched_on(subtree_reuse=self.subtree_reuse, virtual_loss=self.virtual_loss, leaf_symmetry=self.leaf_symmetry,
                                      evaluator=self.evaluator, playout_cap=self.playout_cap, forced_playouts=self.forced_playouts,
                                      gumbel=self.gumbel, solver=self.solver, threat_search=self.threat_search, selection=self.selection,
                                      candidates=self.candidates))

    def _eng(self, n, k, slots):
        p = self.mcts_params
        key = (n, k, p.get("num_simulations", 100), slots, p.get("c_puct", _c.SELF_PLAY_EXPLORATION_CONSTANT),
               p.get("dirichlet_alpha", 0.3), p.get("dirichlet_weight", 0.25), model_kind(self.controller.net),
               self.virtual_loss, self.eval_cache, self.leaf_symmetry)
        if self._engine is None or self._engine_key != key:
            if self._engine is not None:
                self._engine.close()
            # lanes per GPU: the library's own rule (1 on small boards, one per 128 slots up to 4) unless the caller fixed it
            self._engine = Engine(n, k, key[2], slots, engines=self.engines_per_gpu or 0, c_puct=key[4], dirichlet_alpha=key[5],
                                  dirichlet_weight=key[6], device=device_index(self.device),
                                  log_table=numpy_log_table(key[2]), model=key[7], deep=key[2] > AZ_MAX_SIMULATIONS)
            self._engine.set_virtual_loss(self.virtual_loss)
            self._engine.set_eval_cache(self.eval_cache)
            self._engine.set_leaf_symmetry(self.leaf_symmetry)
            if self.evaluator is not None:
                self.evaluator.attach(self._engine)
            self._engine_key = key
        return self._engine

    def generate_self_play(self, num_games: int, num_workers: int = None, flatten=False) -> list:
        """Returns list[(state f32 (4,n,n) CPU tensor, pi f32 (n,n) ndarray, z int)] in (game, ply, k) order
        (self_play.py:110-159; num_workers / flatten are accepted and unused like the reference's `flatten`).  With a playout
        cap: the examples of the full plies only, unless the cap says train_on_fast."""
        packed, total, eng, dev, n = self.generate_packed(num_games)
        aug = self.augmentation
        states = torch.empty((total * aug, 4, n, n), dtype=torch.float32, device=dev)
        pis = torch.empty((total * aug, n, n), dtype=torch.float32, device=dev)
        zs = torch.empty(total * aug, dtype=torch.float32, device=dev)
        if total:
            eng.examples_from_packed(packed.data_ptr(), total, aug, states.data_ptr(), pis.data_ptr(), zs.data_ptr())
        states, pis, zs = states.cpu(), pis.cpu().numpy(), zs.cpu().numpy().astype(np.int64)
        print(f"[SelfPlayManager] Collected {len(zs)} examples from {num_games} games.")
        return list(zip(states.unbind(0), list(pis), zs.tolist()))     # (tensor view, ndarray view, int) per example

    def _resign_stats(self, eng, lo, mine):
        """resign_stats of the games this rank has just played (ids lo .. lo + mine); X moves first from the empty board,
        a start position names its own side to move"""
        _, result = eng.games()
        cross, exempt = eng.resign_info()
        first, ply0 = np.ones(mine, np.int64), np.zeros(mine, np.int64)
        if self.start_positions is not None:
            boards, players, _ = self.start_positions
            boards = np.asarray(boards).reshape(len(players), -1)
            idx = (lo + np.arange(mine)) % len(players)
            first, ply0 = np.asarray(players, np.int64)[idx], (boards != 0).sum(axis=1)[idx]
        movers = np.where((cross - ply0) % 2 == 0, first, 3 - first)
        return resign_stats(result, cross, exempt, movers)

    def generate_packed(self, num_games: int):
        """The same episode, but the result stays on the device as packed records (one per position, all ranks'
        records after the exchange): (uint8 tensor, record count, engine, device, n).  Feed it to
        device_replay.DeviceReplayBuffer.extend_packed to train without materialising Python tuples.
        Games are always played to the end here (max_plies is never passed), so no record carries the label of a cut
        game, z = 99 (include/az_engine.h), which the example kernels would hand on as a value target."""
        self._check_options()
        n = self.controller.net.board_size
        k = min(_c.WIN_LENGTH, n)
        rank, world = parallel.rank_world()
        per = (num_games + world - 1) // world
        lo, hi = min(rank * per, num_games), min((rank + 1) * per, num_games)
        mine = hi - lo
        seed0 = self.seed if self.seed is not None else int(np.random.randint(0, 2 ** 31 - 1))
        if self.seed is None:
            seed0 = parallel.broadcast_seed(seed0, torch.device("cuda", device_index(self.device)))
        dev = torch.device("cuda", device_index(self.device))
        sims = self.mcts_params.get("num_simulations", 100)
        if self.subtree_reuse and sims > REUSE_MAX_SIMULATIONS:
            raise ValueError(f"subtree_reuse supports at most {REUSE_MAX_SIMULATIONS} simulations per move (got {sims}): "
                             "the retained tree is renumbered in a 1024-row table")
        eng = self._eng(n, k, max(1, min(self.concurrent_games, max(mine, 1))))
        if self.evaluator is None:
            eng.load_weights(self.controller.net.state_dict(), 0)
        bring_candidates(eng, self.candidates, before=True)    # before the selection rule or any other refused partner may come on
        bring_selection(eng, self.selection, before=True)      # before subtree reuse, the solver or the Gumbel root may come on
        eng.set_subtree_reuse(self.subtree_reuse)
        if eng.trunk_mode() != self.trunk:
            eng.set_trunk_mode(self.trunk)
        T = np.array([float(self.temperature_schedule(m)) for m in range(n * n + 1)], dtype=np.float64)
        apply_options(eng, win_rule=self.win_rule, start_positions=self.start_positions, first=lo, resign=self.resign,
                      playout_cap=self.playout_cap, forced_playouts=self.forced_playouts, gumbel=self.gumbel, solver=self.solver,
                      threat_search=self.threat_search, rng=self.rng)
        bring_selection(eng, self.selection, before=False)
        bring_candidates(eng, self.candidates, before=False)
        self.last_resign_stats = self.last_playout_cap_stats = None
        if mine > 0:
            self.last_counters = eng.selfplay(mine, seed0=seed0 + lo, temperature_table=T)
            if self.resign is not None:
                self.last_resign_stats = self._resign_stats(eng, lo, mine)
            if self.playout_cap is not None:
                ply0 = 0
                if self.start_positions is not None:
                    boards, players, _ = self.start_positions
                    ply0 = (np.asarray(boards).reshape(len(players), -1) != 0).sum(axis=1)[(lo + np.arange(mine)) % len(players)]
                full = playout_cap_full_plies(seed0 + lo, eng.games()[0], ply0, self.playout_cap["full"])
                self.last_playout_cap_stats = playout_cap_stats(eng.sims(), full)
        else:
            eng.clear_episode()       # no games for this rank: it must not send the engine's previous episode again
        packed, counts = parallel.gather_packed_records(eng, dev, dst=self.gather_to)
        total = int(sum(counts)) if (self.gather_to is None or rank == self.gather_to) else 0
        return packed, total, eng, dev, n
