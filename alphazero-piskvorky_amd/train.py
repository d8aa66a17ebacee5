#!/usr/bin/env python3
"""The reference's training loop (train.py:39-131) on the GPU path: self-play -> replay buffer -> AdamW steps ->
arena -> promote.  Everything expensive runs in the HIP engine; this file is glue and mirrors the reference's
episode structure so that the drop-in can be exercised end to end:

    python -m alphazero_piskvorky_amd.train --episodes 2 --games 64 --sims 50
"""
import argparse
import os
import tempfile
import time

import numpy as np
import torch

from . import constants as C
from . import parallel
from .controller import NeuralNetworkController, make_batch_policy_value_fn
from .evaluator import ModelEvaluator
from .games import Gomoku
from .net import GomokuNet
from .options import option_from_flags
from .promoter import ModelPromoter
from .replay_buffer import ReplayBuffer
from .self_play import SelfPlayManager

PROMOTION_THRESHOLD = 0.55          # promoter.py:19, strict ">" with draws counted one half


def run(episodes, games, sims, eval_games, device="cuda:0", seed=0, model_dir=None, log=print, device_replay=False,
        subtree_reuse=False, trunk="f32", eval_sims=None, start_positions=None, resign=None, torch_eval=False,
        playout_cap=None, forced_playouts=None, gumbel=None, solver=False, win_rule=None, threat_search=None, selection=None, candidates=None,
        rng=None):
    """eval_sims: simulations per move in the arena (evaluator.py:53-62 takes NUM_EVAL_SIMULATIONS = 200 whatever the
    self-play count is; main() passes that constant); None = as many as self-play, which keeps small test runs short.
    device_replay=True keeps the examples on the GPU from the episode-end gather to the optimizer step (packed records
    in a device ring, batches unpacked + augmented by az_examples_gather) instead of materialising Python tuples.
    start_positions: (boards, players, lasts) the self-play games continue instead of starting on the empty board
    (Engine.set_start_positions); the arena keeps the empty board.
    resign: dict(threshold, min_ply, playout) for the self-play games (Engine.set_resign): a game ends as a loss of the mover
    once a ply's search value falls below -threshold; the share `playout` of the games plays on and gives the false-positive
    rate that every episode's log line reports.  The arena, which decides promotions, plays every game to its end.
    playout_cap: dict(fast_sims, full) for the self-play games (Engine.set_playout_cap): only the share `full` of the plies gets
    `sims` simulations with root noise and becomes examples; the rest is searched with fast_sims simulations.  With
    device_replay the ring receives the engine's filtered export.  The arena and the promoter are untouched.
    forced_playouts: dict(k, prune) for the self-play games (Engine.set_forced_playouts): every noised root guarantees its
    children visits by the square root of their prior, and with prune the policy target leaves those visits out again.  The
    arena is untouched.
    gumbel: dict(m, c_visit, c_scale) for the self-play games (Engine.set_gumbel): every noised root is searched by sequential
    halving over m Gumbel-top candidates and the policy target is softmax(logits + sigma(completed Q)).  Not with
    forced_playouts, subtree_reuse or torch_eval.  The arena is untouched.
    solver=True: MCTS-Solver in the self-play searches (Engine.set_solver): proven wins, losses and draws are kept in the tree,
    the policy target leaves refuted moves out and a proven root records an exact value.  Not with forced_playouts, gumbel,
    subtree_reuse or torch_eval.  The arena is untouched.  Whether it trains a stronger net per GPU hour is not measured.
    threat_search: dict(max_depth, node_budget) for the self-play searches (Engine.set_threat_search): an exact forced-four search
    on every root before the simulations; its proven wins and forced blocks reach the solver as premarked root statuses.  Needs
    solver=True.  The arena is untouched.  Whether it trains a stronger net per GPU hour is not measured.
    selection: dict(fpu, fpu_root, cpuct_base, cpuct_factor) for the self-play searches (Engine.set_selection): an unvisited child is
    worth its parent's value less fpu * sqrt(visited prior mass) instead of 0, and c_puct grows with the parent's count.  Not with
    subtree_reuse, gumbel or solver.  The arena is untouched.  Whether it trains a stronger net per GPU hour is not measured.
    candidates: dict(radius=r) for the self-play searches (Engine.set_candidates): they expand, noise and select only the empty cells
    within Chebyshev distance r of a stone, the priors normalised over them.  Not with subtree_reuse, gumbel, solver, selection or
    torch_eval.  The arena is untouched.  Whether it trains a stronger net per GPU hour is not measured.
    win_rule: "freestyle" (constants.WIN_RULE's default: a run of WIN_LENGTH or more wins) or "exact" (standard Gomoku: exactly
    WIN_LENGTH, overlines win nothing; Engine.set_win_rule).  It is the game itself, so self-play AND the arena play it, and it
    combines with every option.  Whether exact-rule self-play trains a stronger standard-rule net is not measured.
    rng: "numpy" (the default: RandomState streams made on host cores, the reference's numbers) or "philox": self-play's root
    noise and move draws and the arena's move draws come from a counter-based stream made on the GPU (Engine.set_rng), with no
    host tape thread.  Combines with every option.
    torch_eval=True: the searches of self-play and the arena are evaluated by the controllers' own torch modules on the GPU
    (controller.make_batch_policy_value_fn, az_set_external_evaluator) instead of the engine's net kernels -- the loop a
    changed net.py runs on before it has kernels of its own."""
    torch.manual_seed(seed)
    n = C.BOARD_SIZE
    rank, world = parallel.rank_world()
    candidate = NeuralNetworkController(GomokuNet(board_size=n), device=device)
    parallel.broadcast_module_(candidate.net)            # every rank starts from rank 0's initialisation
    model_dir = model_dir or tempfile.mkdtemp(prefix="az_models_")
    # multi-rank: every rank plays its shard of the games; the records go to rank 0 only (the reference has one trainer,
    # train.py:95-104), rank 0 takes the optimizer steps and its weights are broadcast; only rank 0 writes model_dir
    manager = SelfPlayManager(candidate, device, mcts_params={"num_simulations": sims, "c_puct": C.SELF_PLAY_EXPLORATION_CONSTANT},
                              seed=seed, subtree_reuse=subtree_reuse, gather_to=0 if world > 1 else None, trunk=trunk,
                              start_positions=start_positions, resign=resign, playout_cap=playout_cap,
                              forced_playouts=forced_playouts, gumbel=gumbel, solver=solver, win_rule=win_rule, threat_search=threat_search,
                              selection=selection, candidates=candidates, rng=rng, evaluator=make_batch_policy_value_fn(candidate.net, device) if torch_eval else None)
    evaluator = ModelEvaluator(game_class=Gomoku, print_games=False, device=device, seed=seed,
                               evaluators=True if torch_eval else None, win_rule=win_rule, rng=rng)
    promoter = ModelPromoter(model_dir, evaluator, lambda: GomokuNet(board_size=n), device, threshold=PROMOTION_THRESHOLD)
    buffer = ReplayBuffer(capacity=C.BUFFER_CAPACITY)
    ring = None
    history = []
    saved_eval_sims = C.NUM_EVAL_SIMULATIONS
    C.NUM_EVAL_SIMULATIONS = sims if eval_sims is None else eval_sims
    try:
        for ep in range(episodes):
            t0 = time.perf_counter()
            # disjoint seed ranges per episode and per use: game g of the episode's self-play draws from
            # RandomState(base + g), arena game g from RandomState(base + 500_000 + g)
            base = seed + 1_000_003 * ep
            manager.seed = base
            losses = []
            if device_replay:
                from .device_replay import DeviceReplayBuffer
                packed, records, eng, dev, _ = manager.generate_packed(games)
                data = range(records * manager.augmentation)
                if rank == 0:
                    if ring is None:
                        ring = DeviceReplayBuffer(eng, capacity=C.BUFFER_CAPACITY, aug=manager.augmentation, device=dev, seed=seed)
                    ring.extend_packed(packed, records)
                    for _ in range(C.BATCHES_PER_EPISODE):
                        losses.append(candidate.train_tensors(*ring.sample_batch(C.BATCH_SIZE), epochs=C.NUM_EPOCHS))
            else:
                data = manager.generate_self_play(num_games=games, num_workers=C.NUM_WORKERS)   # train.py:89-92
                if rank == 0:
                    buffer.extend(data)                                                          # train.py:95
                    for _ in range(C.BATCHES_PER_EPISODE):                                       # train.py:100-104
                        losses.append(candidate.train(buffer.sample_batch(C.BATCH_SIZE), epochs=C.NUM_EPOCHS))
            parallel.broadcast_module_(candidate.net)          # multi-rank: everybody continues with rank 0's weights
            evaluator.seed = base + 500_000
            win_rate, metrics, promoted = promoter.evaluate_and_maybe_promote(candidate, num_games=eval_games)   # train.py:114-119
            loss = losses[-1].get("loss") if losses else None
            history.append(dict(metrics, episode=ep, examples=len(data), loss=loss,
                                promoted=promoted, seconds=time.perf_counter() - t0))
            rs = manager.last_resign_stats
            if rs is not None:           # this rank's games
                history[-1]["resign"] = rs
                fp = rs["false_positive_rate"]
                log(f"[train] episode {ep}: {rs['resigned']} of {rs['games']} games resigned; {rs['exempt']} played out, "
                    f"{rs['exempt_crossed']} of them crossed the threshold, {rs['false_positives']} of those did not lose: "
                    f"false-positive rate {'n/a' if fp is None else format(fp, '.1%')}")
            ps = manager.last_playout_cap_stats
            if ps is not None and ps["records"]:           # this rank's games
                history[-1]["playout_cap"] = ps
                log(f"[train] episode {ep}: {ps['full_records']} of {ps['records']} plies searched in full "
                    f"({ps['full_records'] / ps['records']:.1%}), {ps['mean_sims_per_ply']:.1f} simulations per ply on average")
            log(f"[train] episode {ep}: {len(data)} examples, loss {'n/a' if loss is None else format(loss, '.4f')}, "
                f"arena {metrics['wins']}/{metrics['losses']}/{metrics['draws']} -> {win_rate:.2%}"
                f"{' (promoted)' if promoted else ''}, {history[-1]['seconds']:.1f}s")
    finally:
        C.NUM_EVAL_SIMULATIONS = saved_eval_sims
    return history


def selection_from_flags(error, fpu, fpu_root, cpuct_base, cpuct_factor):
    """--fpu / --fpu-root / --cpuct-base / --cpuct-factor as the dict the seams take, None when none is given.  --fpu or
    --cpuct-factor switches the option on; the other two without one of them are an error."""
    message = "--fpu-root and --cpuct-base need --fpu or --cpuct-factor"
    flags = {"fpu": fpu, "fpu_root": fpu_root, "cpuct_base": cpuct_base, "cpuct_factor": cpuct_factor}
    if fpu is None and cpuct_factor is not None:
        flags = {"cpuct_factor": flags.pop("cpuct_factor"), **flags}       # the option's own flag goes first
    return option_from_flags(error, flags, message)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=C.NUM_EPISODES)
    ap.add_argument("--games", type=int, default=C.NUM_SELF_PLAY_GAMES)
    ap.add_argument("--sims", type=int, default=C.NUM_SELF_PLAY_SIMULATIONS,
                    help="simulations per move; above 1024 the engines are created deep (az_create_deep, up to 65534), "
                         "and so is the arena's when NUM_EVAL_SIMULATIONS is above 1024")
    ap.add_argument("--eval-games", type=int, default=C.EVALUATION_GAMES)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--trunk", default="f32", choices=["f32", "bf16x3", "f16x2"], help="self-play conv trunk: f32 (bit-exact default) or an fp32-emulating trunk on the 16-bit matrix cores (opt-in: bf16x3, or the faster f16x2 with float16's range)")
    ap.add_argument("--subtree-reuse", action="store_true", help="self-play keeps the chosen child's subtree between plies (opt-in search upgrade)")
    ap.add_argument("--device-replay", action="store_true", help="keep examples on the GPU (packed ring + on-device batch unpacking)")
    ap.add_argument("--start-positions", default=None, metavar="FILE.npz",
                    help="self-play games continue these positions instead of starting on the empty board: arrays boards "
                         "[count, n*n] (0 / 1 X / 2 O), players [count] (1 / 2), lasts [count] (-1 none); game g takes position g mod count")
    ap.add_argument("--resign-threshold", type=float, default=None, metavar="T",
                    help="self-play games resign: a game ends as a loss of the mover once a ply's search value is below -T (0 < T <= 1)")
    ap.add_argument("--resign-min-ply", type=int, default=0, help="no resignation before this ply")
    ap.add_argument("--resign-playout", type=float, default=None, metavar="SHARE",
                    help="share of the games that play on past the threshold, to measure its false-positive rate "
                         "(default 0.1 when --resign-threshold is given)")
    ap.add_argument("--playout-cap-fast", type=int, default=None, metavar="F",
                    help="playout cap randomisation: self-play plies outside the full share are searched with F simulations "
                         "and no root noise, and give no examples")
    ap.add_argument("--playout-cap-full", type=float, default=None, metavar="P",
                    help="share of the self-play plies that get the full search (default 0.25 when --playout-cap-fast is given)")
    ap.add_argument("--forced-playouts", type=float, default=None, metavar="K",
                    help="forced playouts at the noised roots of self-play: a root child is searched while its visits squared "
                         "are below K x prior x simulations so far (0 < K <= 16; KataGo uses 2), and the policy target is pruned")
    ap.add_argument("--no-target-pruning", action="store_true",
                    help="with --forced-playouts: keep the forced visits in the policy target")
    ap.add_argument("--gumbel", type=int, default=None, metavar="M",
                    help="Gumbel root search at the noised roots of self-play: M Gumbel-top candidates searched by sequential "
                         "halving, policy target from the completed Q values (1 <= M <= 64; the paper uses 16)")
    ap.add_argument("--gumbel-c-visit", type=float, default=None, metavar="X", help="with --gumbel: c_visit of sigma (default 50)")
    ap.add_argument("--gumbel-c-scale", type=float, default=None, metavar="Y", help="with --gumbel: c_scale of sigma (default 1)")
    ap.add_argument("--solver", action="store_true",
                    help="MCTS-Solver in the self-play searches: proven wins, losses and draws are kept in the tree, the policy "
                         "target leaves refuted moves out and a proven root records an exact value")
    ap.add_argument("--threat-depth", type=int, default=None, metavar="D",
                    help="root threat search in the self-play searches: an exact forced-four search of depth D (1..16) on every root "
                         "before the simulations, handed to the solver; implies --solver")
    ap.add_argument("--threat-nodes", type=int, default=None, metavar="N", help="with --threat-depth: fours tried per root at most (default 256)")
    ap.add_argument("--fpu", type=float, default=None, metavar="R",
                    help="selection rule in the self-play searches: an unvisited child is worth its parent's value less "
                         "R x sqrt(prior mass already visited) instead of 0 (0 <= R <= 2; Leela Zero and KataGo use about 0.2)")
    ap.add_argument("--fpu-root", type=float, default=None, metavar="R0", help="with --fpu or --cpuct-factor: the reduction at the root (default 0)")
    ap.add_argument("--cpuct-base", type=float, default=None, metavar="B", help="with --fpu or --cpuct-factor: c_base of the c_puct growth (default 19652)")
    ap.add_argument("--cpuct-factor", type=float, default=None, metavar="F",
                    help="selection rule in the self-play searches: c_puct + F x log((N + B + 1) / B) at a parent with N visits "
                         "(0 <= F <= 16; AlphaZero's rule is F = 1); unvisited children are scored as under --fpu (default R 0.2)")
    ap.add_argument("--candidate-radius", type=int, default=None, metavar="R",
                    help="candidate moves in the self-play searches: only the empty cells within Chebyshev distance R (1 .. n-1) of a "
                         "stone are expanded, noised and selected, and the priors are normalised over them")
    ap.add_argument("--win-rule", choices=("freestyle", "exact"), default=None,
                    help="the game that self-play and the arena play: freestyle (default; a run of WIN_LENGTH or more wins) or "
                         "exact (standard Gomoku: exactly WIN_LENGTH, an overline wins nothing)")
    ap.add_argument("--rng", choices=("numpy", "philox"), default=None,
                    help="where the engine's random numbers come from: numpy (default; RandomState streams made on host cores, the "
                         "reference's numbers) or philox (a counter-based stream made on the GPU, no host tape threads)")
    ap.add_argument("--torch-eval", action="store_true",
                    help="evaluate the searches with the controller's own torch module as a batched external evaluator "
                         "(any net; no HIP trunk needed) instead of the engine's net kernels")
    a = ap.parse_args()
    resign = None
    if a.resign_threshold is not None:
        resign = {"threshold": a.resign_threshold, "min_ply": a.resign_min_ply,
                  "playout": 0.1 if a.resign_playout is None else a.resign_playout}
    elif a.resign_playout is not None or a.resign_min_ply:
        ap.error("--resign-min-ply and --resign-playout need --resign-threshold")
    playout_cap = None
    if a.playout_cap_fast is not None:
        playout_cap = {"fast_sims": a.playout_cap_fast, "full": 0.25 if a.playout_cap_full is None else a.playout_cap_full}
    elif a.playout_cap_full is not None:
        ap.error("--playout-cap-full needs --playout-cap-fast")
    forced_playouts = None
    if a.forced_playouts is not None:
        forced_playouts = {"k": a.forced_playouts, "prune": not a.no_target_pruning}
    elif a.no_target_pruning:
        ap.error("--no-target-pruning needs --forced-playouts")
    gumbel = option_from_flags(ap.error, {"m": a.gumbel, "c_visit": a.gumbel_c_visit, "c_scale": a.gumbel_c_scale},
                               "--gumbel-c-visit and --gumbel-c-scale need --gumbel")
    threat_search = option_from_flags(ap.error, {"max_depth": a.threat_depth, "node_budget": a.threat_nodes},
                                      "--threat-nodes needs --threat-depth")
    if threat_search is not None:
        a.solver = True
    selection = selection_from_flags(ap.error, a.fpu, a.fpu_root, a.cpuct_base, a.cpuct_factor)
    candidates = None if a.candidate_radius is None else {"radius": a.candidate_radius}
    start_positions = None
    if a.start_positions:
        with np.load(a.start_positions) as z:
            start_positions = (z["boards"], z["players"], z["lasts"])
    # one process per GPU under torch.distributed.run: games and arena games are sharded over the ranks (self_play.py,
    # evaluator.py), the examples are gathered to rank 0, which trains, writes the checkpoints and broadcasts the weights
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as td
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        td.init_process_group("nccl", device_id=torch.device("cuda", local))
        a.device = f"cuda:{local}"
    run(a.episodes, a.games, a.sims, a.eval_games, a.device, model_dir=a.model_dir, device_replay=a.device_replay,
        subtree_reuse=a.subtree_reuse, trunk=a.trunk, eval_sims=C.NUM_EVAL_SIMULATIONS, start_positions=start_positions,
        resign=resign, torch_eval=a.torch_eval, playout_cap=playout_cap, forced_playouts=forced_playouts,
        gumbel=gumbel, solver=a.solver, win_rule=a.win_rule, threat_search=threat_search, selection=selection,
        candidates=candidates, rng=a.rng)
    if world > 1:
        td.barrier()
        td.destroy_process_group()


if __name__ == "__main__":
    main()
