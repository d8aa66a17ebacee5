#!/usr/bin/env python3
"""Searches per second with a torch module as the evaluator: the batched external evaluator (az_set_external_evaluator)
against the one-leaf-per-round-trip loop of az_search_callback, on one GPU, from the repo root:

    python tools/external_eval_gain.py --parent-lib PATH/libaz_engine.so [--out profiles/external_eval.json]

The evaluator of every leg but `native` is the torch GomokuNet (synthetic weights) on the engine's GPU.  Legs per
configuration, each in a fresh process of its own under `timeout -k 10`; the first non-zero status ends the run (what was
measured before it is still written):
  callback_parent  MCTS(plain callable).run over a SAMPLE of 16 positions on a library built from the PARENT commit
                   (--parent-lib, loaded through the AZ_ENGINE_LIB switch): one position at a time, one leaf per host round
                   trip.  searches/s = 16 / seconds; the baseline of every speed-up
  ext_L1           MCTS(make_batch_policy_value_fn(net)).run_many over ALL positions: one request per simulation
  ext_L8           the same with virtual-loss batching, 8 leaves per game and request
  native           MCTS(make_policy_value_fn(controller)).run_many, the engine's own net kernels: for orientation
Every leg makes one warm-up call and takes the median of 3 timed runs.
Configurations: 15x15 / 5, S = 150, 1024 positions; 5x5 / 4, S = 100, 4096 positions.  Positions: random undecided ones by
legal play from a fixed RandomState, noise on."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "15x15": dict(n=15, k=5, S=150, positions=1024),
    "5x5": dict(n=5, k=4, S=100, positions=4096),
}
LEGS = ("callback_parent", "ext_L1", "ext_L8", "native")
SAMPLE = 16


def _states(n, k, count, seed):
    """undecided positions: X and O in turn on the cells of a random permutation, kept when nobody has a line anywhere"""
    import numpy as np
    from alphazero_piskvorky_amd import games
    rs = np.random.RandomState(seed)
    nn = n * n
    out = []
    while len(out) < count:
        stones = int(rs.randint(0, nn // 2))
        where = rs.permutation(nn)[:stones]
        s = games.Gomoku(n, k)
        s.cells[where] = 1 + (np.arange(stones) & 1)
        s.current_player = "X" if stones % 2 == 0 else "O"
        s.last_action = None if stones == 0 else (int(where[-1]) // n, int(where[-1]) % n)
        if not s.is_terminal():
            out.append(s)
    return out


def run_leg(config, leg):
    import numpy as np
    import torch
    from alphazero_piskvorky_amd.controller import NeuralNetworkController, make_batch_policy_value_fn, make_policy_value_fn
    from alphazero_piskvorky_amd.mcts import MCTS
    from alphazero_piskvorky_amd.net import GomokuNet
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c = CONFIGS[config]
    n, k, S, P = c["n"], c["k"], c["S"], c["positions"]
    m = GomokuNet(board_size=n)
    m.load_state_dict({key: torch.as_tensor(v) for key, v in synthetic_state_dict(n).items()})
    ctrl = NeuralNetworkController(m.eval(), device="cuda:0")
    states = _states(n, k, P, 2024)
    if leg == "callback_parent":
        states = states[:SAMPLE]

        def plain(state):              # controller.py:39-53, the reference's evaluator for one state
            with torch.no_grad():
                logits, value = ctrl.net(state.encode("cuda:0").unsqueeze(0))
                return torch.softmax(logits[0], dim=0).cpu().numpy().reshape(n, n), float(value.item())

        mcts = MCTS(plain, num_simulations=S, c_puct=2.0)
        once = lambda: [mcts.run(s, 1.0, add_root_noise=True) for s in states]
    elif leg == "native":
        mcts = MCTS(make_policy_value_fn(ctrl), num_simulations=S, c_puct=2.0)
        once = lambda: mcts.run_many(states, 1.0, add_root_noise=True)
    else:
        bf = make_batch_policy_value_fn(ctrl.net)
        inner, seen, t_leg = bf.fn, [0], time.perf_counter()

        def counted(planes, net):      # progress in the log: a slow evaluator and a stuck one look different there
            seen[0] += 1
            if seen[0] <= 3 or seen[0] % 100 == 0:
                print(f"  request {seen[0]}: {planes.shape[0]} items, {time.perf_counter() - t_leg:.2f} s into the leg", flush=True)
            return inner(planes, net)

        bf.fn = counted
        mcts = MCTS(bf, num_simulations=S, c_puct=2.0, virtual_loss=8 if leg == "ext_L8" else 1)
        once = lambda: mcts.run_many(states, 1.0, add_root_noise=True)
    np.random.seed(1)
    once()                             # warm-up: kernels loaded, buffers allocated, torch's convolutions chosen
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        out = once()
        runs.append(time.perf_counter() - t)
        assert len(out) == len(states) and all(a is not None for _, a in out)
    row = {"config": config, "leg": leg, "library": "parent commit" if leg == "callback_parent" else "this build",
           "board": n, "simulations": S, "positions": len(states), "runs_seconds": runs,
           "searches_per_sec": len(states) / statistics.median(runs), "ms_per_search": statistics.median(runs) * 1e3 / len(states)}
    eng = mcts._batch_engine
    if leg.startswith("ext") and eng is not None:
        row["ext_stats_last_call"] = eng.ext_stats()
        row["slots"], row["lanes"] = eng.slots, eng.lanes()
    print(row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "external_eval.json"))
    ap.add_argument("--parent-lib", help="libaz_engine.so built from the parent commit (leg callback_parent); without it that leg runs on this build")
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.leg:
        row = run_leg(a.config, a.leg)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    result = {"configs": CONFIGS, "sample_of_the_callback_loop": SAMPLE, "rows": []}
    rc = 0
    for config in ("15x15", "5x5"):
        for leg in LEGS:
            part = a.out + f".{config}.{leg}.part"
            env = dict(os.environ)
            env.pop("AZ_ENGINE_LIB", None)
            if leg == "callback_parent" and a.parent_lib:
                env["AZ_ENGINE_LIB"] = os.path.abspath(a.parent_lib)
            rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
                                 "--leg", leg, "--config", config, "--out", part], cwd=ROOT, env=env).returncode
            if rc != 0:
                print(f"{config} / {leg} failed ({rc}); stopping", flush=True)
                result["failed"] = {"config": config, "leg": leg, "returncode": rc}
                break
            with open(part) as f:
                row = json.load(f)
            if leg == "callback_parent" and not a.parent_lib:
                row["library"] = "this build"
            result["rows"].append(row)
            os.remove(part)
        if rc != 0:
            break
    by = {(r["config"], r["leg"]): r["searches_per_sec"] for r in result["rows"]}
    result["speedup_over_parent_callback_loop"] = {f"{c}/{leg}": by[(c, leg)] / by[(c, "callback_parent")] for c in CONFIGS
                                                   for leg in ("ext_L1", "ext_L8", "native") if (c, leg) in by and (c, "callback_parent") in by}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
