#!/usr/bin/env python3
"""Searches per second of a list of given positions: a loop of Engine.search against Engine.search_batch, on one GPU, from
the repo root:

    python tools/search_batch_timing.py --parent-lib PATH/libaz_engine.so [--out profiles/search_batch.json]

Three legs per configuration, each in a fresh process of its own under `timeout -k 10`; the first non-zero status ends the
run (what was measured before it is still written):
  (a) loop_parent  a loop of Engine.search on a library built from the PARENT commit (--parent-lib, loaded through the
                   AZ_ENGINE_LIB switch): the baseline of every speed-up
  (b) loop         the same loop on this build: what the wider DevState costs the single search
  (c) batch        Engine.search_batch on this build
Every leg makes one warm-up call and takes the median of 3 timed runs over all positions.  The loops use a one-slot engine,
as MCTS.run does (the configuration of the single-search latency figure); the batch uses `slots` slots.
Configurations: 15x15 / 5, S = 150, 1024 slots, 1024 positions; 5x5 / 4, S = 100, 1024 slots, 4096 positions (persistent
search kernel).  Positions: random undecided ones by legal play from a fixed RandomState, noise on, per-position temperature."""
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
    "15x15": dict(n=15, k=5, S=150, slots=1024, positions=1024),
    "5x5": dict(n=5, k=4, S=100, slots=1024, positions=4096),
}
LEGS = ("loop_parent", "loop", "batch")


def _positions(n, k, count, seed):
    """undecided positions: X and O in turn on the cells of a random permutation (X first), kept when nobody has a line
    anywhere and a cell is free.  games.Gomoku.is_terminal scans every stone of the board in all four directions, not only
    the last action, so a line made on the way and played past is caught too."""
    import numpy as np
    from alphazero_piskvorky_amd import games
    rs = np.random.RandomState(seed)
    nn = n * n
    boards, players, lasts = [], [], []
    while len(boards) < count:
        stones = int(rs.randint(0, nn // 2))
        where = rs.permutation(nn)[:stones]
        s = games.Gomoku(n, k)
        s.cells[where] = 1 + (np.arange(stones) & 1)          # X and O in turn, X first
        s.current_player = "X" if stones % 2 == 0 else "O"
        s.last_action = None if stones == 0 else (int(where[-1]) // n, int(where[-1]) % n)
        if s.is_terminal():                                     # whole-board scan
            continue
        boards.append(np.asarray(s.cells, np.uint8).copy()); players.append(s.player_code()); lasts.append(s.last_index())
    noise = [rs.dirichlet([0.3] * int((b == 0).sum())) for b in boards]
    us = rs.random_sample(count)
    Ts = rs.uniform(0.05, 1.0, count)
    return np.stack(boards), np.array(players, np.uint8), np.array(lasts, np.int16), noise, us, Ts


def run_leg(config, leg):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c = CONFIGS[config]
    n, k, S, P = c["n"], c["k"], c["S"], c["positions"]
    boards, players, lasts, noise, us, Ts = _positions(n, k, P, 2024)
    slots = c["slots"] if leg == "batch" else 1
    e = az.Engine(n, k, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)

    def once():
        if leg == "batch":
            r = e.search_batch(boards, players, lasts, Ts, noise, us)
            return int(r["N"].sum())
        tot = 0
        for i in range(P):
            tot += int(e.search(boards[i], int(players[i]), int(lasts[i]), float(Ts[i]), noise[i], float(us[i]))["N"].sum())
        return tot

    if leg == "batch":
        once()                                                  # warm-up: kernels loaded, buffers allocated, graphs captured
    else:
        e.search(boards[0], int(players[0]), int(lasts[0]), float(Ts[0]), noise[0], float(us[0]))
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        tot = once()
        runs.append(time.perf_counter() - t)
        assert tot == P * S
    row = {"config": config, "leg": leg, "library": "parent commit" if leg == "loop_parent" else "this build",
           "board": n, "simulations": S, "slots": slots, "lanes": e.lanes(), "positions": P, "persistent": e.persistent(),
           "runs_seconds": runs, "searches_per_sec": P / statistics.median(runs),
           "ms_per_search": statistics.median(runs) * 1e3 / P}
    e.close()
    print(row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_batch.json"))
    ap.add_argument("--parent-lib", help="libaz_engine.so built from the parent commit (leg a); without it leg a is left out")
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.leg:
        row = run_leg(a.config, a.leg)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    result = {"configs": CONFIGS, "rows": []}
    rc = 0
    for config in ("15x15", "5x5"):
        for leg in LEGS:
            if leg == "loop_parent" and not a.parent_lib:
                continue
            part = a.out + f".{config}.{leg}.part"
            env = dict(os.environ)
            if leg == "loop_parent":
                env["AZ_ENGINE_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("AZ_ENGINE_LIB", None)
            rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
                                 "--leg", leg, "--config", config, "--out", part], cwd=ROOT, env=env).returncode
            if rc != 0:
                print(f"{config} / {leg} failed ({rc}); stopping", flush=True)
                result["failed"] = {"config": config, "leg": leg, "returncode": rc}
                break
            with open(part) as f:
                result["rows"].append(json.load(f))
            os.remove(part)
        if rc != 0:
            break
    by = {(r["config"], r["leg"]): r["searches_per_sec"] for r in result["rows"]}
    result["speedup_over_parent_loop"] = {c: by[(c, "batch")] / by[(c, "loop_parent")] for c in CONFIGS
                                          if (c, "batch") in by and (c, "loop_parent") in by}
    result["loop_this_build_over_parent"] = {c: by[(c, "loop")] / by[(c, "loop_parent")] for c in CONFIGS
                                             if (c, "loop") in by and (c, "loop_parent") in by}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
