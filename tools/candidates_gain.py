#!/usr/bin/env python3
"""What candidate moves (az_set_candidates: expansion, noise and selection over the empty cells within a Chebyshev radius of the
stones) do to self-play throughput, game length and the shape of the searches, on one GPU, from the repo root:

    python tools/candidates_gain.py [--out profiles/candidates.json] [--configs 15x15,9x9,5x5] [--legs off,r1,r2,r3]

Per configuration one steady-state episode shape (games >> slots, slots refilled all the time), the engine's own net kernels
with synthetic weights, and these legs, each in a fresh process of its own under `timeout -k 10`; the first non-zero status
ends the run (what was measured before it is still written):
  off           the option never set
  r1, r2, r3    radius 1, 2, 3
  off_lockstep  5x5 only: the option off with AZ_PERSIST=0, i.e. the lock-step kernels the option runs on -- what giving up the
                persistent search kernel costs by itself
Every leg plays a short warm-up episode and then 3 timed episodes; it reports each run, the median and the spread
(max - min) / median of games/s and node expansions/s, the plies per game, the mean number of distinct root children visited
per record, the mean depth per simulation (the counters' depth_sum / simulations) and the mean size of the root's candidate
set (for the off legs: the legal cells).  There are no pass thresholds: these are measurements.  Whether the option trains a
stronger net per GPU hour is NOT measured here."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "15x15": dict(n=15, k=5, S=400, slots=1024, games=2048),
    "9x9": dict(n=9, k=5, S=200, slots=4096, games=8192),
    "5x5": dict(n=5, k=4, S=100, slots=1024, games=8192),
}
LEGS = {"off": 0, "r1": 1, "r2": 2, "r3": 3, "off_lockstep": 0}
ONLY = {"off_lockstep": ("5x5",)}
RUNS = 3
SAMPLE = 20000          # records the candidate-set size is averaged over


def _stat(xs):
    med = statistics.median(xs)
    return {"runs": xs, "median": med, "spread": (max(xs) - min(xs)) / med if med else None}


def root_candidates(boards, n, radius):
    """mean |C| over the recorded root positions (radius 0: the legal cells), by dilating the occupancy radius times"""
    b = boards[:: max(1, len(boards) // SAMPLE)].reshape(-1, n, n) != 0
    if radius == 0:
        return float((~b).sum(axis=(1, 2)).mean())
    h = b.copy()
    for _ in range(radius):
        t = h.copy()
        t[:, :, 1:] |= h[:, :, :-1]; t[:, :, :-1] |= h[:, :, 1:]
        h = t
    for _ in range(radius):
        t = h.copy()
        t[:, 1:, :] |= h[:, :-1, :]; t[:, :-1, :] |= h[:, 1:, :]
        h = t
    size = (h & ~b).sum(axis=(1, 2))
    return float(np.where(b.any(axis=(1, 2)), size, n * n).mean())


def run_leg(config, leg):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c, radius = CONFIGS[config], LEGS[leg]
    n, kw, S, slots, G = c["n"], c["k"], c["S"], c["slots"], c["games"]
    e = az.Engine(n, kw, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    if radius:
        e.set_candidates(radius)
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, eps, ppg, secs, width, depth, cand = [], [], [], [], [], [], []
    for r in range(RUNS):
        cnt = e.selfplay(G, seed0=1000 + 100000 * r)
        s = cnt["seconds"]
        rec = e.records()
        visits = rec["visits"]
        secs.append(s); gps.append(G / s); eps.append(cnt["expansions"] / s); ppg.append(cnt["plies"] / G)
        width.append(float((visits > 0).sum(axis=1).mean())); depth.append(cnt["depth_sum"] / cnt["simulations"])
        cand.append(root_candidates(rec["boards"], n, radius))
        print(f"  {config} / {leg} run {r}: {s:.2f} s, {G / s:.1f} games/s, {ppg[-1]:.1f} plies per game, {width[-1]:.1f} root children, "
              f"depth {depth[-1]:.2f}, |C| {cand[-1]:.1f}", flush=True)
    row = {"config": config, "leg": leg, "board": n, "simulations": S, "radius": radius, "slots": slots, "lanes": e.lanes(), "games": G,
           "persistent": e.persistent(), "seconds": secs, "games_per_sec": _stat(gps), "expansions_per_sec": _stat(eps),
           "plies_per_game": statistics.median(ppg), "root_children_per_record": statistics.median(width),
           "depth_per_simulation": statistics.median(depth), "root_candidates": statistics.median(cand)}
    e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidates.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg", choices=sorted(LEGS), help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--step-timeout", type=int, default=400)
    a = ap.parse_args()
    if a.leg:
        row = run_leg(a.config, a.leg)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    result = {"configs": CONFIGS, "legs": LEGS, "runs_per_leg": RUNS, "rows": [],
              "not_measured": "whether candidate moves train a stronger net per GPU hour (playing strength)"}
    if os.path.exists(a.out):                  # figures another measurement put beside the table (the bench comparison) stay
        with open(a.out) as f:
            result.update({key: v for key, v in json.load(f).items() if key not in result and key not in ("cost", "failed")})
    rc = 0
    for config in a.configs.split(","):
        for leg in a.legs.split(","):
            if config not in ONLY.get(leg, (config,)):
                continue
            part = a.out + f".{config}.{leg}.part"
            env = dict(os.environ, AZ_PERSIST="0") if leg == "off_lockstep" else None
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
    by = {(r["config"], r["leg"]): r for r in result["rows"]}
    result["cost"] = {}
    for (config, leg), r in by.items():
        if leg != "off" and (config, "off") in by:
            off = by[config, "off"]
            result["cost"].setdefault(config, {})[leg] = {
                "games_per_sec_over_off": r["games_per_sec"]["median"] / off["games_per_sec"]["median"],
                "expansions_per_sec_over_off": r["expansions_per_sec"]["median"] / off["expansions_per_sec"]["median"],
                "plies_per_game_over_off": r["plies_per_game"] / off["plies_per_game"],
                "root_children_over_off": r["root_children_per_record"] / off["root_children_per_record"]}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
