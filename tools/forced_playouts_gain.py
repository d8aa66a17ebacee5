#!/usr/bin/env python3
"""What forced playouts and policy target pruning (az_set_forced_playouts) cost in self-play throughput, on one GPU, from the
repo root:

    python tools/forced_playouts_gain.py [--out profiles/forced_playouts_gain.json] [--configs 15x15,5x5] [--legs off,forced]

Per configuration one steady-state episode shape (games >> slots, slots refilled all the time), the engine's own net kernels
with synthetic weights, and two legs, each in a fresh process of its own under `timeout -k 10`; the first non-zero status ends
the run (what was measured before it is still written):
  off      the option off
  forced   k = 2 with pruning
Every leg plays a short warm-up episode and then 3 timed episodes; it reports each run, the median and the spread
(max - min) / median of games/s and node expansions/s, and the plies per game (forced visits change the moves, and so the
length of the games).  The records keep the raw visits and neither W nor the priors, so what the pruning removes is measured
on a sample: 256 positions of the last episode's records are searched again with fresh root noise (az_search_batch, same
setting) and az_forced_prune is applied to their root statistics -- the share of visits pruned, and of positions with any.
Whether the option helps playing strength per GPU hour is NOT measured here."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "15x15": dict(n=15, k=5, S=400, slots=1024, games=2048),
    "5x5": dict(n=5, k=4, S=100, slots=1024, games=8192),
}
LEGS = {"off": None, "forced": 2.0}
RUNS = 3
SAMPLE = 256


def _stat(xs):
    med = statistics.median(xs)
    return {"runs": xs, "median": med, "spread": (max(xs) - min(xs)) / med if med else None}


def pruned_share(e, k, c_puct, rec, rs):
    """az_forced_prune on the root statistics of SAMPLE recorded positions, searched again with fresh noise"""
    import numpy as np
    from alphazero_piskvorky_amd import _capi
    idx = rs.choice(len(rec["boards"]), size=min(SAMPLE, len(rec["boards"])), replace=False)
    boards = rec["boards"][idx]
    noise = [rs.dirichlet([0.3] * int((b == 0).sum())) for b in boards]
    r = e.search_batch(boards, rec["movers"][idx], rec["lasts"][idx], 1.0, noise, rs.random_sample(len(idx)))
    visits = removed = hit = 0
    for i, b in enumerate(boards):
        legal = np.flatnonzero(b == 0)
        _, rem = _capi.forced_prune(k, c_puct, r["N"][i][legal], r["W"][i][legal], r["P"][i][legal])
        visits += int(r["N"][i].sum()); removed += rem; hit += rem > 0
    return {"positions": int(len(idx)), "visits_pruned_share": removed / visits, "positions_pruned_share": hit / len(idx)}


def run_leg(config, leg):
    import numpy as np
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c, k = CONFIGS[config], LEGS[leg]
    n, kw, S, slots, G = c["n"], c["k"], c["S"], c["slots"], c["games"]
    e = az.Engine(n, kw, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    if k is not None:
        e.set_forced_playouts(k, True)
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, eps, ppg, secs = [], [], [], []
    for r in range(RUNS):
        cnt = e.selfplay(G, seed0=1000 + 100000 * r)
        s = cnt["seconds"]
        secs.append(s); gps.append(G / s); eps.append(cnt["expansions"] / s); ppg.append(cnt["plies"] / G)
        print(f"  {config} / {leg} run {r}: {s:.2f} s, {G / s:.1f} games/s, {ppg[-1]:.1f} plies per game", flush=True)
    row = {"config": config, "leg": leg, "board": n, "simulations": S, "forced_k": k, "prune": k is not None, "slots": slots,
           "lanes": e.lanes(), "games": G, "persistent": e.persistent(), "seconds": secs, "games_per_sec": _stat(gps),
           "expansions_per_sec": _stat(eps), "plies_per_game": statistics.median(ppg)}
    if k is not None:
        row["pruning_sample"] = pruned_share(e, k, 2.0, e.records(), np.random.RandomState(7))
    e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forced_playouts_gain.json"))
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
    result = {"configs": CONFIGS, "runs_per_leg": RUNS, "rows": [],
              "not_measured": "whether forced playouts and target pruning help playing strength per GPU hour"}
    rc = 0
    for config in a.configs.split(","):
        for leg in a.legs.split(","):
            part = a.out + f".{config}.{leg}.part"
            rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
                                 "--leg", leg, "--config", config, "--out", part], cwd=ROOT).returncode
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
    result["cost"] = {config: {"games_per_sec_over_off": by[config, "forced"]["games_per_sec"]["median"] / by[config, "off"]["games_per_sec"]["median"],
                               "expansions_per_sec_over_off": by[config, "forced"]["expansions_per_sec"]["median"] / by[config, "off"]["expansions_per_sec"]["median"]}
                      for config in CONFIGS if (config, "off") in by and (config, "forced") in by}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
