#!/usr/bin/env python3
"""What playout cap randomisation (az_set_playout_cap) buys in self-play throughput, on one GPU, from the repo root:

    python tools/playout_cap_gain.py [--out profiles/playout_cap.json] [--configs 15x15,9x9,5x5] [--legs off,cap,...]

Per configuration one steady-state episode shape (games >> slots, slots refilled all the time), the engine's own net kernels
with synthetic weights, and these legs, each in a fresh process of its own under `timeout -k 10`; the first non-zero status
ends the run (what was measured before it is still written):
  off           the cap off: the replayed graph of a whole ply (the persistent search kernel at 5x5)
  cap           F = S / 4 at 250 permille, full-first compaction
  cap_nocompact the same with AZ_COMPACT=0: phase B runs over every slot, the budgets keep the FAST ones idle
  off_eager     the cap off with AZ_GRAPH=0 (and AZ_PERSIST=0): what launching a ply kernel by kernel costs
  cap_1000      F = S / 4 at 1000 permille: the work of `off` through the capped ply's two eager phases
Every leg plays a short warm-up episode and then 3 timed episodes; it reports each run, the median and the spread
(max - min) / median of games/s, FULL records/s and node expansions/s, and mean(sims) / S of the episode, which is the
ceiling of the gain.  Whether the cap helps playing strength per GPU hour is NOT measured here."""
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
    "9x9": dict(n=9, k=5, S=200, slots=4096, games=8192),
    "5x5": dict(n=5, k=4, S=100, slots=1024, games=8192),
}
LEGS = {
    "off": dict(cap=None, env={}),
    "cap": dict(cap=250, env={}),
    "cap_nocompact": dict(cap=250, env={"AZ_COMPACT": "0"}),
    "off_eager": dict(cap=None, env={"AZ_GRAPH": "0", "AZ_PERSIST": "0"}),
    "cap_1000": dict(cap=1000, env={}),
}
RUNS = 3


def _stat(xs):
    med = statistics.median(xs)
    return {"runs": xs, "median": med, "spread": (max(xs) - min(xs)) / med if med else None}


def run_leg(config, leg):
    import numpy as np
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c, spec = CONFIGS[config], LEGS[leg]
    n, k, S, slots, G = c["n"], c["k"], c["S"], c["slots"], c["games"]
    e = az.Engine(n, k, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    F = S // 4
    if spec["cap"] is not None:
        e.set_playout_cap(F, spec["cap"] / 1000, export_full_only=True)
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, fps, eps, ratio, secs = [], [], [], [], []
    for r in range(RUNS):
        cnt = e.selfplay(G, seed0=1000 + 100000 * r)
        sims = e.sims()
        s = cnt["seconds"]
        secs.append(s); gps.append(G / s); fps.append(float((sims == S).sum()) / s); eps.append(cnt["expansions"] / s)
        ratio.append(float(sims.mean()) / S)
        assert cnt["simulations"] == int(sims.sum())
        print(f"  {config} / {leg} run {r}: {s:.2f} s, {G / s:.1f} games/s, mean sims / S = {ratio[-1]:.3f}", flush=True)
    row = {"config": config, "leg": leg, "board": n, "simulations": S, "fast_sims": F if spec["cap"] is not None else None,
           "full_permille": spec["cap"], "env": spec["env"], "slots": slots, "lanes": e.lanes(), "games": G,
           "persistent": e.persistent(), "seconds": secs, "games_per_sec": _stat(gps), "full_records_per_sec": _stat(fps),
           "expansions_per_sec": _stat(eps), "mean_sims_over_S": statistics.median(ratio), "steps_last_run": cnt["steps"],
           "plies_last_run": cnt["plies"]}
    e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_cap.json"))
    ap.add_argument("--configs", default="15x15,9x9,5x5")
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
              "not_measured": "whether the cap helps playing strength per GPU hour"}
    rc = 0
    for config in a.configs.split(","):
        for leg in a.legs.split(","):
            part = a.out + f".{config}.{leg}.part"
            env = {key: v for key, v in os.environ.items() if key not in ("AZ_COMPACT", "AZ_GRAPH", "AZ_PERSIST")}
            env.update(LEGS[leg]["env"])
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
    gain = {}
    for config in CONFIGS:
        off = by.get((config, "off"))
        for leg in ("cap", "cap_nocompact", "off_eager", "cap_1000"):
            r = by.get((config, leg))
            if off and r:
                gain[f"{config}/{leg}"] = {
                    "games_per_sec_over_off": r["games_per_sec"]["median"] / off["games_per_sec"]["median"],
                    "full_records_per_sec_over_off": r["full_records_per_sec"]["median"] / off["full_records_per_sec"]["median"],
                    "ceiling_S_over_mean_sims": 1.0 / r["mean_sims_over_S"]}
    result["gain"] = gain
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
