#!/usr/bin/env python3
"""What the root threat search (az_set_threat_search) costs and changes in self-play next to the solver alone, on one GPU, from
the repo root:

    python tools/threat_gain.py [--out profiles/threat.json] [--configs 15x15,9x9,5x5] [--legs solver,threat,solver-lockstep]
                                [--parent-lib PATH/libaz_engine_parent.so]

Per configuration one steady-state episode shape (games >> slots), the engine's own net kernels with synthetic weights, and the
legs -- the solver alone, the solver with the threat search (max_depth 8, node_budget 256), and at 5x5 also the solver alone
under AZ_PERSIST=0, since the option gives the persistent kernel up -- each in a fresh process of its own under `timeout -k 10`;
the first non-zero status ends the run (what was measured before it is still written).  Every leg plays a short warm-up episode
and then 3 timed episodes; it reports each run, the median and the spread of games/s and node expansions/s, plies per game, net
evaluations per ply, the share of roots proven WIN / LOSS / block-only by the threat search, the depth histogram, nodes per root
(mean, the maximum of a probe with the budget at 65535 over a sample of the last episode's records, share exhausted), the missed wins, and
the time of az_threat_batch on one wave of the last episode's records against the ply's (16 calls between two events: upload,
position kernel, threat kernel per lane one after another, one synchronisation -- an upper bound of the kernel's share).
--parent-lib: the cost with the option OFF, bench.py (unchanged) three times on a library built from the parent commit
(AZ_ENGINE_LIB) and three times on this build, alternating.
Whether the threat search trains a stronger net per GPU hour is NOT measured here."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from solver_gain import _stat, bench_off, missed_wins  # noqa: E402

CONFIGS = {
    "15x15": dict(n=15, k=5, S=400, slots=1024, games=2048),
    "9x9": dict(n=9, k=5, S=200, slots=4096, games=8192),
    "5x5": dict(n=5, k=4, S=100, slots=1024, games=8192),
}
LEGS = ("solver", "threat", "solver-lockstep")
RUNS = 3
DEPTH, BUDGET = 8, 256


def run_leg(config, leg):
    if leg == "solver-lockstep":
        os.environ["AZ_PERSIST"] = "0"
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c = CONFIGS[config]
    n, kw, S, slots, G = c["n"], c["k"], c["S"], c["slots"], c["games"]
    e = az.Engine(n, kw, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    e.set_solver(True)
    if leg == "threat":
        e.set_threat_search(DEPTH, BUDGET)
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, eps, ppg, secs, evals, stats = [], [], [], [], [], []
    for r in range(RUNS):
        cnt = e.selfplay(G, seed0=1000 + 100000 * r)
        s = cnt["seconds"]
        secs.append(s); gps.append(G / s); eps.append(cnt["expansions"] / s); ppg.append(cnt["plies"] / G)
        evals.append(cnt["trunk_boards"] / cnt["plies"])
        stats.append(dict(e.threat_stats(), plies=cnt["plies"]))
        print(f"  {config} / {leg} run {r}: {s:.2f} s, {G / s:.1f} games/s, {ppg[-1]:.1f} plies per game", flush=True)
    rec = e.records()
    could, missed = missed_wins(rec, n, kw)
    proofs = e.proofs()
    row = {"config": config, "leg": leg, "board": n, "simulations": S, "slots": slots, "lanes": e.lanes(), "games": G,
           "threat_search": list(e.threat_search()), "persistent": e.persistent(), "seconds": secs, "games_per_sec": _stat(gps),
           "expansions_per_sec": _stat(eps), "plies_per_game": statistics.median(ppg), "net_evaluations_per_ply": _stat(evals),
           "records": len(rec["movers"]), "records_with_an_immediate_win": could, "missed_wins": missed,
           "proven_roots_after_the_search": {name: float((proofs == code).mean()) for name, code in (("win", 1), ("loss", 2), ("draw", 3))}}
    if leg == "threat":
        t = e.threats()
        last = stats[-1]
        row["threat_roots"] = {key: sum(s[key] for s in stats) / sum(s["plies"] for s in stats) for key in ("win_roots", "lost_roots", "block_roots", "exhausted")}
        row["nodes_per_root_mean"] = sum(s["nodes"] for s in stats) / sum(s["plies"] for s in stats)
        row["depth_histogram"] = {str(d): int((t == d).sum()) for d in range(0, DEPTH + 1)}
        # what the default budget rests on: the same roots with the budget out of the way
        sub = np.random.RandomState(1).choice(len(rec["movers"]), min(len(rec["movers"]), 8 * slots), replace=False)
        probe = e.threat_batch(rec["boards"][sub], rec["movers"][sub], DEPTH, 65535, outputs=("nodes",))["nodes"]
        row["nodes_per_root_unlimited"] = {"mean": float(probe.mean()), "max": int(probe.max()), "p999": float(np.quantile(probe, 0.999)),
                                           "share_above_budget": float((probe > BUDGET).mean()), "records_probed": int(len(sub))}
        row["last_episode_exhausted"] = last["exhausted"]
        # the kernel alone, HIP events: the records' boards in waves of the slots, against the ply time of the timed episodes
        import torch
        pick = np.random.RandomState(0).choice(len(rec["movers"]), slots, replace=False)     # a wave with the episode's mix of plies
        boards, movers = rec["boards"][pick], rec["movers"][pick]
        e.threat_batch(boards, movers, DEPTH, BUDGET, outputs=("nodes",))
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); t0.record()
        for _ in range(16):
            e.threat_batch(boards, movers, DEPTH, BUDGET, outputs=())
        t1.record(); torch.cuda.synchronize()
        call_ms = t0.elapsed_time(t1) / 16                 # one wave: upload, position kernel, threat kernel, one sync
        ply_ms = 1e3 * statistics.median(secs) / (statistics.median(ppg) * G / slots)
        row["threat_batch_wave_ms"] = call_ms
        row["ply_ms"] = ply_ms
        row["wave_over_ply"] = call_ms / ply_ms
    e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threat.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: measure the cost with the option off")
    ap.add_argument("--step-timeout", type=int, default=400)
    a = ap.parse_args()
    if a.leg:
        row = run_leg(a.config, a.leg)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    result = {"configs": CONFIGS, "legs": list(LEGS), "runs_per_leg": RUNS, "max_depth": DEPTH, "node_budget": BUDGET, "rows": [],
              "not_measured": "whether the threat search trains a stronger net per GPU hour"}
    if os.path.exists(a.out):                             # a run split over several calls keeps what the earlier ones measured
        with open(a.out) as f:
            old = json.load(f)
        result["rows"] = [r for r in old.get("rows", []) if not (r["config"] in a.configs.split(",") and r["leg"] in a.legs.split(","))]
        if "option_off" in old:
            result["option_off"] = old["option_off"]

    def save():
        by = {(r["config"], r["leg"]): r for r in result["rows"]}
        result["threat_over_solver"] = {config: {key: by[config, "threat"][key]["median"] / by[config, "solver"][key]["median"]
                                                 for key in ("games_per_sec", "expansions_per_sec", "net_evaluations_per_ply")}
                                        for config in CONFIGS if all((config, leg) in by for leg in ("solver", "threat"))}
        with open(a.out, "w") as f:                       # after every step: a run that is cut short keeps what it measured
            json.dump(result, f, indent=1)

    rc = 0
    for config in [c for c in a.configs.split(",") if c]:
        for leg in [x for x in a.legs.split(",") if x]:
            if rc != 0:
                break
            if leg == "solver-lockstep" and config != "5x5":
                continue                                  # only 5x5 has a persistent kernel to give up
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
            save()
    if a.parent_lib and rc == 0:
        result["option_off"], rc = bench_off(a.parent_lib, a.step_timeout)
    save()
    print(json.dumps({k: result[k] for k in result if k != "rows"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
