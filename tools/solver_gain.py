#!/usr/bin/env python3
"""What the MCTS-Solver (az_set_solver) costs and changes in self-play, on one GPU, from the repo root:

    python tools/solver_gain.py [--out profiles/solver.json] [--configs 15x15,9x9,5x5] [--legs off,on]
                                [--parent-lib PATH/libaz_engine_parent.so]

Per configuration one steady-state episode shape (games >> slots, slots refilled all the time), the engine's own net kernels
with synthetic weights, and two legs -- the option off and on -- each in a fresh process of its own under `timeout -k 10`; the
first non-zero status ends the run (what was measured before it is still written).  Every leg plays a short warm-up episode and
then 3 timed episodes; it reports each run, the median and the spread (max - min) / median of games/s and node expansions/s,
the plies per game, the terminal hits per simulation and, among them, the stops on proven edges per simulation
(az_solver_stops), the share of records whose root is proven, by status,
and the "missed wins": records where the mover had a cell that makes the line at once and played elsewhere, counted on the host
from the boards and actions of the last timed episode.
--parent-lib: the cost with the option OFF.  bench.py (unchanged) runs three times on a library built from the parent commit
(AZ_ENGINE_LIB) and three times on this build, alternating; both sets of numbers are written down.
Whether the solver trains a stronger net per GPU hour is NOT measured here."""
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
LEGS = {"off": 0, "on": 1}
RUNS = 3


def _stat(xs):
    med = statistics.median(xs)
    return {"runs": xs, "median": med, "spread": (max(xs) - min(xs)) / med if med else None}


def winning_cells(boards, movers, n, k):
    """bool[R, n, n]: the empty cells with which the mover makes a line of k at once (a window of k cells along a row, a column
    or a diagonal that holds k - 1 of the mover's stones and this empty cell)"""
    b = boards.reshape(-1, n, n)
    me = b == movers[:, None, None]
    empty = b == 0
    out = np.zeros(b.shape, bool)
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        rows = n - (k - 1) * dr
        cols = n - (k - 1) * abs(dc)
        c0 = (k - 1) if dc < 0 else 0

        def window(x, s):
            return x[:, s * dr:s * dr + rows, c0 + s * dc:c0 + s * dc + cols]
        mine = sum(window(me, s).astype(np.int8) for s in range(k))
        for s in range(k):
            hit = (mine == k - 1) & window(empty, s)
            out[:, s * dr:s * dr + rows, c0 + s * dc:c0 + s * dc + cols] |= hit
    return out


def missed_wins(rec, n, k):
    """(records where the mover could win at once, those among them where it played another cell)"""
    win = winning_cells(rec["boards"], rec["movers"], n, k).reshape(len(rec["movers"]), n * n)
    could = win.any(axis=1)
    played = win[np.arange(len(could)), rec["actions"].astype(np.int64)]
    return int(could.sum()), int((could & ~played).sum())


def run_leg(config, leg):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c = CONFIGS[config]
    n, kw, S, slots, G = c["n"], c["k"], c["S"], c["slots"], c["games"]
    e = az.Engine(n, kw, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    e.set_solver(bool(LEGS[leg]))
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, eps, ppg, secs, term, stops = [], [], [], [], [], []
    for r in range(RUNS):
        cnt = e.selfplay(G, seed0=1000 + 100000 * r)
        s = cnt["seconds"]
        secs.append(s); gps.append(G / s); eps.append(cnt["expansions"] / s); ppg.append(cnt["plies"] / G)
        term.append(cnt["terminal_hits"] / cnt["simulations"])
        stops.append(e.solver_stops() / cnt["simulations"])
        print(f"  {config} / {leg} run {r}: {s:.2f} s, {G / s:.1f} games/s, {ppg[-1]:.1f} plies per game", flush=True)
    rec = e.records()
    could, missed = missed_wins(rec, n, kw)
    row = {"config": config, "leg": leg, "board": n, "simulations": S, "solver": e.solver(), "slots": slots, "lanes": e.lanes(),
           "games": G, "persistent": e.persistent(), "search_kernel": "k_search (persistent)" if e.persistent() else "k_step (lock-step)",
           "seconds": secs, "games_per_sec": _stat(gps), "expansions_per_sec": _stat(eps), "plies_per_game": statistics.median(ppg),
           "terminal_hits_per_simulation": _stat(term), "proven_edge_stops_per_simulation": _stat(stops), "records": len(rec["movers"]),
           "records_with_an_immediate_win": could, "missed_wins": missed}
    if LEGS[leg]:
        proofs = e.proofs()
        row["proven_roots"] = {name: float((proofs == code).mean()) for name, code in (("win", 1), ("loss", 2), ("draw", 3))}
    e.close()
    return row


def bench_off(parent_lib, step_timeout):
    """bench.py on the parent's library and on this build, alternating, three runs each"""
    out = {"command": "bench.py --gpus 1 --steps 8 --warmup 1 --no-cpu --no-emul", "parent": [], "this": []}
    for r in range(RUNS):
        for name, libpath in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("AZ_ENGINE_LIB", None)
            if libpath:
                env["AZ_ENGINE_LIB"] = os.path.abspath(libpath)
            p = subprocess.run(["timeout", "-k", "10", str(step_timeout), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                                "--steps", "8", "--warmup", "1", "--no-cpu", "--no-emul"], cwd=ROOT, env=env, capture_output=True, text=True)
            if p.returncode != 0:
                out["failed"] = {"which": name, "run": r, "returncode": p.returncode, "stderr": p.stderr[-1000:]}
                return out, p.returncode
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            out[name].append(json.loads(line)["value"])
            print(f"  bench {name} run {r}: {out[name][-1]:.0f} node expansions/s", flush=True)
    out["parent"], out["this"] = _stat(out["parent"]), _stat(out["this"])
    out["this_over_parent"] = out["this"]["median"] / out["parent"]["median"]
    lo, hi = min(out["parent"]["runs"]), max(out["parent"]["runs"])
    out["this_median_inside_parent_runs"] = bool(lo <= out["this"]["median"] <= hi)
    return out, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg", choices=sorted(LEGS), help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: measure the cost with the option off")
    ap.add_argument("--step-timeout", type=int, default=400)
    a = ap.parse_args()
    if a.leg:
        row = run_leg(a.config, a.leg)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    result = {"configs": CONFIGS, "legs": list(LEGS), "runs_per_leg": RUNS, "rows": [],
              "not_measured": "whether the solver trains a stronger net per GPU hour"}
    if os.path.exists(a.out):                             # a run split over several calls keeps what the earlier ones measured
        with open(a.out) as f:
            old = json.load(f)
        result["rows"] = [r for r in old.get("rows", []) if not (r["config"] in a.configs.split(",") and r["leg"] in a.legs.split(","))]
        for key in ("option_off", "build"):
            if key in old:
                result[key] = old[key]

    def save():
        by = {(r["config"], r["leg"]): r for r in result["rows"]}
        result["on_over_off"] = {config: {key: by[config, "on"][key]["median"] / by[config, "off"][key]["median"]
                                          for key in ("games_per_sec", "expansions_per_sec")}
                                 for config in CONFIGS if all((config, leg) in by for leg in LEGS)}
        with open(a.out, "w") as f:                       # after every step: a run that is cut short keeps what it measured
            json.dump(result, f, indent=1)

    rc = 0
    for config in [c for c in a.configs.split(",") if c]:
        for leg in [x for x in a.legs.split(",") if x]:
            if rc != 0:
                break
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
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
