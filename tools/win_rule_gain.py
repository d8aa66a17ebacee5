#!/usr/bin/env python3
"""What the exact-k win rule (az_set_win_rule, standard Gomoku) changes in self-play against the freestyle default, on one GPU,
from the repo root:

    python tools/win_rule_gain.py [--out profiles/win_rule.json] [--configs 15x15,9x9,5x5] [--legs freestyle,exact]
                                  [--parent-lib PATH/libaz_engine_parent.so]

Per configuration one steady-state episode shape (games >> slots, slots refilled all the time), the engine's own net kernels
with synthetic weights, and two legs -- the rule never set and the rule set to exact -- each in a fresh process of its own under
`timeout -k 10`; the first non-zero status ends the run (what was measured before it is still written).  Every leg plays a short
warm-up episode and then 3 timed episodes; it reports each run, the median and the spread (max - min) / median of games/s and
node expansions/s, the mean plies per game, the share of drawn games and the share of games in which any overline (a run of
win_length + 1 or more) was made, counted on the host from the final boards of the last timed episode (a run never shrinks, so
the final board shows every overline that was ever made).
--parent-lib: the cost with the rule never set.  bench.py (unchanged) runs three times on a library built from the parent
commit (AZ_ENGINE_LIB) and three times on this build, alternating; both sets of numbers are written down.
Whether exact-rule self-play trains a stronger standard-rule net is NOT measured here."""
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
LEGS = ("freestyle", "exact")
RUNS = 3


def _stat(xs):
    med = statistics.median(xs)
    return {"runs": xs, "median": med, "spread": (max(xs) - min(xs)) / med if med else None}


def has_run(boards, n, length):
    """bool[G]: the board holds `length` stones of one colour in a row, a column or a diagonal"""
    b = boards.reshape(-1, n, n)
    out = np.zeros(len(b), bool)
    if length > n:
        return out
    for colour in (1, 2):
        me = b == colour
        for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
            rows = n - (length - 1) * dr
            cols = n - (length - 1) * abs(dc)
            c0 = (length - 1) if dc < 0 else 0
            full = np.ones((len(b), rows, cols), bool)
            for s in range(length):
                full &= me[:, s * dr:s * dr + rows, c0 + s * dc:c0 + s * dc + cols]
            out |= full.any(axis=(1, 2))
    return out


def final_boards(rec, nply, n):
    """the board of every game after its last move"""
    last = np.cumsum(nply) - 1
    boards = rec["boards"][last].copy()
    boards[np.arange(len(last)), rec["actions"][last].astype(np.int64)] = rec["movers"][last]
    return boards


def run_leg(config, leg):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c = CONFIGS[config]
    n, kw, S, slots, G = c["n"], c["k"], c["S"], c["slots"], c["games"]
    e = az.Engine(n, kw, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    if leg != "freestyle":                               # the freestyle leg never sets the rule: the default engine
        e.set_win_rule(leg)
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, eps, ppg, secs, draws = [], [], [], [], []
    for r in range(RUNS):
        cnt = e.selfplay(G, seed0=1000 + 100000 * r)
        s = cnt["seconds"]
        secs.append(s); gps.append(G / s); eps.append(cnt["expansions"] / s); ppg.append(cnt["plies"] / G)
        draws.append(float((e.games()[1] == 3).mean()))
        print(f"  {config} / {leg} run {r}: {s:.2f} s, {G / s:.1f} games/s, {ppg[-1]:.1f} plies per game", flush=True)
    nply, res = e.games()
    over = has_run(final_boards(e.records(), nply, n), n, kw + 1)
    row = {"config": config, "leg": leg, "board": n, "win_length": kw, "simulations": S, "win_rule": e.win_rule(), "slots": slots,
           "lanes": e.lanes(), "games": G, "persistent": e.persistent(),
           "search_kernel": "k_search (persistent)" if e.persistent() else "k_step (lock-step)",
           "seconds": secs, "games_per_sec": _stat(gps), "expansions_per_sec": _stat(eps), "plies_per_game": _stat(ppg),
           "draw_share": _stat(draws), "games_with_an_overline_share": float(over.mean()),
           "results_last_episode": {name: float((res == code).mean()) for name, code in (("x", 1), ("o", 2), ("draw", 3))}}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "win_rule.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: measure the cost with the rule never set")
    ap.add_argument("--step-timeout", type=int, default=400)
    a = ap.parse_args()
    if a.leg:
        row = run_leg(a.config, a.leg)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    result = {"configs": CONFIGS, "legs": list(LEGS), "runs_per_leg": RUNS, "rows": [],
              "not_measured": "whether exact-rule self-play trains a stronger standard-rule net"}
    if os.path.exists(a.out):                             # a run split over several calls keeps what the earlier ones measured
        with open(a.out) as f:
            old = json.load(f)
        result["rows"] = [r for r in old.get("rows", []) if not (r["config"] in a.configs.split(",") and r["leg"] in a.legs.split(","))]
        for key in ("rule_never_set", "build"):
            if key in old:
                result[key] = old[key]

    def save():
        by = {(r["config"], r["leg"]): r for r in result["rows"]}
        result["exact_over_freestyle"] = {config: {key: by[config, "exact"][key]["median"] / by[config, "freestyle"][key]["median"]
                                                   for key in ("games_per_sec", "expansions_per_sec", "plies_per_game")}
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
        result["rule_never_set"], rc = bench_off(a.parent_lib, a.step_timeout)
    save()
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
