#!/usr/bin/env python3
"""What the Gumbel root search (az_set_gumbel) costs and buys in self-play throughput, on one GPU, from the repo root:

    python tools/gumbel_gain.py [--out profiles/gumbel.json] [--configs 15x15,5x5] [--legs puct,puct32,gumbel32]
                                [--parent-lib PATH/libaz_engine_parent.so]

Per configuration one steady-state episode shape (games >> slots, slots refilled all the time), the engine's own net kernels
with synthetic weights, and three legs, each in a fresh process of its own under `timeout -k 10`; the first non-zero status
ends the run (what was measured before it is still written):
  puct       the option off at the configuration's headline simulation count
  puct32     the option off at 32 simulations per move
  gumbel32   m = 16, c_visit = 50, c_scale = 1 at 32 simulations per move
puct32 against gumbel32 is the rule's own cost per simulation at an equal budget; puct against gumbel32 is the games per second
a user gains by moving to the small budget the rule is made for.  Every leg plays a short warm-up episode and then 3 timed
episodes; it reports each run, the median and the spread (max - min) / median of games/s and node expansions/s, the plies per
game, and which search kernel served.
--parent-lib: the cost with the option OFF.  bench.py (unchanged) runs three times on a library built from the parent commit
(AZ_ENGINE_LIB) and three times on this build, alternating; both sets of numbers are written down.
Whether Gumbel targets at 32 simulations train a stronger net per GPU hour than visit counts at 400 is NOT measured here."""
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
LEGS = {"puct": dict(S=None, m=0), "puct32": dict(S=32, m=0), "gumbel32": dict(S=32, m=16)}
RUNS = 3


def _stat(xs):
    med = statistics.median(xs)
    return {"runs": xs, "median": med, "spread": (max(xs) - min(xs)) / med if med else None}


def run_leg(config, leg):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c, lg = CONFIGS[config], LEGS[leg]
    n, kw, slots = c["n"], c["k"], c["slots"]
    S = lg["S"] or c["S"]
    G = c["games"] * (4 if S < c["S"] else 1)             # the short searches play more games in the same time
    e = az.Engine(n, kw, S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    if lg["m"]:
        e.set_gumbel(lg["m"])
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, eps, ppg, secs = [], [], [], []
    for r in range(RUNS):
        cnt = e.selfplay(G, seed0=1000 + 100000 * r)
        s = cnt["seconds"]
        secs.append(s); gps.append(G / s); eps.append(cnt["expansions"] / s); ppg.append(cnt["plies"] / G)
        print(f"  {config} / {leg} run {r}: {s:.2f} s, {G / s:.1f} games/s, {ppg[-1]:.1f} plies per game", flush=True)
    row = {"config": config, "leg": leg, "board": n, "simulations": S, "gumbel": e.gumbel(), "slots": slots, "lanes": e.lanes(),
           "games": G, "persistent": e.persistent(), "search_kernel": "k_search (persistent)" if e.persistent() else "k_step (lock-step)",
           "seconds": secs, "games_per_sec": _stat(gps), "expansions_per_sec": _stat(eps), "plies_per_game": statistics.median(ppg)}
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
    return out, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gumbel.json"))
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
    result = {"configs": CONFIGS, "legs": LEGS, "runs_per_leg": RUNS, "rows": [],
              "not_measured": "whether Gumbel targets at 32 simulations train a stronger net per GPU hour than visit counts at 400"}
    if os.path.exists(a.out):                             # a run split over several calls keeps what the earlier ones measured
        with open(a.out) as f:
            old = json.load(f)
        result["rows"] = [r for r in old.get("rows", []) if not (r["config"] in a.configs.split(",") and r["leg"] in a.legs.split(","))]
        for key in ("option_off", "build"):
            if key in old:
                result[key] = old[key]

    def save():
        by = {(r["config"], r["leg"]): r for r in result["rows"]}

        def ratio(config, a_leg, b_leg, key):
            return by[config, a_leg][key]["median"] / by[config, b_leg][key]["median"]
        result["cost"] = {config: {"gumbel32_over_puct32_games_per_sec": ratio(config, "gumbel32", "puct32", "games_per_sec"),
                                   "gumbel32_over_puct32_expansions_per_sec": ratio(config, "gumbel32", "puct32", "expansions_per_sec"),
                                   "gumbel32_over_puct_games_per_sec": ratio(config, "gumbel32", "puct", "games_per_sec")}
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
