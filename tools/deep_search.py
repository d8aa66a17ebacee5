#!/usr/bin/env python3
"""Deep searches (az_create_deep, more than 1024 simulations per move): latency and rates on one GPU, from the repo root:

    python tools/deep_search.py [--out profiles/deep_search.json] [--step-timeout 300]

Every measurement runs in a child process of its own under its own time limit; the first one that fails or runs out of
time ends the run (what was measured before it is still written).  Steps:
  search    15x15 single search from the empty board (seeded GomokuNet), S = 1000 / 1600 / 10 000, L = 1 and 8:
            median of 5 after one warm-up, ms per search and us per simulation
  selfplay  15x15 self-play, 256 games on 256 slots cut at 4 plies, S = 400 vs 1600: expansions/s
  small     5x5, 1024 games on 1024 slots, S = 1600 (deep, launched kernel by kernel): games/s; beside it S = 1000 with the
            ply graph and with AZ_GRAPH=0, the cost of launching kernel by kernel where both paths exist
  arena     the 51-game 15x15 arena of ModelEvaluator.evaluate at S = 1600 (two seeded nets): seconds
and the tree bytes per slot, (S + 1) x roundup(n^2, 64) x 16 B."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("search", "selfplay", "small", "arena")


def _engine(n, k, S, slots, **kw):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    return az.Engine(n, k, S, slots, log_table=numpy_log_table(S), deep=S > az._capi.AZ_MAX_SIMULATIONS, **kw)


def step_search():
    import numpy as np
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    n, k = 15, 5
    sd = synthetic_state_dict(n)
    board = np.zeros(n * n, np.uint8)
    rows = []
    for S in (1000, 1600, 10_000):
        for L in (1, 8):
            e = _engine(n, k, S, 1)
            e.load_weights(sd, 0)
            e.set_virtual_loss(L)
            e.search(board, 1, -1, 1.0, None, 0.5)
            ts = []
            for _ in range(5):
                t = time.perf_counter()
                r = e.search(board, 1, -1, 1.0, None, 0.5)
                ts.append(time.perf_counter() - t)
            assert int(r["N"].sum()) == S
            e.close()
            ms = statistics.median(ts) * 1e3
            rows.append({"S": S, "L": L, "ms_per_search": ms, "us_per_simulation": ms * 1e3 / S, "runs_ms": [t * 1e3 for t in ts]})
            print(rows[-1], flush=True)
    return {"search_15x15": rows}


def _selfplay_rate(n, k, S, G, cut, sd, env=None):
    old = {key: os.environ.get(key) for key in (env or {})}
    os.environ.update(env or {})
    try:
        e = _engine(n, k, S, G)
    finally:
        for key, v in old.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
    e.load_weights(sd, 0)
    e.selfplay(min(G, 8), seed0=1, max_plies=2)                # warm-up: kernels loaded, graphs captured
    t = time.perf_counter()
    c = e.selfplay(G, seed0=100, max_plies=cut)
    dt = time.perf_counter() - t
    pers = e.persistent()
    e.close()
    return {"S": S, "games": G, "max_plies": cut, "seconds": dt, "plies": int(c["plies"]), "expansions": int(c["expansions"]),
            "expansions_per_sec": c["expansions"] / dt, "games_per_sec": G / dt, "persistent": pers}


def step_selfplay():
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(15)
    rows = []
    for S in (400, 1600):
        rows.append(_selfplay_rate(15, 5, S, 256, 4, sd))
        print(rows[-1], flush=True)
    return {"selfplay_15x15": rows}


def step_small():
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(5)
    rows = []
    for S, env, how in ((1600, None, "deep: kernel by kernel"), (1000, {"AZ_PERSIST": "0"}, "ply graph"),
                        (1000, {"AZ_PERSIST": "0", "AZ_GRAPH": "0"}, "kernel by kernel (AZ_GRAPH=0)")):
        r = _selfplay_rate(5, 4, S, 1024, 0, sd, env)
        r["launch"] = how
        rows.append(r)
        print(rows[-1], flush=True)
    return {"selfplay_5x5": rows}


def step_arena():
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    n, k, S, G = 15, 5, 1600, 51
    e = _engine(n, k, S, G)
    e.load_weights(synthetic_state_dict(n), 0)
    e.load_weights(synthetic_state_dict(n, seed=99), 1)
    e.arena(2, seed0=7)                                        # warm-up
    t = time.perf_counter()
    r = e.arena(G, seed0=1)
    dt = time.perf_counter() - t
    e.close()
    row = {"S": S, "games": G, "seconds": dt, "plies": int(r["nply"].sum()), "tally": [int(r["wins"]), int(r["losses"]), int(r["draws"])]}
    print(row, flush=True)
    return {"arena_15x15": row}


def tree_bytes():
    out = {}
    for n in (5, 9, 15):
        RW = (n * n + 63) // 64 * 64
        out[f"{n}x{n}"] = {str(S): (S + 1) * RW * 16 for S in (1000, 1600, 10_000, 65_534)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_search.json"))
    ap.add_argument("--step", choices=STEPS, help="run one measurement in this process (what the parent does per child)")
    ap.add_argument("--step-timeout", type=float, default=300.0)
    a = ap.parse_args()
    if a.step:
        res = globals()["step_" + a.step]()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    import torch
    result = {"device": torch.cuda.get_device_name(0), "tree_bytes_per_slot": tree_bytes()}
    rc = 0
    for s in STEPS:
        part = a.out + f".{s}.part"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", s, "--out", part], cwd=ROOT,
                               timeout=a.step_timeout)
            rc = p.returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {s} failed ({rc}); stopping", flush=True)
            result["failed_step"] = {"step": s, "returncode": rc}
            break
        with open(part) as f:
            result.update(json.load(f))
        os.remove(part)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
