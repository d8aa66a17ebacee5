"""Latency of the single-position search entry points: milliseconds per call of az_search and of
az_search_callback with a trivial evaluator, through the raw C-ABI, on a one-slot engine (MCTS.run's configuration).

  5x5 / S = 64     az_search runs the persistent search kernel; the callback never does
  15x15 / S = 200  lock-step, the captured graph for az_search; and Engine.net_eval (az_net_eval) of 1 and of 256 positions on
                   a 256-slot engine: the tile-split trunk for the one, one full pass for the 256

    python tools/preset_search_latency.py --parent-lib <libaz_engine.so built from the parent commit>

runs parent, this build, parent, this build per configuration (the parent twice: the spread between its two runs is what a
difference is judged by), every leg a fresh process under `timeout -k 10` with the library selected through AZ_ENGINE_LIB, after
20 warm-up calls; a host clock around each synchronising call.  Writes --out (default profiles/preset_search_path.json)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"5x5": dict(n=5, k=4, S=64, calls=600, callback_calls=400), "15x15": dict(n=15, k=5, S=200, calls=400, callback_calls=300, net_eval={1: 400, 256: 150})}
LEGS = ("parent_1", "branch_1", "parent_2", "branch_2")
WARMUP = 20


def run_leg(config, leg):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd import _capi
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    cfg = CONFIGS[config]
    n, k, S = cfg["n"], cfg["k"], cfg["S"]
    nn = n * n
    e = az.Engine(n, k, S, 1)
    e.load_weights(synthetic_state_dict(n), 0)
    board = np.zeros(nn, np.uint8)
    board[n + 1] = 1; board[2 * n + 2] = 2; board[n + 2] = 1
    noise = np.random.RandomState(3).dirichlet([0.3] * (nn - 3))
    L, p = _capi.lib(), _capi._p
    pi = np.zeros(nn, np.float32); N = np.zeros(nn, np.int32); W = np.zeros(nn, np.float64); P = np.zeros(nn, np.float32)
    a = C.c_int32(-1)
    table = np.full(nn, 1.0 / nn, np.float32)

    def _cb(user, b, pl, la, pol, val):         # the trivial evaluator: a uniform table and a constant value
        C.memmove(pol, table.ctypes.data, nn * 4)
        val[0] = 0.125
        return 0

    cb = az.Engine._EVAL_CB(_cb)

    def search():
        return L.az_search(e.h, 0, p(board), 2, n + 2, C.c_double(0.6), _capi._dp(noise), C.c_double(0.81), p(pi), C.byref(a), p(N), p(W), p(P))

    def callback():
        return L.az_search_callback(e.h, p(board), 2, n + 2, C.c_double(0.6), _capi._dp(noise), C.c_double(0.81), cb, None, p(pi),
                                    C.byref(a), p(N), p(W), p(P))

    row = dict(config=config, leg=leg, library="parent commit" if leg.startswith("parent") else "this build", board=n, simulations=S, slots=1)
    for what, fn, calls in (("az_search", search, cfg["calls"]), ("az_search_callback", callback, cfg["callback_calls"])):
        for _ in range(WARMUP):
            assert fn() == 0
        ms = np.zeros(calls)
        for i in range(calls):
            t = time.perf_counter()
            rc = fn()
            ms[i] = (time.perf_counter() - t) * 1e3
            assert rc == 0
        assert int(N.sum()) == S
        row[what] = dict(calls=calls, mean_ms=float(ms.mean()), median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)),
                         p90_ms=float(np.percentile(ms, 90)), action=int(a.value))
        if what == "az_search":
            row["az_search_persistent_kernel"] = e.persistent()
    e.close()
    if "net_eval" in cfg:
        e = az.Engine(n, k, S, 256)
        e.load_weights(synthetic_state_dict(n), 0)
        rs = np.random.RandomState(5)
        boards = (rs.random_sample((256, nn)) < 0.2).astype(np.uint8) * rs.randint(1, 3, (256, nn)).astype(np.uint8)
        players, lasts = np.ones(256, np.uint8), -np.ones(256, np.int16)
        for count, calls in cfg["net_eval"].items():
            ms = np.zeros(calls)
            for i in range(-WARMUP, calls):
                t = time.perf_counter()
                out = e.net_eval(boards[:count], players[:count], lasts[:count])
                if i >= 0:
                    ms[i] = (time.perf_counter() - t) * 1e3
            row[f"az_net_eval_{count}"] = dict(calls=calls, mean_ms=float(ms.mean()), median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)),
                                               p90_ms=float(np.percentile(ms, 90)), value_bits=int(np.float32(out[2][0]).view(np.uint32)))
        e.close()
    print(row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preset_search_path.json"))
    ap.add_argument("--parent-lib", required=True, help="libaz_engine.so built from the parent commit")
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--step-timeout", type=int, default=150)
    a = ap.parse_args()
    if a.leg:
        with open(a.out, "w") as f:
            json.dump(run_leg(a.config, a.leg), f)
        return 0
    result = {"configs": CONFIGS, "warmup_calls": WARMUP, "rows": []}
    rc = 0
    for config in CONFIGS:
        for leg in LEGS:
            part = a.out + f".{config}.{leg}.part"
            env = dict(os.environ)
            env.pop("AZ_ENGINE_LIB", None)
            if leg.startswith("parent"):
                env["AZ_ENGINE_LIB"] = os.path.abspath(a.parent_lib)
            rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--parent-lib", a.parent_lib,
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
    # per configuration and entry point: the parent's two medians, their spread, this build's two medians
    by = {(r["config"], r["leg"]): r for r in result["rows"]}
    summary = {}
    for config in CONFIGS:
        if not all((config, leg) in by for leg in LEGS):
            continue
        for what in ["az_search", "az_search_callback"] + [f"az_net_eval_{c}" for c in CONFIGS[config].get("net_eval", ())]:
            par = [by[(config, leg)][what]["median_ms"] for leg in ("parent_1", "parent_2")]
            new = [by[(config, leg)][what]["median_ms"] for leg in ("branch_1", "branch_2")]
            summary[f"{config}/{what}"] = dict(parent_median_ms=par, this_build_median_ms=new, parent_spread_ms=abs(par[0] - par[1]),
                                               slower_than_the_slower_parent_run_ms=max(new) - max(par))
    result["summary"] = summary
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(summary, indent=1), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
