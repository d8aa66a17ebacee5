#!/usr/bin/env python3
"""Delta evaluation at the headline configuration, in one process: milliseconds per ply with the switch off
and on, over a sweep of the fallback threshold, with the path counters and the conv3 tile histogram of the timed plies.
python tools/delta_gain.py [plies per setting] [thresholds, comma separated]
Every setting plays the same plies (same seed); settings alternate `rounds` times so that drift shows."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.weights import synthetic_state_dict

n, k, S, B = 15, 5, 400, 1024
plies = int(sys.argv[1]) if len(sys.argv) > 1 else 6
thresholds = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "4,8,10,12,14,15").split(",")]
rounds = 2
e = az.Engine(n, k, S, B)
e.load_weights(synthetic_state_dict(n), 0)
settings = [("off", None)] + [("on", t) for t in thresholds]
out = {f"{name}{'' if t is None else t}": {"ms_per_ply": []} for name, t in settings}
for r in range(rounds):
    for name, t in settings:
        key = f"{name}{'' if t is None else t}"
        e.set_delta_eval(name == "on")
        if t is not None:
            e.delta_max_tiles(t)
        e.selfplay_begin(B, seed0=1)
        e.selfplay_step(1)                                   # warm-up ply (graph capture)
        t0 = time.perf_counter()
        _, c = e.selfplay_step(plies)
        dt = time.perf_counter() - t0
        st = e.delta_stats(by_tiles=True)
        e.selfplay_end()
        out[key]["ms_per_ply"].append(round(dt / plies * 1e3, 3))
        evals = c["expansions"] + c["root_evals"] - c["cache_hits"]
        out[key].update(evaluations=evals, mean_select_depth=round(c["depth_sum"] / max(c["simulations"], 1), 4), **st)
        if st["delta"]:
            out[key]["tiles_per_delta_evaluation"] = round(st["tiles"] / st["delta"], 3)
        print(key, out[key]["ms_per_ply"], flush=True)
e.close()
print(json.dumps(out))
