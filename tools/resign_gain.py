#!/usr/bin/env python3
"""Diagnostic: what opt-in resignation (az_set_resign) saves and what it costs.  5x5 with the trained checkpoint fixture at
100 simulations, 1024 games on 256 slots (freed slots are refilled: the steady state), at a few thresholds with a tenth of
the games playing on: games/s, mean plies per game and the false-positive rate of the threshold, each against resignation
off in the same process.  15x15 with random-init weights is recorded as what it is: search values near 0, nothing resigns,
so it shows what the feature costs when it is idle.  Writes $AZ_OUT/resign.json (default out/); copy what is to be judged
into profiles/."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.self_play import resign_stats
from alphazero_piskvorky_amd.weights import synthetic_state_dict
from tests.util import weights_from_fixture

PLAYOUT, SEED0 = 0.1, 1_000_000
rows = []
for name, n, k, S, G, slots, sd, thresholds in (
        ("5x5 trained checkpoint", 5, 4, 100, 1024, 256, weights_from_fixture(5, "ckpt_saved"), (0.0, 0.95, 0.9, 0.8, 0.0)),
        ("15x15 random-init", 15, 5, 400, 1024, 1024, synthetic_state_dict(15), (0.0, 0.9, 0.0))):
    eng = az.Engine(n, k, S, slots)
    eng.load_weights(sd, 0)
    eng.selfplay(min(G, slots), seed0=1, max_plies=2)            # warm-up: library, graphs, allocations
    for thr in thresholds:                                     # off first and last: the spread of the process is on the page
        eng.set_resign(thr, playout=PLAYOUT if thr else 0.0)
        t0 = time.perf_counter()
        c = eng.selfplay(G, seed0=SEED0)
        dt = time.perf_counter() - t0
        nply, result = eng.games()
        cross, exempt = eng.resign_info()
        values = eng.values()
        st = resign_stats(result, cross, exempt, 1 + (np.maximum(cross, 0) & 1))     # X moves first from the empty board
        row = dict(config=name, board=n, simulations=S, slots=slots, threshold=thr, playout=PLAYOUT if thr else 0.0,
                   seconds=dt, games_per_second=G / dt, plies=int(c["plies"]), mean_plies_per_game=float(nply.mean()),
                   simulations_run=int(c["simulations"]), value_min=float(values.min()), value_mean=float(values.mean()), **st)
        rows.append(row)
        fp = st["false_positive_rate"]
        print(f"{name}, threshold {thr}: {dt:.2f} s, {G / dt:.1f} games/s, {nply.mean():.2f} plies per game, resigned {st['resigned']}, "
              f"played out {st['exempt']} (crossed {st['exempt_crossed']}, false positives {st['false_positives']}: "
              f"{'n/a' if fp is None else format(fp, '.1%')}), values min {values.min():.3f} mean {values.mean():.3f}", flush=True)
    eng.close()
out = os.environ.get("AZ_OUT", "out")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "resign.json"), "w") as f:
    json.dump(rows, f, indent=1)
print("wrote", os.path.join(out, "resign.json"))
