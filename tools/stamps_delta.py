#!/usr/bin/env python3
"""Diagnostic: phase breakdown of k_trunk_delta<15> by conv3 tile count, from s_memtime stamps (csrc/az_delta.h, AZ_DSTAMP; build
with `make EXTRA=-DAZ_STAMPS` or a variant of it selected with AZ_ENGINE_LIB):
python tools/stamps_delta.py [readings] [out.json]
256 slots on one lane, the headline's 400 simulations; a reading is the stamps of a ply's last delta launch (simulation 400: deeper
leaves than the ply's mix), the readings of `readings` plies are pooled (default 40).  Figures are shader clock ticks per workgroup."""
import ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.weights import synthetic_state_dict

n, B = 15, 256
GAMES = 32 * B        # many more games than slots: a freed slot takes the next game, so every launch is of 256 live workgroups
readings = int(sys.argv[1]) if len(sys.argv) > 1 else 40
S = int(os.environ.get("AZ_STAMPS_SIMS", "400"))
e = az.Engine(n, 5, S, B, engines=1)
e.load_weights(synthetic_state_dict(n), 0)
e.selfplay_begin(GAMES, seed0=1)
t_end = time.time() + float(os.environ.get("AZ_STAMPS_WARM_SECONDS", "2.2"))     # >= 2 s of back-to-back launches before the first reading
while time.time() < t_end:
    e.selfplay_step(1)
rows = []
buf = np.zeros((B, 16), np.uint64)
for _ in range(readings):
    e.selfplay_step(1)
    rc = _capi.lib().az_debug_stamps(e.h, buf.ctypes.data_as(C.c_void_p), B)
    assert rc == 0, rc
    rows.append(buf.astype(np.int64))
e.close()
t = np.concatenate(rows)
# a workgroup that evaluated: five rising stamps up to conv2, a tile count, and as many chunk stamps as the count asks for
tiles = t[:, 13] & 0xFF          # (bits 8-15: the conv2 tile count)
ok = (np.diff(t[:, :5], axis=1) > 0).all(axis=1) & (tiles >= 1) & (tiles <= 15) & (t[:, 15] > t[:, 14]) & (t[:, 15] - t[:, 14] < 100000)
# k_trunk_delta stamps the rows of the launch's boards only, and k_fc's stamps follow them (az_kernels.hip): with fewer live
# slots than B (games ended and none left to start) the rows behind them hold k_fc's words and fail the conditions above
print("rows:", len(t), " entry only (no evaluation in this launch):", int(((t[:, 0] > 0) & (t[:, 1] == 0)).sum()),
      " not this kernel's stamps:", int(((t[:, 1] > 0) & ~ok).sum()))
t, tiles = t[ok], tiles[ok]
nchunk = np.count_nonzero(t[:, 5:13:2], axis=1)
print("workgroups with a complete set of stamps:", len(t), "of", B * readings)
names = ["lists", "windows", "conv1", "conv2", "conv3", "heads", "total"]    # since 5i "windows" is the issue of the loads, their wait is in conv1
table = {}
print(f"{'tiles':>5s} {'count':>6s} {'chunks':>6s} " + " ".join(f"{x:>8s}" for x in names))
for k in list(range(1, 16)) + [0]:
    sel = t[tiles == k] if k else t
    if not len(sel):
        continue
    nc = nchunk[tiles == k] if k else nchunk
    d = np.diff(sel[:, :5], axis=1).astype(np.float64)                 # lists, windows, conv1, conv2
    conv3, heads, prev = np.zeros(len(sel)), np.zeros(len(sel)), sel[:, 4].copy()
    for i in range(4):
        c, h = sel[:, 5 + 2 * i], sel[:, 6 + 2 * i]
        on = c > 0
        conv3[on] += (c - prev)[on]; heads[on] += (h - c)[on]
        prev = np.where(on, h, prev)
    cols = [d[:, 0], d[:, 1], d[:, 2], d[:, 3], conv3, heads, (prev - sel[:, 0]).astype(np.float64)]
    means = [float(np.mean(x)) for x in cols]
    label = str(k) if k else "all"
    table[label] = dict(count=int(len(sel)), chunks=float(np.mean(nc)), **{nm: round(m, 1) for nm, m in zip(names, means)})
    print(f"{label:>5s} {len(sel):6d} {np.mean(nc):6.2f} " + " ".join(f"{m:8.0f}" for m in means))
last = np.max(t[:, 5:13], axis=1)
ghz = (last - t[:, 0]) / (t[:, 15] - t[:, 14]) * 0.1
print(f"in-kernel clock: median {np.median(ghz):.3f} GHz; mean conv3 tiles {tiles.mean():.2f}")
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(dict(slots=B, sims=S, readings=readings, units="shader clock ticks per workgroup, mean", clock_ghz=round(float(np.median(ghz)), 3),
                       mean_tiles=round(float(tiles.mean()), 3), by_tiles=table), f, indent=1)
