#!/usr/bin/env python3
"""What the device RNG (az_set_rng: Philox tapes made by k_tape on the GPU instead of numpy streams made on host cores) costs and
buys, on one GPU, from the repo root:

    python tools/device_rng_gain.py [--out profiles/device_rng.json] [--parent-lib PATH] [--parts headline,modes,two_cores,kernel]

Every GPU step is a fresh process of its own under `timeout -k 10`; the first non-zero status ends the run (what was measured
before it is still written).
  headline   bench.py --gpus 1 with the mode never set, three runs of this build alternating with three of a library built from
             the parent commit (--parent-lib, selected with AZ_ENGINE_LIB): both medians and the parent's own spread.  Skipped
             without --parent-lib.
  modes      per configuration a numpy leg and a philox leg on this build: a warm-up and three steady-state episodes (games >>
             slots) through the step API, so that az_selfplay_begin is timed by itself.  Reported per leg: games/s, the wall time
             of az_selfplay_begin, tape_wait_seconds and the host CPU seconds of the process per episode (resource.getrusage,
             user + system, over begin .. end).
  two_cores  the 15x15 pair again with the child confined to two of the CPUs it may use (taskset) and AZ_TAPE_THREADS=1: one of
             eight ranks on the 16 CPUs a job gets.  It is one rank on one GPU; the 1 -> 8 GPU curve is NOT measured here.
  kernel     k_tape alone for 1024 games x all 225 plies at 15x15 (az_rng_philox_tape_device, three calls) under
             `rocprofv3 --kernel-trace --stats`: the kernel's own time.
There are no pass thresholds: these are measurements."""
import argparse
import csv
import glob
import json
import os
import resource
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "15x15": dict(n=15, k=5, S=400, slots=1024, games=2048),
    "9x9": dict(n=9, k=5, S=200, slots=4096, games=8192),
    "5x5": dict(n=5, k=4, S=100, slots=1024, games=8192),
}
RUNS = 3
BENCH = ["--gpus", "1", "--steps", "8", "--warmup", "1"]


def _stat(xs):
    med = statistics.median(xs)
    return {"runs": xs, "median": med, "spread": (max(xs) - min(xs)) / med if med else None}


def _cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def run_leg(config, mode):
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    c = CONFIGS[config]
    n, S, slots, G = c["n"], c["S"], c["slots"], c["games"]
    e = az.Engine(n, c["k"], S, slots, log_table=numpy_log_table(S))
    e.load_weights(synthetic_state_dict(n), 0)
    e.set_rng(mode)
    e.selfplay(slots, seed0=99, max_plies=3)             # warm-up: kernels loaded, buffers allocated, a graph captured
    gps, begin, wait, cpu, secs = [], [], [], [], []
    for r in range(RUNS):
        cpu0, t0 = _cpu_seconds(), time.perf_counter()
        e.selfplay_begin(G, seed0=1000 + 100000 * r)
        t1 = time.perf_counter()
        while e.selfplay_step(1 << 20)[0]:
            pass
        cnt = e.selfplay_end()
        t2 = time.perf_counter()
        secs.append(t2 - t0); gps.append(G / (t2 - t0)); begin.append(t1 - t0); wait.append(cnt["tape_wait_seconds"])
        cpu.append(_cpu_seconds() - cpu0)
        print(f"  {config} / {mode} run {r}: {t2 - t0:.2f} s, {gps[-1]:.1f} games/s, begin {begin[-1] * 1e3:.1f} ms, tape wait "
              f"{wait[-1]:.3f} s, host CPU {cpu[-1]:.2f} s, tape threads {cnt['tape_threads']}", flush=True)
    row = {"config": config, "mode": mode, "board": n, "simulations": S, "slots": slots, "lanes": e.lanes(), "games": G,
           "tape_threads": cnt["tape_threads"], "host_cpus": cnt["host_cpus"], "cpus_allowed": len(os.sched_getaffinity(0)),
           "seconds": secs, "games_per_sec": _stat(gps), "begin_seconds": _stat(begin), "tape_wait_seconds": _stat(wait),
           "host_cpu_seconds": _stat(cpu)}
    e.close()
    return row


def run_kernel():
    import alphazero_piskvorky_amd as az
    e = az.Engine(15, 5, 8, 2, synthetic=True)
    for r in range(RUNS):
        t0 = time.perf_counter()
        e.philox_tape_device(5000 + 2000 * r, 1024, 0.3, 0)
        print(f"  az_rng_philox_tape_device, 1024 games x 225 plies, with its buffers and the copy back: {time.perf_counter() - t0:.3f} s", flush=True)
    e.close()
    return {}


def child(args, timeout, env=None, prefix=()):
    cmd = ["timeout", "-k", "10", str(timeout)] + list(prefix) + [sys.executable] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_rng.json"))
    ap.add_argument("--parent-lib", help="libaz_engine.so built from the parent commit")
    ap.add_argument("--parts", default="headline,modes,two_cores,kernel")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--leg", choices=("numpy", "philox", "kernel"), help="run one leg in this process (what the parent does per child)")
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.leg:
        row = run_kernel() if a.leg == "kernel" else run_leg(a.config, a.leg)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    parts = a.parts.split(",")
    result = {"configs": CONFIGS, "runs_per_leg": RUNS,
              "not_measured": "the 1 -> 8 GPU curve; whether the host tape producer binds at eight ranks on the CPUs of one job"}
    if os.path.exists(a.out):                  # parts measured by an earlier call stay
        with open(a.out) as f:
            result.update({key: v for key, v in json.load(f).items() if key not in result and key != "failed"})
    me = os.path.abspath(__file__)

    def finish(rc):
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result), flush=True)
        return rc

    if "headline" in parts and a.parent_lib:
        vals = {"parent": [], "this": []}
        for r in range(RUNS):
            for who in ("parent", "this"):
                env = dict(os.environ)
                env.pop("AZ_ENGINE_LIB", None)
                if who == "parent":
                    env["AZ_ENGINE_LIB"] = os.path.abspath(a.parent_lib)
                p = child([os.path.join(ROOT, "bench.py")] + BENCH, a.step_timeout, env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                if p.returncode != 0 or not line:
                    result["failed"] = {"part": "headline", "who": who, "returncode": p.returncode}
                    return finish(p.returncode or 1)
                vals[who].append(json.loads(line[0])["value"])
                print(f"  bench.py {' '.join(BENCH)} / {who} run {r}: {vals[who][-1]:.0f} node-expansions/s", flush=True)
        result["headline"] = {"what": "bench.py " + " ".join(BENCH) + ", the mode never set, runs alternating parent / this build",
                              "unit": "node-expansions/s", "parent": _stat(vals["parent"]), "this": _stat(vals["this"]),
                              "this_over_parent": statistics.median(vals["this"]) / statistics.median(vals["parent"])}

    def pair(config, key, env, prefix, extra):
        for mode in ("numpy", "philox"):
            part = a.out + f".{key}.{config}.{mode}.part"
            p = child([me, "--leg", mode, "--config", config, "--out", part], a.step_timeout, env, prefix)
            sys.stdout.write(p.stdout)
            if p.returncode != 0:
                result["failed"] = {"part": key, "config": config, "mode": mode, "returncode": p.returncode}
                return p.returncode
            with open(part) as f:
                result.setdefault(key, []).append(dict(json.load(f), **extra))
            os.remove(part)
        return 0

    if "modes" in parts:
        result.pop("modes", None)
        for config in a.configs.split(","):
            rc = pair(config, "modes", None, (), {})
            if rc:
                return finish(rc)
    if "two_cores" in parts:
        result.pop("two_cores", None)
        cpus = sorted(os.sched_getaffinity(0))[:2]
        rc = pair("15x15", "two_cores", dict(os.environ, AZ_TAPE_THREADS="1"), ("taskset", "-c", ",".join(map(str, cpus))),
                  {"confined_to_cpus": cpus, "AZ_TAPE_THREADS": 1})
        if rc:
            return finish(rc)
    if "kernel" in parts and shutil.which("rocprofv3"):
        d = a.out + ".prof"
        shutil.rmtree(d, ignore_errors=True)
        part = a.out + ".kernel.part"
        p = child([me, "--leg", "kernel", "--out", part], a.step_timeout, dict(os.environ, TMPDIR="/tmp"),
                  ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tape", "--"))
        sys.stdout.write(p.stdout)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))
                if "k_tape" in r["Name"]]
        if p.returncode != 0 or not rows:
            result["failed"] = {"part": "kernel", "returncode": p.returncode, "rows": len(rows)}
            return finish(p.returncode or 1)
        result["kernel"] = {"what": "k_tape, 1024 games x 225 plies at 15x15 (26.0 M gamma draws, 208 MB written), alpha 0.3",
                            "calls": int(rows[0]["Calls"]), "average_ms": float(rows[0]["AverageNs"]) / 1e6,
                            "min_ms": float(rows[0].get("MinNs", "nan")) / 1e6, "max_ms": float(rows[0].get("MaxNs", "nan")) / 1e6}
        shutil.rmtree(d, ignore_errors=True)
        if os.path.exists(part):
            os.remove(part)
    by = {(r["config"], r["mode"]): r for r in result.get("modes", [])}
    result["philox_over_numpy"] = {config: {"games_per_sec": by[config, "philox"]["games_per_sec"]["median"] / by[config, "numpy"]["games_per_sec"]["median"],
                                            "host_cpu_seconds": by[config, "philox"]["host_cpu_seconds"]["median"] / by[config, "numpy"]["host_cpu_seconds"]["median"]}
                                   for config in CONFIGS if (config, "philox") in by and (config, "numpy") in by}
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
