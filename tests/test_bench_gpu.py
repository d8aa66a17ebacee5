"""bench.py's plain run and --dump-outputs on a small config: the plain line carries the headline and leaves the --full
measurements out; the dump is the engine's own records of the last timed ply, the same from run to run; --steps beyond
the length of the games still times that many plies (the plies left go to the next block of games)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.util import ROOT

ARGS = ["--gpus", "1", "--board", "5", "--win", "4", "--sims", "40", "--slots", "64", "--warmup", "1"]


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "bench.py"] + args, env=env, timeout=600, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _engine_last_ply(steps):
    """The bench's timed path restated on the engine: 64 games from seed 1_000_000, warm-up + the ply the --full run
    profiles, then `steps` plies; when every game has ended, the plies left on the next 64 games (seeds from 3_000_000)."""
    import alphazero_piskvorky_amd as az
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    e = az.Engine(5, 4, 40, 64)
    e.load_weights(synthetic_state_dict(5), 0)
    e.selfplay_begin(64, seed0=1_000_000)
    e.selfplay_step(2)
    left, ply0, blocks = steps, 2, 0
    while True:
        active, _ = e.selfplay_step(left)
        e.selfplay_end()
        nply, res = e.games()
        played = int(nply.max()) - ply0
        if active > 0 or played >= left:
            break
        left, ply0, blocks = left - played, 0, blocks + 1
        e.selfplay_begin(64, seed0=3_000_000 + (blocks - 1) * 64)
    rec = e.records()
    e.close()
    ply = ply0 + left - 1
    games = np.nonzero(nply > ply)[0]
    r = np.concatenate([[0], np.cumsum(nply)[:-1]])[games] + ply
    return blocks, {"game": games, "action": rec["actions"][r], "visits": rec["visits"][r], "pi": rec["pis"][r],
                    "board": rec["boards"][r], "plies_per_game": nply, "result_per_game": res}


@pytest.mark.parametrize("steps", [3, 40])
def test_plain_run_dumps_the_records_of_its_last_timed_ply(tmp_path, steps):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(ARGS + ["--steps", str(steps), "--dump-outputs", str(a)])
    assert line["metric"] == "mcts_node_expansions_per_sec" and line["value"] > 0 and line["higher_is_better"] is True
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    for key in ("roofline", "episode", "opt_in_emulated_trunks", "cpu_baseline"):
        assert line[key] is None, key
    _bench(ARGS + ["--steps", str(steps), "--dump-outputs", str(b)])
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "pi.npy" in names
    for f in names:
        x = np.load(a / f)
        assert x.dtype == np.float32 and np.array_equal(x, np.load(b / f)), f
    blocks, want = _engine_last_ply(steps)
    assert (blocks > 0) == (steps == 40) and len(want["game"]) > 0       # 5x5 games last at most 25 plies
    for name, v in want.items():
        assert np.array_equal(np.load(a / f"{name}.npy"), v.astype(np.float32)), name


def test_full_run_keeps_the_roofline_and_the_episode():
    line = _bench(ARGS + ["--steps", "2", "--full", "--no-cpu", "--steady-games", "0"])
    assert line["roofline"]["achieved"] > 0 and line["episode"]["games"] == 64 and line["self_play_games_per_sec"] > 0
