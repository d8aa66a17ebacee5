"""AZ_RNG_PHILOX on the GPU.  The tape kernel against the host function that runs the same sampler, as uint64; then whole
episodes: an engine in Philox mode must play, byte for byte, what an engine in numpy mode plays when it is handed the host
function's tapes as explicit noise_tape / u_tape -- under every launch path and option that reads the tapes.  No consumer kernel
changed, so this is exact and needs no oracle of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_device_rng_cpu import ALPHAS, KINDS

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.weights import synthetic_state_dict

REC_KEYS = ("boards", "movers", "lasts", "visits", "pis", "actions", "z")
SLOTS, GAMES = 3, 7          # fewer slots than games: slots are refilled


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _host_tapes(seed0, games, n, alpha, max_plies, kind):
    """[games, tape length] and [games, n*n] as the engine takes explicit tapes"""
    rows = [_capi.philox_tape(seed0 + g, n, alpha, max_plies, kind) for g in range(games)]
    u = np.zeros((games, n * n), np.float64)
    for g, r in enumerate(rows):
        u[g, :len(r[1])] = r[1]
    return np.stack([r[0] for r in rows]), u


# ---------------------------------------------------------------------------------------------------------------------
# the kernel on its own
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tape_engines():
    es = {n: az.Engine(n, min(n, 5), 4, 2, synthetic=True, log_table=orc.numpy_log_table(4)) for n in (3, 5, 9, 15)}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n", [3, 5, 9, 15])
def test_kernel_equals_the_host_sampler(tape_engines, n, alpha, kind):
    seed0, games = 2 ** 32 - 2, 5                       # the low half of the key wraps inside the run
    noise, u = tape_engines[n].philox_tape_device(seed0, games, alpha, 0, kind)
    want_n, want_u = _host_tapes(seed0, games, n, alpha, 0, kind)
    assert noise.shape == want_n.shape and np.array_equal(_bits(noise), _bits(want_n))
    assert np.array_equal(_bits(u), _bits(want_u))


def test_kernel_cut_tape_and_arguments(tape_engines):
    e = tape_engines[5]
    noise, u = e.philox_tape_device(11, 3, 0.3, 4)
    want_n, want_u = _host_tapes(11, 3, 5, 0.3, 4, "dirichlet")
    assert noise.shape == (3, 25 + 24 + 23 + 22) and np.array_equal(_bits(noise), _bits(want_n))
    assert u.shape == (3, 4) and np.array_equal(_bits(u), _bits(want_u[:, :4]))
    assert e.philox_tape_device(11, 0)[0].shape == (0, 325)
    for bad in (dict(alpha=0.0), dict(alpha=float("nan"))):
        with pytest.raises(az.AzError, match=r"\(-1\)"):
            e.philox_tape_device(11, 2, **bad)
    L = _capi.lib()
    buf = np.zeros(2 * 325, np.float64)
    assert L.az_rng_philox_tape_device(e.h, 11, 2, 0.3, 0, 2, _capi._p(buf), _capi._p(buf)) == -1 and not buf.any()
    assert L.az_rng_philox_tape_device(e.h, 11, 2, 0.3, 0, 0, _capi._p(buf), None) == -1 and not buf.any()


# ---------------------------------------------------------------------------------------------------------------------
# episodes
# ---------------------------------------------------------------------------------------------------------------------
def _engine(n, k, S, slots=SLOTS, lanes=0, synthetic=False):
    e = az.Engine(n, k, S, slots, synthetic=synthetic, engines=lanes, log_table=orc.numpy_log_table(S), model="plain")
    if not synthetic:
        e.load_weights(synthetic_state_dict(n), 0)
    return e


def _result(e, c):
    out = dict(e.records(), values=e.values(), sims=e.sims())
    out["nply"], out["result"] = e.games()
    out["counters"] = {k: c[k] for k in ("games", "plies", "records", "simulations", "expansions", "root_evals", "terminal_hits")}
    return out


def _assert_same(a, b, what):
    for key in REC_KEYS + ("sims", "nply", "result"):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), f"{what}: {key}"
    assert np.array_equal(a["values"].view(np.uint32), b["values"].view(np.uint32)), f"{what}: values"
    assert np.array_equal(a["pis"].view(np.uint32), b["pis"].view(np.uint32)), f"{what}: pis as bits"
    assert a["counters"] == b["counters"], f"{what}: counters"


def _pair(n, k, S, seed0, cut=0, setup=None, lanes=0, games=GAMES, kind="dirichlet", what=""):
    """the episode of a fresh engine in Philox mode and that of a fresh engine in numpy mode on the host function's tapes"""
    got = want = None
    for mode in ("philox", "numpy"):
        e = _engine(n, k, S, lanes=lanes)
        try:
            if setup:
                setup(e)
            if mode == "philox":
                e.set_rng("philox")
                assert e.rng() == "philox"
                c = e.selfplay(games, seed0=seed0, max_plies=cut)
                assert c["tape_threads"] == 0 and c["tape_wait_seconds"] == 0.0
                got = _result(e, c)
            else:
                assert e.rng() == "numpy"
                noise, u = _host_tapes(seed0, games, n, 0.3, cut, kind)
                want = _result(e, e.selfplay(games, seed0=seed0, max_plies=cut, noise_tape=noise, u_tape=u))
        finally:
            e.close()
    _assert_same(got, want, what or f"{n}x{n}")
    assert got["nply"].sum() > 0 and got["counters"]["games"] == games
    return got


@pytest.mark.parametrize("persist", ["1", "0"])
def test_episode_5x5(monkeypatch, persist):
    monkeypatch.setenv("AZ_PERSIST", persist)
    _pair(5, 4, 16, 7100, what=f"5x5 AZ_PERSIST={persist}")


def test_episode_9x9():
    _pair(9, 5, 12, 7200)


def test_episode_15x15_delta_eval():
    def setup(e):
        e.set_delta_eval(True)
    got = _pair(15, 5, 8, 7300, cut=6, setup=setup)
    assert got["nply"].tolist() == [6] * GAMES


def _start_positions(e):
    """three 5x5 positions of 2, 3 and 4 stones: the games run `ahead` of the episode's ply count"""
    boards = np.zeros((3, 25), np.uint8)
    boards[0, [12, 7]] = (1, 2)
    boards[1, [0, 24, 13]] = (1, 2, 1)
    boards[2, [6, 8, 16, 18]] = (1, 2, 1, 2)
    e.set_start_positions(boards, [1, 2, 1], [7, 13, 18])


OPTIONS = {
    "gumbel root": (lambda e: e.set_gumbel(4), "gumbel", 0),
    "playout cap": (lambda e: e.set_playout_cap(4, 0.5), "dirichlet", 0),
    "forced playouts": (lambda e: e.set_forced_playouts(2.0), "dirichlet", 0),
    "start positions": (_start_positions, "dirichlet", 0),
    "virtual loss 4": (lambda e: e.set_virtual_loss(4), "dirichlet", 0),
    "two lanes": (None, "dirichlet", 2),
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_episode_5x5_under_option(name):
    setup, kind, lanes = OPTIONS[name]
    _pair(5, 4, 16, 7400, setup=setup, lanes=lanes, kind=kind, what=name)


def test_episode_5x5_without_tape_streaming(monkeypatch):
    monkeypatch.setenv("AZ_TAPE_STREAM", "0")
    _pair(5, 4, 16, 7500, what="AZ_TAPE_STREAM=0")


def test_arena_5x5():
    res = {}
    for mode in ("philox", "numpy"):
        e = _engine(5, 4, 16, slots=SLOTS)
        try:
            e.load_weights(synthetic_state_dict(5), 1)
            if mode == "philox":
                e.set_rng("philox")
                r = e.arena(6, seed0=7600)
                assert e.counters()["tape_threads"] == 0
            else:
                r = e.arena(6, seed0=7600, u_tape=_host_tapes(7600, 6, 5, 0.3, 0, "dirichlet")[1])
            res[mode] = dict(r, records=e.records(), games=e.games())
        finally:
            e.close()
    a, b = res["philox"], res["numpy"]
    for key in ("results", "actions", "nply"):
        assert np.array_equal(a[key], b[key]), key
    for key in REC_KEYS:
        assert np.array_equal(a["records"][key], b["records"][key]), key
    assert (a["wins"], a["losses"], a["draws"]) == (b["wins"], b["losses"], b["draws"]) and a["total"] == 6


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
def test_switching_modes_on_one_engine():
    n, k, S, seed0 = 5, 4, 16, 7700

    def fresh(mode):
        e = _engine(n, k, S, synthetic=True)
        try:
            e.set_rng(mode)
            return _result(e, e.selfplay(GAMES, seed0=seed0))
        finally:
            e.close()
    want = {mode: fresh(mode) for mode in ("philox", "numpy")}
    assert not np.array_equal(want["philox"]["actions"], want["numpy"]["actions"])
    e = _engine(n, k, S, synthetic=True)
    try:
        for step, mode in enumerate(("philox", "numpy", "philox")):
            e.set_rng(mode)
            assert e.rng() == mode
            c = e.selfplay(GAMES, seed0=seed0)
            assert (c["tape_threads"] == 0) == (mode == "philox")
            _assert_same(_result(e, c), want[mode], f"step {step}: {mode}")
    finally:
        e.close()
    # numpy mode is still the oracle's game, as tests/test_engine_gpu.py compares it
    o = orc.Oracle(n, k, S, synthetic=True)
    got, off = want["numpy"], 0
    for g in range(GAMES):
        noise, us = orc.selfplay_tape(seed0 + g, n)
        r = o.selfplay_game(None, noise, us, maxply=n * n)
        sl = slice(off, off + int(got["nply"][g]))
        assert np.array_equal(got["pis"][sl], r["pis"]) and np.array_equal(got["z"][sl], r["z"]) and np.array_equal(got["lasts"][sl], r["lasts"])
        off = sl.stop


def test_set_rng_is_refused_while_an_episode_is_open():
    e = _engine(5, 4, 8, synthetic=True)
    try:
        with pytest.raises(ValueError):
            e.set_rng("mt19937")
        assert _capi.lib().az_set_rng(e.h, 2) == -1 and e.rng() == "numpy"
        e.selfplay_begin(4, seed0=7800)
        with pytest.raises(az.AzError, match=r"\(-6\)"):
            e.set_rng("philox")
        with pytest.raises(az.AzError, match=r"\(-6\)"):
            e.philox_tape_device(1, 1)
        assert e.rng() == "numpy"
        while e.selfplay_step(4)[0]:
            pass
        c = e.selfplay_end()
        want = _engine(5, 4, 8, synthetic=True)
        try:
            _assert_same(_result(e, c), _result(want, want.selfplay(4, seed0=7800)), "the refused call changed nothing")
        finally:
            want.close()
        e.set_rng("philox")
        e.selfplay_begin(4, seed0=7800)
        active, prog = e.selfplay_step(1)
        assert prog["tape_threads"] == 0 and prog["tape_wait_seconds"] == 0.0
        with pytest.raises(az.AzError, match=r"\(-6\)"):
            e.set_rng("numpy")
        assert e.rng() == "philox"
        while e.selfplay_step(4)[0]:
            pass
        assert e.selfplay_end()["tape_threads"] == 0
    finally:
        e.close()
