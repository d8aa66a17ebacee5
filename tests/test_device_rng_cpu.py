"""The AZ_RNG_PHILOX stream, the parts that need no GPU: Philox4x32-10 against the Random123 known answers, the host tape
(az_rng_philox_tape) against the contract restated in tests/philox.py bit for bit, the stream's independence of max_plies and
of the other games, az_rng_log against numpy, and the distributions against numpy's own samplers."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from tests import philox
from tests.util import ROOT

from alphazero_piskvorky_amd import _capi

NEW = ("az_set_rng", "az_get_rng", "az_rng_philox4x32", "az_rng_log", "az_rng_exp", "az_rng_philox_tape", "az_rng_philox_tape_device")
ALPHAS = (0.03, 0.3, 1.0, 2.5)              # a shape far below 1, the reference's, exactly 1, above 1
KINDS = ("dirichlet", "gumbel")
KAT = (                                      # Random123's kat_vectors for philox4x32_10: counter, key, output
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_symbols_are_exported_declared_and_listed():
    L = _capi.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        header = f.read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s
    assert L.az_set_rng(None, 1) == -1 and L.az_get_rng(None) == -1


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % x for x in _capi.philox4x32(counter, key)) == want
    assert " ".join("%08x" % x for x in philox.philox4x32(counter, key)) == want          # the restatement's own


def test_host_tape_refuses_bad_arguments():
    L = _capi.lib()
    buf = np.zeros(400, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.az_rng_philox_tape(1, 0, 0.3, 0, 0, p, p) == -1 and L.az_rng_philox_tape(1, 16, 0.3, 0, 0, p, p) == -1
    assert L.az_rng_philox_tape(1, 3, 0.3, 0, 2, p, p) == -1 and L.az_rng_philox_tape(1, 3, 0.3, 0, 0, p, None) == -1
    assert L.az_rng_philox_tape(1, 3, 0.0, 0, 0, p, p) == -1 and L.az_rng_philox_tape(1, 3, float("nan"), 0, 0, p, p) == -1
    assert not buf.any()
    assert L.az_rng_philox_tape(1, 3, 0.3, 0, 0, None, p) == 0 and buf[:9].tobytes() == _capi.philox_tape(1, 3)[1].tobytes()
    with pytest.raises(ValueError):
        _capi.check_rng("mt19937")
    assert _capi.check_rng(None) == "numpy" and _capi.check_rng("philox") == "philox"


# ---------------------------------------------------------------------------------------------------------------------
# the host tape is the contract, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n,max_plies", [(3, 0), (5, 0), (15, 3)])
def test_host_tape_is_the_restated_contract(n, max_plies, alpha, kind):
    for seed in (0, 1, 123456, 2 ** 32 + 9, 2 ** 64 - 1):          # both halves of the key, and the wrap of seed0 + g
        noise, u = _capi.philox_tape(seed, n, alpha, max_plies, kind)
        want_n, want_u = philox.tape(seed, n, alpha, max_plies, kind)
        assert noise.shape == want_n.shape and np.array_equal(_bits(noise), _bits(want_n)), (seed, "noise")
        assert np.array_equal(_bits(u), _bits(want_u)), (seed, "u")


def test_the_two_halves_of_the_seed_are_the_key():
    a, b = _capi.philox_tape(7, 3)[0], _capi.philox_tape(7 + 2 ** 32, 3)[0]
    assert not np.array_equal(a, b)                                 # numpy's tapes would be equal: RandomState takes 32 bits


@pytest.mark.parametrize("kind", KINDS)
def test_prefix_and_independence(kind):
    n, nn = 5, 25
    full_n, full_u = _capi.philox_tape(42, n, 0.3, 0, kind)
    cut_n, cut_u = _capi.philox_tape(42, n, 0.3, 3, kind)
    assert len(cut_u) == 3 and len(cut_n) == nn + (nn - 1) + (nn - 2)
    assert np.array_equal(_bits(cut_n), _bits(full_n[:len(cut_n)])) and np.array_equal(_bits(cut_u), _bits(full_u[:3]))
    # game g of a run is seed0 + g whatever else is generated: in another order, alone, as game 0 of a later shard
    again = [_capi.philox_tape(40 + g, n, 0.3, 0, kind) for g in (5, 2, 0)]
    assert np.array_equal(_bits(again[1][0]), _bits(full_n)) and np.array_equal(_bits(again[1][1]), _bits(full_u))
    assert not np.array_equal(again[0][0], full_n)


# ---------------------------------------------------------------------------------------------------------------------
# az_rng_log against numpy
# ---------------------------------------------------------------------------------------------------------------------
LOG_MEASURED_ULP = 1.0       # the largest |az_rng_log - np.log| over the sweep below, in ulps of np.log's value, as measured
LOG_BOUND_ULP = 2.0          # asserted: twice that


def test_log_against_numpy():
    rs = np.random.RandomState(20261021)
    powers = 2.0 ** np.arange(-1074, 1024, dtype=np.float64)                      # every power of two from the smallest subnormal up
    unit = rs.random_sample(100000)
    unit = unit[unit > 0]
    near_one = 1.0 + (rs.random_sample(10000) - 0.5) * 2.0 ** -rs.randint(1, 53, 10000).astype(np.float64)
    worst = 0.0
    for xs in (powers, unit, near_one):
        got = np.array([_capi.rng_log(x) for x in xs])
        want = np.log(xs)
        zero = want == 0
        assert np.array_equal(got[zero], want[zero])                              # log(1) is +0 exactly
        err = np.abs(got[~zero] - want[~zero]) / np.spacing(np.abs(want[~zero]))
        worst = max(worst, float(err.max()))
    print("az_rng_log: largest error %.3f ulp (bound %.1f)" % (worst, LOG_BOUND_ULP))
    assert worst <= LOG_BOUND_ULP
    assert _capi.rng_log(0.0) == -math.inf and _capi.rng_log(-0.0) == -math.inf and _capi.rng_log(math.inf) == math.inf
    assert math.isnan(_capi.rng_log(-1.0)) and math.isnan(_capi.rng_log(math.nan))
    assert _capi.rng_exp(-math.inf) == 0.0 and _capi.rng_exp(0.0) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# distributions (deterministic: fixed seeds on both sides)
# ---------------------------------------------------------------------------------------------------------------------
GAMES = 2000
KS_ALPHA = 1e-6


def ks_critical(n, m):
    """two-sample Kolmogorov-Smirnov critical value at significance KS_ALPHA: sqrt(-ln(alpha / 2) / 2) * sqrt((n + m) / (n m))"""
    return math.sqrt(-math.log(KS_ALPHA / 2.0) / 2.0) * math.sqrt((n + m) / (n * m))


def ks_two_sample(a, b):
    a, b = np.sort(a), np.sort(b)
    both = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, both, side="right") / len(a) - np.searchsorted(b, both, side="right") / len(b)).max())


def ks_uniform(a):
    a = np.sort(a)
    i = np.arange(len(a))
    return float(max(((i + 1) / len(a) - a).max(), (a - i / len(a)).max()))


@functools.lru_cache(maxsize=None)
def _ply0(kind):
    rows = [_capi.philox_tape(9000 + g, 5, 0.3, 1, kind) for g in range(GAMES)]
    return np.array([r[0] for r in rows]), np.array([r[1][0] for r in rows])


def _numpy_dirichlet(seed):
    return np.random.RandomState(seed).dirichlet([0.3] * 25, size=GAMES)


def test_ks_critical_value():
    assert abs(ks_critical(GAMES, GAMES) - 0.085) < 5e-4


def test_dirichlet_rows_are_distributions():
    noise, _ = _ply0("dirichlet")
    assert noise.shape == (GAMES, 25) and np.isfinite(noise).all() and (noise >= 0).all()
    assert np.abs(noise.sum(axis=1) - 1.0).max() <= 2.0 ** -50
    for alpha in ALPHAS:
        t = _capi.philox_tape(5, 5, alpha)[0]
        assert np.isfinite(t).all() and (t >= 0).all()
        off = 0
        for m in range(25):
            assert abs(t[off:off + 25 - m].sum() - 1.0) <= 2.0 ** -50
            off += 25 - m


@pytest.mark.parametrize("rank", [0, 24])
def test_dirichlet_marginals_against_numpy(rank):
    noise, _ = _ply0("dirichlet")
    crit = ks_critical(GAMES, GAMES)
    a, b = _numpy_dirichlet(1)[:, rank], _numpy_dirichlet(2)[:, rank]
    assert ks_two_sample(a, b) < crit                   # the yardstick: numpy against numpy under another seed
    assert ks_two_sample(noise[:, rank], a) < crit


def test_move_uniforms_against_uniform():
    _, u = _ply0("dirichlet")
    assert ((u >= 0) & (u < 1)).all()
    crit = ks_critical(GAMES, GAMES)
    a, b = np.random.RandomState(1).random_sample(GAMES), np.random.RandomState(2).random_sample(GAMES)
    assert ks_two_sample(a, b) < crit
    assert ks_two_sample(u, a) < crit
    assert ks_uniform(u) < math.sqrt(-math.log(KS_ALPHA / 2.0) / (2.0 * GAMES))     # one sample against U(0, 1) itself


def test_gumbel_kind_against_numpy():
    noise, u = _ply0("gumbel")
    assert np.isfinite(noise).all() and (noise < 0).any() and (noise > 1).any()
    assert np.array_equal(_bits(u), _bits(_ply0("dirichlet")[1]))                 # the move uniform does not depend on the kind
    crit = ks_critical(GAMES, GAMES)
    a, b = np.random.RandomState(1).gumbel(size=GAMES), np.random.RandomState(2).gumbel(size=GAMES)
    assert ks_two_sample(a, b) < crit
    for rank in (0, 24):
        assert ks_two_sample(noise[:, rank], a) < crit


# ---------------------------------------------------------------------------------------------------------------------
# the seams
# ---------------------------------------------------------------------------------------------------------------------
class _Engine:
    def __init__(self):
        self.mode, self.calls = "numpy", []

    def rng(self):
        return self.mode

    def set_rng(self, mode):
        self.calls.append(mode)
        self.mode = mode


def test_seams_take_and_check_the_option():
    from alphazero_piskvorky_amd.evaluator import ModelEvaluator
    from alphazero_piskvorky_amd.options import apply_options
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    assert SelfPlayManager(None, "cuda:0", rng="philox").rng == "philox" and SelfPlayManager(None, "cuda:0").rng == "numpy"
    assert ModelEvaluator(rng="philox").rng == "philox" and ModelEvaluator().rng == "numpy"
    for seam in (lambda: SelfPlayManager(None, "cuda:0", rng="pcg"), lambda: ModelEvaluator(rng="pcg")):
        with pytest.raises(ValueError):
            seam()
    # a cached engine is brought to the mode and back; the same mode again calls nothing
    off = dict(win_rule="freestyle", start_positions=None, first=0, resign=None, playout_cap=None, forced_playouts=None, gumbel=None,
               solver=False, threat_search=None)

    class Fake(_Engine):
        win_rule = lambda self: "freestyle"
        start_positions = lambda self: 0
        resign = lambda self: {"threshold": 0.0}
        playout_cap = lambda self: {"fast_sims": 0}
        forced_playouts = lambda self: {"k": 0.0}
        gumbel = lambda self: {"m": 0}
        threat_search = lambda self: (0, 0)
        solver = lambda self: False
    e = Fake()
    apply_options(e, **off, rng="philox")
    apply_options(e, **off, rng="philox")
    apply_options(e, **off)
    assert e.calls == ["philox"] and e.mode == "philox"
    apply_options(e, **off, rng="numpy")
    assert e.calls == ["philox", "numpy"]
