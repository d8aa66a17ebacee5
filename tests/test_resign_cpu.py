"""Resignation and the search value per record, the parts that need no GPU: the C ABI declares and exports what the binding
calls, the exemption rule of the header against a numpy restatement, the argument checks of the Python layer and the
statistics a threshold is calibrated from."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.util import ROOT

from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.evaluator import ModelEvaluator
from alphazero_piskvorky_amd.self_play import SelfPlayManager, check_resign, resign_stats

NEW = ("az_set_resign", "az_get_resign", "az_selfplay_values", "az_selfplay_pack_values", "az_selfplay_resign_info",
       "az_resign_mix", "az_resign_exempt")


def np_mix(x):
    """murmur3's 32-bit finaliser as include/az_engine.h writes it out, on a uint32 array"""
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B); x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35); x ^= x >> np.uint32(16)
    return x


def np_exempt(seed0, games, permille):
    """exempt[g] for the games seed0 .. seed0 + games - 1: mix(low 32 bits of seed0 + g) % 1000 < permille"""
    keys = ((int(seed0) + np.arange(games, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return (np_mix(keys) % np.uint32(1000)).astype(np.int64) < permille


def test_header_declares_and_library_exports_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    for decl in ("int az_set_resign(az_engine *e, double threshold, int min_ply, int playout_permille);",
                 "int az_get_resign(const az_engine *e, double *threshold, int *min_ply, int *playout_permille);",
                 "int az_selfplay_values(az_engine *e, float *values);",
                 "int az_selfplay_pack_values(az_engine *e, float *values_dev);",
                 "int az_selfplay_resign_info(az_engine *e, int32_t *cross_ply, uint8_t *exempt);",
                 "uint32_t az_resign_mix(uint32_t x);", "int az_resign_exempt(uint32_t key, int playout_permille);"):
        assert decl in text, decl
    assert re.search(r"x \^= x >> 16;\s+x \*= 0x85EBCA6B;\s+x \^= x >> 13;\s+x \*= 0xC2B2AE35;\s+x \^= x >> 16;", text)
    L = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    # the counters and the configuration keep their layout: the setting is an engine option
    assert len(_capi.az_counters._fields_) == 21 and len(_capi.az_config._fields_) == 12


def test_null_engine_is_an_error():
    L = _capi.lib()
    assert L.az_set_resign(None, 0.5, 0, 0) == -1
    assert L.az_get_resign(None, None, None, None) == -1
    assert L.az_selfplay_values(None, None) == -6 and L.az_selfplay_pack_values(None, None) == -6
    assert L.az_selfplay_resign_info(None, None, None) == -6


def test_mix_and_exemption_equal_the_numpy_restatement():
    rs = np.random.RandomState(11)
    keys = np.concatenate([np.arange(2048, dtype=np.uint32), np.array([0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32),
                           rs.randint(0, 2 ** 32, 3000, dtype=np.uint64).astype(np.uint32)])
    want = np_mix(keys)
    assert want[0] == 0 and len(set(want.tolist())) == len(set(keys.tolist()))        # fmix32 is a bijection with mix(0) = 0
    assert [_capi.resign_mix(int(k)) for k in keys] == want.tolist()
    for permille in (0, 1, 100, 500, 999, 1000):
        got = np.array([_capi.resign_exempt(int(k), permille) for k in keys])
        assert np.array_equal(got, (want % np.uint32(1000)).astype(np.int64) < permille), permille
    assert not any(_capi.resign_exempt(int(k), 0) for k in keys[:64]) and all(_capi.resign_exempt(int(k), 1000) for k in keys[:64])
    # the key is the low 32 bits of seed0 + g
    assert _capi.resign_exempt(2 ** 32 + 77, 300) == _capi.resign_exempt(77, 300)
    assert np.array_equal(np_exempt(2 ** 32 - 3, 8, 400), [_capi.resign_exempt((2 ** 32 - 3 + g) & 0xFFFFFFFF, 400) for g in range(8)])
    share = np_exempt(5000, 4000, 100).mean()
    assert 0.07 < share < 0.13                       # a tenth of the games, 4000 draws: 0.1 +- 6 sigma (sigma = 0.0047)


def test_python_argument_validation():
    assert _capi.resign_permille(0.0) == 0 and _capi.resign_permille(1.0) == 1000 and _capi.resign_permille(0.1) == 100
    assert _capi.resign_permille(0.0004) == 0 and _capi.resign_permille(0.0006) == 1
    for bad in (-0.1, 1.001, float("nan")):
        with pytest.raises(ValueError, match="playout"):
            _capi.resign_permille(bad)
    e = object.__new__(_capi.Engine)          # the checks come before the library is called: no engine needed
    e.h = ctypes.c_void_p()
    for kw in (dict(threshold=-0.1), dict(threshold=1.5), dict(threshold=float("nan"))):
        with pytest.raises(ValueError, match="threshold"):
            e.set_resign(**kw)
    with pytest.raises(ValueError, match="min_ply"):
        e.set_resign(0.5, min_ply=-1)
    with pytest.raises(ValueError, match="playout"):
        e.set_resign(0.5, playout=2)
    # the seams
    assert check_resign(None) is None
    assert check_resign({"threshold": 0.9}) == {"threshold": 0.9, "min_ply": 0, "playout": 0.0}
    assert check_resign({"threshold": 1, "min_ply": 4, "playout": 0.1}) == {"threshold": 1.0, "min_ply": 4, "playout": 0.1}
    for bad in ({}, {"min_ply": 3}, {"threshold": 0.0}, {"threshold": 1.1}, {"threshold": 0.5, "min_ply": -1},
                {"threshold": 0.5, "playout": 1.5}, {"threshold": 0.5, "share": 0.1}):
        with pytest.raises(ValueError):
            check_resign(bad)
        with pytest.raises(ValueError):
            SelfPlayManager(controller=None, device="cuda:0", resign=bad)
        with pytest.raises(ValueError):
            ModelEvaluator(device="cuda:0", resign=bad)
    m = SelfPlayManager(controller=None, device="cuda:0", resign={"threshold": 0.8, "playout": 0.1})
    assert m.resign == {"threshold": 0.8, "min_ply": 0, "playout": 0.1} and m.last_resign_stats is None
    assert SelfPlayManager(None, "cuda:0").resign is None and ModelEvaluator(device="cuda:0").resign is None
    assert ModelEvaluator(device="cuda:0", resign={"threshold": 0.7}).resign["threshold"] == 0.7


def test_resign_stats_on_hand_made_games():
    #            0: never crossed   1: resigned (X crossed, O won)   2: exempt, crossed, lost anyway
    #            3: exempt, crossed, WON (false positive)   4: exempt, crossed, draw (false positive)   5: exempt, never crossed
    #            6: crossed on the ply whose move won the game (natural end: not a resignation)   7: resigned (O crossed)
    result = [1, 2, 1, 1, 3, 2, 2, 1]
    cross = [-1, 6, 9, 4, 10, -1, 7, 5]
    exempt = [0, 0, 1, 1, 1, 1, 0, 0]
    movers = [0, 1, 2, 1, 1, 0, 2, 2]
    s = resign_stats(result, cross, exempt, movers)
    assert s == {"games": 8, "resigned": 2, "exempt": 4, "exempt_crossed": 3, "false_positives": 2,
                 "false_positive_rate": 2 / 3}
    s = resign_stats([1, 2], [-1, -1], [False, True], [0, 0])
    assert s["resigned"] == 0 and s["exempt"] == 1 and s["exempt_crossed"] == 0 and s["false_positive_rate"] is None
    assert resign_stats([], [], [], [])["games"] == 0
    with pytest.raises(ValueError):
        resign_stats([1, 2], [3], [0, 0], [1, 1])
    with pytest.raises(ValueError):
        resign_stats([1], [3], [0], [0])             # a crossing ply has a mover
