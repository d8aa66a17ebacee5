"""Playout cap randomisation, the parts that need no GPU: the C ABI declares and exports what the binding calls, the fullness
rule of the header against a numpy restatement, the argument checks of the Python layer, and a check of the inputs the GPU
tests are built on (both kinds of ply must be present where a test claims to mix them)."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_resign_cpu import np_mix
from tests.util import ROOT

from alphazero_piskvorky_amd import _capi
from alphazero_piskvorky_amd.self_play import SelfPlayManager, check_playout_cap, playout_cap_full_plies, playout_cap_stats

NEW = ("az_set_playout_cap", "az_get_playout_cap", "az_playout_cap_full", "az_selfplay_sims", "az_selfplay_export_count")


def np_full(key, ply, permille):
    """the header's rule on arrays: mix(key ^ mix(ply + 0x9E3779B9)) % 1000 < permille, key = low 32 bits of seed0 + g"""
    key = (np.asarray(key, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    inner = np_mix((np.asarray(ply, np.uint64) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF))
    return (np_mix(key ^ inner) % np.uint32(1000)).astype(np.int64) < np.asarray(permille, np.int64)


def full_table(seed0, games, plies, permille):
    """[games][plies] bool: ply p of game seed0 + g is FULL"""
    g, p = np.meshgrid(np.arange(games, dtype=np.uint64), np.arange(plies, dtype=np.uint64), indexing="ij")
    return np_full(np.uint64(seed0) + g, p, permille)


def test_header_declares_and_library_exports_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    for decl in ("int az_set_playout_cap(az_engine *e, int fast_sims, int full_permille, int export_full_only);",
                 "int az_get_playout_cap(const az_engine *e, int *fast_sims, int *full_permille, int *export_full_only);",
                 "int az_playout_cap_full(uint32_t key, int ply, int full_permille);",
                 "int az_selfplay_sims(az_engine *e, int32_t *sims);",
                 "int az_selfplay_export_count(az_engine *e, int64_t *records);"):
        assert decl in text, decl
    assert "az_resign_mix(key(g) ^ az_resign_mix((uint32_t)p + 0x9E3779B9u)) % 1000 < full_permille" in text
    L = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)
    # the counters, the configuration and the self-play arguments keep their layout: the cap is an engine option
    assert len(_capi.az_counters._fields_) == 21 and len(_capi.az_config._fields_) == 12
    assert len(_capi.az_selfplay_args._fields_) == 7


def test_null_engine_is_an_error():
    L = _capi.lib()
    assert L.az_set_playout_cap(None, 4, 250, 1) == -1 and L.az_set_playout_cap(None, 0, 0, 0) == -1
    assert L.az_get_playout_cap(None, None, None, None) == -1           # like az_get_resign
    assert L.az_selfplay_sims(None, None) == -6                         # like az_selfplay_values
    assert L.az_selfplay_export_count(None, None) == -6


def test_fullness_equals_the_numpy_restatement():
    rs = np.random.RandomState(23)
    keys = rs.randint(0, 2 ** 32, 10000, dtype=np.uint64)
    keys[:4] = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    plies = rs.randint(0, 226, 10000)
    permille = rs.randint(0, 1001, 10000)
    permille[:6] = [0, 1, 500, 999, 1000, 1000]
    want = np_full(keys, plies, permille)
    got = np.array([_capi.playout_cap_full(int(k), int(p), int(m)) for k, p, m in zip(keys, plies, permille)])
    assert np.array_equal(got, want)
    assert 0 < want.sum() < len(want)
    assert not np_full(keys, plies, 0).any() and np_full(keys, plies, 1000).all()
    assert not any(_capi.playout_cap_full(int(k), int(p), 0) for k, p in zip(keys[:256], plies[:256]))
    assert all(_capi.playout_cap_full(int(k), int(p), 1000) for k, p in zip(keys[:256], plies[:256]))
    # the key is the low 32 bits of seed0 + g, and the ply matters
    assert _capi.playout_cap_full(2 ** 32 + 77, 5, 300) == _capi.playout_cap_full(77, 5, 300)
    t = full_table(9000, 64, 64, 250)
    assert len({tuple(row) for row in t.tolist()}) > 32 and len({tuple(col) for col in t.T.tolist()}) > 32
    assert 0.22 < full_table(5000, 200, 50, 250).mean() < 0.28      # a quarter of 10000 plies: 0.25 +- 6 sigma (sigma = 0.0043)


def test_python_argument_validation():
    assert _capi.playout_cap_permille(0.0) == 0 and _capi.playout_cap_permille(1.0) == 1000
    assert _capi.playout_cap_permille(0.25) == 250 and _capi.playout_cap_permille(0.0006) == 1
    for bad in (-0.1, 1.001, float("nan")):
        with pytest.raises(ValueError, match="full"):
            _capi.playout_cap_permille(bad)
    e = object.__new__(_capi.Engine)          # the checks come before the library is called: no engine needed
    e.h = ctypes.c_void_p()
    with pytest.raises(ValueError, match="fast_sims"):
        e.set_playout_cap(-1)
    with pytest.raises(ValueError, match="full"):
        e.set_playout_cap(4, full=1.5)
    # the seam
    assert check_playout_cap(None) is None
    assert check_playout_cap({"fast_sims": 25}) == {"fast_sims": 25, "full": 0.25, "train_on_fast": False}
    assert check_playout_cap({"fast_sims": 100, "full": 1, "train_on_fast": 1}, 100) == {"fast_sims": 100, "full": 1.0, "train_on_fast": True}
    for bad in ({}, {"full": 0.25}, {"fast_sims": 0}, {"fast_sims": -3}, {"fast_sims": 8, "full": 1.5}, {"fast_sims": 8, "full": -0.1},
                {"fast_sims": 8, "share": 0.25}, {"fast_sims": 101}):
        with pytest.raises(ValueError):
            check_playout_cap(bad, 100)
        with pytest.raises(ValueError):
            SelfPlayManager(controller=None, device="cuda:0", playout_cap=bad)        # 100 simulations by default
    m = SelfPlayManager(controller=None, device="cuda:0", mcts_params={"num_simulations": 40}, playout_cap={"fast_sims": 10, "full": 0.5})
    assert m.playout_cap == {"fast_sims": 10, "full": 0.5, "train_on_fast": False} and m.last_playout_cap_stats is None
    assert SelfPlayManager(None, "cuda:0").playout_cap is None
    with pytest.raises(ValueError, match="40"):
        SelfPlayManager(None, "cuda:0", mcts_params={"num_simulations": 40}, playout_cap={"fast_sims": 41})
    with pytest.raises(ValueError, match="subtree_reuse"):
        SelfPlayManager(None, "cuda:0", subtree_reuse=True, playout_cap={"fast_sims": 10})


def test_playout_cap_stats():
    s = playout_cap_stats([24, 6, 6, 24, 6, 6, 6, 6], [1, 0, 0, 1, 0, 0, 0, 0])
    assert s == {"records": 8, "full_records": 2, "mean_sims_per_ply": 10.5}
    assert playout_cap_stats([], []) == {"records": 0, "full_records": 0, "mean_sims_per_ply": None}
    # fast_sims = num_simulations: the simulations cannot tell the kinds apart, the hash can -- as the export filter does
    assert playout_cap_stats([24, 24, 24], [True, False, False])["full_records"] == 1
    with pytest.raises(ValueError):
        playout_cap_stats([24, 6], [True])
    # the per-record flags the statistics are made from: the library's rule, game-major then ply, from each game's first ply
    nply, ply0 = np.array([3, 0, 5, 2]), np.array([0, 0, 4, 7])
    got = playout_cap_full_plies(2 ** 32 - 2, nply, ply0, 0.4)
    want = [_capi.playout_cap_full(2 ** 32 - 2 + g, ply0[g] + m, 400) for g in range(4) for m in range(nply[g])]
    assert got.dtype == bool and got.tolist() == want
    assert np.array_equal(playout_cap_full_plies(7, [5] * 16, 0, 0.25), full_table(7, 16, 5, 250).reshape(-1))


def test_the_inputs_of_the_gpu_tests_mix_both_kinds():
    t = full_table(7, 16, 5, 250)
    assert int(t.sum()) == 21 and 0.15 < t.mean() < 0.40             # 21 of 80
    assert int(t[:, 0].sum()) == 4                                   # ply 0 has both kinds
    assert int(full_table(7, 6, 1, 500).sum()) == 3
    assert bool(_capi.playout_cap_full(7, 0, 250)) == bool(t[0, 0])
