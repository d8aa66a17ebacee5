"""The head convs of the fused trunk on 4-row matrix blocks (az_net.h, trunk_heads): policy_conv and value_conv are computed
with v_mfma_f32_4x4x1_16b_f32 over a cell-major conv3 image, one input channel per instruction in ascending order.  That is
the oracle's chain, so the fused trunk, the tile-split trunk (16-row tiles as before) and the oracle agree as uint32 patterns.

Sizes: 3 and 4 (four boards per workgroup, 36 / 64 cells: cell quads straddle boards, one group of 32 cells is partial), 5,
9 (two boards, 162 cells), 12 (one board, 144 cells) and 15 (row tiles with a pad lane each, the 8th group half empty).  Nine
positions per size, so the last workgroup is never full.

Weights: the synthetic net; a head-sharp set (policy_conv rows x 1, 2, 4, 8, value_conv rows x 16, 32 -- exact in float32 --
and distinct head biases), with which a swapped row, cell or half moves the logits grossly; and a set with every head weight
negative and zero head biases (accumulators end at or below zero: -0 and the ReLU)."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.weights import synthetic_state_dict

SIZES = (3, 4, 5, 9, 12, 15)
TAGS = ("plain", "sharp", "negative")
NPOS = 9


def _k(n):
    return 5 if n > 5 else (4 if n >= 4 else 3)


@functools.lru_cache(maxsize=None)
def _weights(n, tag):
    sd = {k: v.copy() for k, v in synthetic_state_dict(n).items()}
    if tag == "plain":
        return sd
    pw, vw = sd["policy_conv.weight"], sd["value_conv.weight"]
    if tag == "sharp":
        for r, f in enumerate((1.0, 2.0, 4.0, 8.0)):
            pw[r] *= np.float32(f)
        for r, f in enumerate((16.0, 32.0)):
            vw[r] *= np.float32(f)
        sd["policy_conv.bias"] = np.array([0.03125, -0.0625, 0.125, 0.25], np.float32)
        sd["value_conv.bias"] = np.array([-0.5, 0.75], np.float32)
    else:
        pw[...] = -np.abs(pw)
        vw[...] = -np.abs(vw)
        pw[pw == 0] = np.float32(-1e-3)
        vw[vw == 0] = np.float32(-1e-3)
        sd["policy_conv.bias"] = np.zeros(4, np.float32)
        sd["value_conv.bias"] = np.zeros(2, np.float32)
    return sd


@functools.lru_cache(maxsize=None)
def _positions(n):
    """(boards, players, lasts) x 9: the empty board for both movers, then positions of growing density, movers alternating."""
    nn = n * n
    rs = np.random.RandomState(100 + n)
    boards, players, lasts = [np.zeros(nn, np.uint8), np.zeros(nn, np.uint8)], [1, 2], [-1, -1]
    for i in range(NPOS - 2):
        cnt = 1 + (i * (nn - 2)) // (NPOS - 3)
        cells = [int(c) for c in rs.permutation(nn)[:cnt]]
        b = np.zeros(nn, np.uint8)
        for j, c in enumerate(cells):
            b[c] = 1 + j % 2
        boards.append(b)
        players.append(1 + i % 2)
        lasts.append(cells[-1] if i % 3 else -1)
    return np.stack(boards), np.array(players, np.uint8), np.array(lasts, np.int16)


@functools.lru_cache(maxsize=None)
def _oracle_eval(n, tag):
    boards, players, lasts = _positions(n)
    o = orc.Oracle(n, _k(n), 1)
    onet = orc.Net(n, _weights(n, tag))
    return [onet.eval(o.encode(boards[i], int(players[i]), int(lasts[i]))) for i in range(NPOS)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _engine(n, split, S=4, slots=NPOS, **kw):
    env = {"AZ_SPLIT_MAX": split}
    env.update(kw.pop("env", {}))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return az.Engine(n, _k(n), S, slots, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", SIZES)
def test_forward_bits(n, tag):
    boards, players, lasts = _positions(n)
    want = _oracle_eval(n, tag)
    got = {}
    for name, split in (("fused", "0"), ("split", "1000000")):
        e = _engine(n, split)
        e.load_weights(_weights(n, tag), 0)
        got[name] = e.net_eval(boards, players, lasts)
        e.close()
    for i, (ol, oP, ov) in enumerate(want):
        for name in ("fused", "split"):
            logits, P, v = got[name]
            assert np.array_equal(_bits(logits[i]), _bits(ol)), f"n={n} {tag} {name} board {i}: logits"
            assert np.array_equal(_bits(P[i]), _bits(oP)), f"n={n} {tag} {name} board {i}: P"
            assert _bits(v[i:i + 1])[0] == _bits(np.float32(ov).reshape(1))[0], f"n={n} {tag} {name} board {i}: value"
    for a, b in zip(got["fused"], got["split"]):
        assert np.array_equal(_bits(a), _bits(b)), f"n={n} {tag}: fused and tile-split trunks differ"


@pytest.mark.parametrize("n", SIZES)
def test_sharp_heads_reach_the_logits(n):
    """The fixture is sharp: the scaled head rows and biases change every position's logits and value."""
    plain, sharp = _oracle_eval(n, "plain"), _oracle_eval(n, "sharp")
    for i in range(NPOS):
        assert np.abs(plain[i][0] - sharp[i][0]).max() > 1e-3, f"n={n} board {i}: logits"
        assert abs(float(plain[i][2]) - float(sharp[i][2])) > 1e-6, f"n={n} board {i}: value"


@pytest.mark.gpu
@pytest.mark.parametrize("n", (5, 15))
def test_lockstep_ply_equals_the_oracle(n):
    """One ply of self-play on the lock-step path (fused k_trunk: the persistent search kernel and the tile-split trunk are
    switched off), 5 slots -- not a multiple of the boards per workgroup, so a group holds idle boards whose feature rows stay
    untouched -- 16 simulations, the head-sharp weights: actions, visit counts and pi."""
    S, G, seed = 16, 5, 4100 + n
    sd = _weights(n, "sharp")
    e = _engine(n, "0", S=S, slots=5, log_table=orc.numpy_log_table(S), env={"AZ_PERSIST": "0"})
    e.load_weights(sd, 0)
    c = e.selfplay(G, seed0=seed, max_plies=1)
    rec = e.records(); nply, _ = e.games()
    e.close()
    assert c["trunk_launches"] >= S + 1, "one trunk launch per simulation: the ply did not run on the lock-step path"
    o = orc.Oracle(n, _k(n), S, log_table=orc.numpy_log_table(S))
    onet = orc.Net(n, sd)
    off = 0
    for g in range(G):
        noise, us = orc.selfplay_tape(seed + g, n)
        r = o.selfplay_game(onet, noise, us, maxply=1)
        L = int(nply[g]); sl = slice(off, off + L)
        assert L == r["nply"] == 1
        for key in ("actions", "visits", "pis"):
            assert np.array_equal(rec[key][sl], r[key]), f"n={n} game {g}: {key}"
        off += L
