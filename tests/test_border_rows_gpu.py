"""The border rows of the 15x15 board: the fused trunks leave out the conv taps that read only the zero padding row above
row 0 and below row 14 (az_net.h, BorderSkip).  Every layer output must keep its bits, so the fused trunk, the tile-split
trunk (which multiplies the zero rows as before) and the oracle (which skips out-of-board taps by definition) agree as
uint32 bit patterns.

Weights: the ky = 0 and ky = 2 taps of every 3x3 conv behind the first are multiplied by 8 (exact in float32), so that
skipping the wrong row or the wrong tap moves every border logit grossly; a second set has those taps all negative and the
conv biases +0 (products w * 0 are then -0, accumulators start from +0 with nothing added)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.net import fold_resnet_state_dict
from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict, synthetic_state_dict

N, K = 15, 5
NN = N * N
PLAIN_CONVS = ("conv2", "conv3")                                    # the packed-input layers of GomokuNet
PLAIN_BIASES = ("conv1.bias", "conv2.bias", "conv3.bias")
RES_CONVS = ("conv",) + tuple(f"res{r}.conv{c}" for r in (1, 2, 3) for c in (1, 2))      # stem and block convs
RES_BIASES = ("conv.bias",)                                         # the block convs have none


def _weight_sets(sd, convs, biases):
    scaled = {k: v.copy() for k, v in sd.items()}
    for name in convs:
        w = scaled[name + ".weight"]
        w[:, :, 0, :] *= np.float32(8.0)
        w[:, :, 2, :] *= np.float32(8.0)
    negative = {k: v.copy() for k, v in scaled.items()}
    for name in convs:
        w = negative[name + ".weight"]
        w[:, :, 0, :] = -np.abs(w[:, :, 0, :])
        w[:, :, 2, :] = -np.abs(w[:, :, 2, :])
    for name in biases:
        negative[name] = np.zeros_like(negative[name])
    return {"scaled": scaled, "negative": negative}


def _positions():
    """(board, player, last) x 24: what can sit on, next to and away from the two border rows."""
    out = []

    def add(cells, last=None, player=None):
        b = np.zeros(NN, np.uint8)
        for j, c in enumerate(cells):
            b[c] = 1 + j % 2
        out.append((b, (1 + len(cells) % 2) if player is None else player, (cells[-1] if cells else -1) if last is None else last))

    row = lambda r: [r * N + c for c in range(N)]
    corners = [0, N - 1, NN - N, NN - 1]
    rs = np.random.RandomState(15)
    mid = [int(c) for c in rs.permutation(NN)[:61]]
    add([])                                                          # the empty board
    add([], player=2)
    add(row(0)[::2]); add(row(0)[::2], player=2)                     # stones only on row 0, both movers
    add(row(N - 1)[::2]); add(row(N - 1)[::2], player=2)             # only on row 14, both movers
    add(row(0) + row(N - 1)); add(row(0) + row(N - 1), player=2)     # rows 0 and 14 full
    add(row(1)); add(row(N - 2))                                     # full rows next to the border rows
    add(corners); add(corners, player=2)
    add(mid); add(mid, player=1)                                     # a mid-game position, both movers
    for c in corners:                                                # last move in each corner
        add([7 * N + 7, c])
    add([7 * N + 7, 7]); add([7 * N + 7, NN - N + 7])                # last move on row 0 / row 14
    add([7 * N + 7, 7 * N]); add([7 * N + 7, 7 * N + N - 1])         # ... on column 0 / column 14
    add(mid + [3], player=1); add(mid[:40] + [NN - 4])               # mid-game, last move on a border row
    assert len(out) == 24
    boards = np.stack([p[0] for p in out])
    return boards, np.array([p[1] for p in out], np.uint8), np.array([p[2] for p in out], np.int16)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _engine(model, split, S=4, slots=9, **kw):
    env = {"AZ_SPLIT_MAX": split}
    env.update(kw.pop("env", {}))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return az.Engine(N, K, S, slots, model=model, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check_forward(model, sd, tag):
    boards, players, lasts = _positions()
    o = orc.Oracle(N, K, 1)
    onet = orc.Net(N, sd) if model == "plain" else orc.Net(N, resnet_tensors=fold_resnet_state_dict(sd))
    want = [onet.eval(o.encode(boards[i], int(players[i]), int(lasts[i]))) for i in range(len(players))]
    got = {}
    for name, split in (("fused", "0"), ("split", "1000000")):
        e = _engine(model, split)
        e.load_weights(sd, 0)
        got[name] = e.net_eval(boards, players, lasts)
        e.close()
    for i, (ol, oP, ov) in enumerate(want):
        for name in ("fused", "split"):
            logits, P, v = got[name]
            assert np.array_equal(_bits(logits[i]), _bits(ol)), f"{model} {tag} {name} board {i}: logits"
            assert np.array_equal(_bits(P[i]), _bits(oP)), f"{model} {tag} {name} board {i}: P"
            assert _bits(v[i:i + 1])[0] == _bits(np.float32(ov).reshape(1))[0], f"{model} {tag} {name} board {i}: value"
    for a, b in zip(got["fused"], got["split"]):
        assert np.array_equal(_bits(a), _bits(b)), f"{model} {tag}: fused and tile-split trunks differ"


@pytest.mark.parametrize("tag", ["scaled", "negative"])
def test_plain_net_forward_bits(tag):
    _check_forward("plain", _weight_sets(synthetic_state_dict(N), PLAIN_CONVS, PLAIN_BIASES)[tag], tag)


@pytest.mark.parametrize("tag", ["scaled", "negative"])
def test_resnet_forward_bits(tag):
    _check_forward("resnet", _weight_sets(synthetic_resnet_state_dict(N), RES_CONVS, RES_BIASES)[tag], tag)


def test_scaled_taps_reach_the_border_logits():
    """The fixture is sharp: with the original taps in place of the scaled ones every position's logits differ."""
    boards, players, lasts = _positions()
    o = orc.Oracle(N, K, 1)
    sd = synthetic_state_dict(N)
    a, b = orc.Net(N, sd), orc.Net(N, _weight_sets(sd, PLAIN_CONVS, PLAIN_BIASES)["scaled"])
    for i in range(len(players)):
        x = o.encode(boards[i], int(players[i]), int(lasts[i]))
        la, lb = a.eval(x)[0].reshape(N, N), b.eval(x)[0].reshape(N, N)
        assert np.abs(la[0] - lb[0]).max() > 1e-3 and np.abs(la[N - 1] - lb[N - 1]).max() > 1e-3, f"board {i}"


def test_lockstep_ply_equals_the_oracle():
    """One ply of self-play on the lock-step path (captured graph, fused k_trunk: the persistent search kernel and the
    tile-split trunk are switched off), 4 slots, 16 simulations, the scaled weights: visit counts, pi and actions."""
    S, G, seed = 16, 4, 900
    sd = _weight_sets(synthetic_state_dict(N), PLAIN_CONVS, PLAIN_BIASES)["scaled"]
    e = _engine("plain", "0", S=S, slots=4, log_table=orc.numpy_log_table(S), env={"AZ_PERSIST": "0"})
    e.load_weights(sd, 0)
    c = e.selfplay(G, seed0=seed, max_plies=1)
    rec = e.records(); nply, _ = e.games()
    e.close()
    assert c["trunk_launches"] >= S + 1, "one trunk launch per simulation: the ply did not run on the lock-step path"
    o = orc.Oracle(N, K, S, log_table=orc.numpy_log_table(S))
    onet = orc.Net(N, sd)
    off = 0
    for g in range(G):
        noise, us = orc.selfplay_tape(seed + g, N)
        r = o.selfplay_game(onet, noise, us, maxply=1)
        L = int(nply[g]); sl = slice(off, off + L)
        assert L == r["nply"] == 1
        for key in ("actions", "visits", "pis"):
            assert np.array_equal(rec[key][sl], r[key]), f"game {g}: {key}"
        off += L
