"""The border columns of the 15x15 board: the fused float32 trunk lays its 15 cell tiles round the board (az_net.h, RingGeo:
row 0, row 14, column 0, column 14 and eleven tiles of the 13x13 interior) and leaves out the conv taps that read only the zero
padding -- ky = 0 / ky = 2 for the two row tiles as before, kx = 0 / kx = 2 for the two column tiles.  Every layer output must
keep its bits, so the fused trunk, the tile-split trunk (row tiles, multiplies every zero) and the oracle (which skips
out-of-board taps by definition) agree as uint32 bit patterns.

Weights: "scaled" has the kx = 0 and kx = 2 taps of conv2 and conv3 times 8 (exact in float32), so that skipping the wrong
column or the wrong tap moves every border logit grossly; "negative" has those taps all negative and the conv biases +0
(products w * 0 are then -0, accumulators start from +0 with nothing added); "ring" scales all four sides with a factor of its
own (left 4, right 8, top 2, bottom 16), so that a swapped side shows."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.weights import synthetic_state_dict

N, K = 15, 5
NN = N * N
CONVS = ("conv2", "conv3")                                          # the packed-input layers of GomokuNet
BIASES = ("conv1.bias", "conv2.bias", "conv3.bias")


def _weight_sets(sd):
    scaled = {k: v.copy() for k, v in sd.items()}
    for name in CONVS:
        w = scaled[name + ".weight"]
        w[:, :, :, 0] *= np.float32(8.0)
        w[:, :, :, 2] *= np.float32(8.0)
    negative = {k: v.copy() for k, v in scaled.items()}
    for name in CONVS:
        w = negative[name + ".weight"]
        w[:, :, :, 0] = -np.abs(w[:, :, :, 0])
        w[:, :, :, 2] = -np.abs(w[:, :, :, 2])
    for name in BIASES:
        negative[name] = np.zeros_like(negative[name])
    ring = {k: v.copy() for k, v in sd.items()}
    for name in CONVS:
        w = ring[name + ".weight"]
        w[:, :, :, 0] *= np.float32(4.0)                            # left
        w[:, :, :, 2] *= np.float32(8.0)                            # right
        w[:, :, 0, :] *= np.float32(2.0)                            # top
        w[:, :, 2, :] *= np.float32(16.0)                           # bottom
    return {"scaled": scaled, "negative": negative, "ring": ring}


def _positions():
    """(board, player, last) x 36: what can sit on, next to and away from the two border columns (the positions of the border
    rows' test, transposed), the four border-near columns full, the corners one by one."""
    out = []

    def add(cells, last=None, player=None):
        b = np.zeros(NN, np.uint8)
        for j, c in enumerate(cells):
            b[c] = 1 + j % 2
        out.append((b, (1 + len(cells) % 2) if player is None else player, (cells[-1] if cells else -1) if last is None else last))

    col = lambda c: [r * N + c for r in range(N)]
    tr = lambda p: (p % N) * N + p // N
    corners = [0, NN - N, N - 1, NN - 1]
    rs = np.random.RandomState(15)
    mid = [tr(int(c)) for c in rs.permutation(NN)[:61]]
    add([])                                                          # the empty board
    add([], player=2)
    add(col(0)[::2]); add(col(0)[::2], player=2)                     # stones only on column 0, both movers
    add(col(N - 1)[::2]); add(col(N - 1)[::2], player=2)             # only on column 14, both movers
    add(col(0) + col(N - 1)); add(col(0) + col(N - 1), player=2)     # columns 0 and 14 full
    add(col(1)); add(col(N - 2))                                     # full columns next to the border columns
    add(corners); add(corners, player=2)
    add(mid); add(mid, player=1)                                     # a mid-game position, both movers
    for c in corners:                                                # last move in each corner
        add([7 * N + 7, c])
    add([7 * N + 7, 7 * N]); add([7 * N + 7, 7 * N + N - 1])         # last move on column 0 / column 14
    add([7 * N + 7, 7]); add([7 * N + 7, NN - N + 7])                # ... on row 0 / row 14
    add(mid + [3 * N], player=1); add(mid[:40] + [NN - 3 * N - 1])   # mid-game, last move on a border column
    for c in (0, 1, N - 2, N - 1):                                   # each of the four columns alone, full, both movers
        add(col(c)); add(col(c), player=2)
    for c in corners:                                                # one stone in one corner, the opponent to move
        add([c])
    assert len(out) == 36
    boards = np.stack([p[0] for p in out])
    return boards, np.array([p[1] for p in out], np.uint8), np.array([p[2] for p in out], np.int16)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _engine(split, S=4, slots=9, **kw):
    env = {"AZ_SPLIT_MAX": split}
    env.update(kw.pop("env", {}))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return az.Engine(N, K, S, slots, model="plain", **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def weight_sets():
    return _weight_sets(synthetic_state_dict(N))


@pytest.mark.parametrize("tag", ["scaled", "negative", "ring"])
def test_forward_bits(weight_sets, tag):
    sd = weight_sets[tag]
    boards, players, lasts = _positions()
    o = orc.Oracle(N, K, 1)
    onet = orc.Net(N, sd)
    want = [onet.eval(o.encode(boards[i], int(players[i]), int(lasts[i]))) for i in range(len(players))]
    got = {}
    for name, split in (("fused", "0"), ("split", "1000000")):
        e = _engine(split)
        e.load_weights(sd, 0)
        got[name] = e.net_eval(boards, players, lasts)
        e.close()
    for i, (ol, oP, ov) in enumerate(want):
        for name in ("fused", "split"):
            logits, P, v = got[name]
            assert np.array_equal(_bits(logits[i]), _bits(ol)), f"{tag} {name} board {i}: logits"
            assert np.array_equal(_bits(P[i]), _bits(oP)), f"{tag} {name} board {i}: P"
            assert _bits(v[i:i + 1])[0] == _bits(np.float32(ov).reshape(1))[0], f"{tag} {name} board {i}: value"
    for a, b in zip(got["fused"], got["split"]):
        assert np.array_equal(_bits(a), _bits(b)), f"{tag}: fused and tile-split trunks differ"


def test_every_cell_once(weight_sets):
    """225 boards with one stone each, the opponent to move, and 225 more with the stone's owner to move again (the stone then
    sits on the mover's plane): a wrong entry anywhere in the tile map moves the logits of the board whose only stone is on that
    cell.  Each set is one net_eval call on the fused trunk."""
    sd = weight_sets["ring"]
    boards = np.zeros((NN, NN), np.uint8)
    boards[np.arange(NN), np.arange(NN)] = 1
    lasts = np.arange(NN, dtype=np.int16)
    o = orc.Oracle(N, K, 1)
    onet = orc.Net(N, sd)
    e = _engine("0", slots=NN)
    e.load_weights(sd, 0)
    try:
        for mover in (2, 1):
            players = np.full(NN, mover, np.uint8)
            logits, P, v = e.net_eval(boards, players, lasts)
            for i in range(NN):
                ol, oP, ov = onet.eval(o.encode(boards[i], mover, int(lasts[i])))
                assert np.array_equal(_bits(logits[i]), _bits(ol)), f"mover {mover}, stone on cell {i}: logits"
                assert np.array_equal(_bits(P[i]), _bits(oP)), f"mover {mover}, stone on cell {i}: P"
                assert _bits(v[i:i + 1])[0] == _bits(np.float32(ov).reshape(1))[0], f"mover {mover}, stone on cell {i}: value"
    finally:
        e.close()


def test_scaled_taps_reach_the_border_column_logits(weight_sets):
    """The fixture is sharp: with the original taps in place of the scaled ones every position's logits in columns 0 and 14
    differ by more than 1e-3."""
    boards, players, lasts = _positions()
    o = orc.Oracle(N, K, 1)
    a, b = orc.Net(N, synthetic_state_dict(N)), orc.Net(N, weight_sets["scaled"])
    for i in range(len(players)):
        x = o.encode(boards[i], int(players[i]), int(lasts[i]))
        la, lb = a.eval(x)[0].reshape(N, N), b.eval(x)[0].reshape(N, N)
        assert np.abs(la[:, 0] - lb[:, 0]).max() > 1e-3 and np.abs(la[:, N - 1] - lb[:, N - 1]).max() > 1e-3, f"board {i}"


def test_lockstep_ply_equals_the_oracle(weight_sets):
    """One ply of self-play on the lock-step path (captured graph, fused k_trunk: the persistent search kernel and the
    tile-split trunk are switched off), 4 slots, 16 simulations, the "ring" weights: visit counts, pi and actions."""
    S, G, seed = 16, 4, 915
    sd = weight_sets["ring"]
    e = _engine("0", S=S, slots=4, log_table=orc.numpy_log_table(S), env={"AZ_PERSIST": "0"})
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
