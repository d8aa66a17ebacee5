"""Delta evaluation on the GPU (csrc/az_delta.h): within a ply the trunk evaluates the root's stones once per
side to move and every leaf only where its conv footprints differ from them.  Every output element is the same k-ordered fma
chain as in the full trunk, so everything here is compared as uint32 bit patterns: net_eval_delta against net_eval (the full
fused trunk) and against the CPU oracle; lock-step plies with the switch on against the switch off and the oracle's search.

Weights: the synthetic net and the two border-sharp sets of tests/test_border_columns_gpu.py ("negative": border taps of conv2 /
conv3 scaled by 8 and negative, conv biases +0; "ring": each side scaled by a factor of its own), rebuilt here."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict, synthetic_state_dict
from tests.util import build_weights

N, K = 15, 5
NN = N * N
CONVS = ("conv2", "conv3")
BIASES = ("conv1.bias", "conv2.bias", "conv3.bias")
REC_KEYS = ("boards", "movers", "lasts", "visits", "pis", "actions", "z")
MAX_CHANGED, MAX_TILES = 8, 12          # az_delta.h: DELTA_MAX_CHANGED, DELTA_TILES_DEFAULT


def _weight_sets():
    sd = synthetic_state_dict(N)
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
        w[:, :, :, 0] *= np.float32(4.0)
        w[:, :, :, 2] *= np.float32(8.0)
        w[:, :, 0, :] *= np.float32(2.0)
        w[:, :, 2, :] *= np.float32(16.0)
    return {"synthetic": sd, "negative": negative, "ring": ring}


@pytest.fixture(scope="module")
def weight_sets():
    return _weight_sets()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _root(cells, first=1):
    """the position after `cells` were played alternately, `first` moving first: (board, player to move, last)"""
    b = np.zeros(NN, np.uint8)
    for j, c in enumerate(cells):
        b[c] = first if j % 2 == 0 else 3 - first
    return b, first if len(cells) % 2 == 0 else 3 - first, (cells[-1] if cells else -1)


def _leaf(root, cells):
    """the root plus `cells` played alternately by the root's mover and the opponent"""
    b, pl, last = root[0].copy(), root[1], root[2]
    for c in cells:
        assert b[c] == 0
        b[c] = pl
        pl, last = 3 - pl, c
    return b, pl, last


def _tiles(cells):
    """conv3 tiles of a leaf whose changed cells are `cells`: the clipped 7x7 windows, 16 cells per tile"""
    s = set()
    for ch in cells:
        r0, c0 = divmod(int(ch), N)
        s |= {(r, c) for r in range(max(0, r0 - 3), min(N - 1, r0 + 3) + 1) for c in range(max(0, c0 - 3), min(N - 1, c0 + 3) + 1)}
    return (len(s) + 15) // 16


def _mid_root():
    rs = np.random.RandomState(1507)
    return _root([int(c) for c in rs.permutation(NN)[:30]])


def _cases():
    """[(name, root, [leaf cells, ...])]: every leaf is the root plus the listed stones"""
    empty, mid = _root([]), _mid_root()
    out = [("depth 1 from the empty board", empty, [[c] for c in range(NN)]),
           ("depth 1 from a mid-game position", mid, [[c] for c in range(NN) if mid[0][c] == 0])]
    rs = np.random.RandomState(1508)
    deep = []
    corners, edges = [0, N - 1, NN - N, NN - 1], [7, 7 * N, 7 * N + N - 1, NN - N + 7, 1, N, NN - 2, NN - N - 1]
    free = [c for c in range(NN) if mid[0][c] == 0]
    for a in corners + edges:                                   # a border or corner cell with a neighbour, and with a far cell
        if mid[0][a]:
            continue
        r, c = divmod(a, N)
        near = [x for x in free if x != a and max(abs(x // N - r), abs(x % N - c)) <= 2]
        far = [x for x in free if max(abs(x // N - r), abs(x % N - c)) >= 8]
        deep.append([near[0], a]); deep.append([a, far[0]]); deep.append([far[1], near[-1], a])
    while len(deep) < 90:                                       # seeded depth 2 and 3: overlapping, adjacent and disjoint footprints
        d = 2 + len(deep) % 2
        a = int(rs.choice(free)); r, c = divmod(a, N)
        k = int(rs.choice([1, 3, 6, 14]))
        cand = [x for x in free if x != a and max(abs(x // N - r), abs(x % N - c)) <= k]
        pick = [a] + [int(x) for x in rs.choice(cand, d - 1, replace=False)]
        deep.append(pick)
    out.append(("depth 2 and 3 from a mid-game position", mid, deep))
    out.append(("depth 2 and 3 from the empty board", empty, deep))
    return out


def _oracle_rows(onet, o, leaves):
    def one(lf):
        return onet.eval(o.encode(lf[0], int(lf[1]), int(lf[2])))
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(one, leaves))


def _assert_rows(got, want, oracle, what):
    for a, b, name in zip(got[:3], want, ("logits", "P", "value")):
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: {name} differ from the full trunk"
    for i, (ol, oP, ov) in enumerate(oracle):
        assert np.array_equal(_bits(got[0][i]), _bits(ol)), f"{what}, leaf {i}: logits differ from the oracle"
        assert np.array_equal(_bits(got[1][i]), _bits(oP)), f"{what}, leaf {i}: P differs from the oracle"
        assert _bits(got[2][i:i + 1])[0] == _bits(np.float32(ov).reshape(1))[0], f"{what}, leaf {i}: value differs from the oracle"


def _stack(leaves):
    return (np.stack([l[0] for l in leaves]), np.array([l[1] for l in leaves], np.uint8), np.array([l[2] for l in leaves], np.int16))


@pytest.mark.parametrize("tag", ["synthetic", "negative", "ring"])
def test_leaves_equal_the_full_trunk_and_the_oracle(weight_sets, tag):
    sd = weight_sets[tag]
    o, onet = orc.Oracle(N, K, 1), orc.Net(N, sd)
    e = az.Engine(N, K, 4, NN, model="plain")
    e.load_weights(sd, 0)
    try:
        for name, root, cells in _cases():
            leaves = [_leaf(root, cs) for cs in cells]
            boards, players, lasts = _stack(leaves)
            got = e.net_eval_delta(root[0], root[1], boards, players, lasts)
            want = e.net_eval(boards, players, lasts)
            _assert_rows(got, want, _oracle_rows(onet, o, leaves), f"{tag}, {name}")
            # every one of them on the delta path, with the conv3 tiles of its footprint
            assert got[3].tolist() == [_tiles(cs) for cs in cells], f"{tag}, {name}: path taken"
    finally:
        e.close()


def test_the_root_itself_and_the_empty_board(weight_sets):
    sd = weight_sets["ring"]
    o, onet = orc.Oracle(N, K, 1), orc.Net(N, sd)
    e = az.Engine(N, K, 4, 8, model="plain")
    e.load_weights(sd, 0)
    try:
        for root in (_root([]), _root([]) [:1] + (2, -1), _mid_root(), _root([0]), _root([7 * N + 7, NN - 1])):
            boards, players, lasts = _stack([root])
            got = e.net_eval_delta(root[0], root[1], boards, players, lasts)
            want = e.net_eval(boards, players, lasts)
            _assert_rows(got, want, _oracle_rows(onet, o, [root]), "the root as its own leaf")
            # one changed cell, its last-move cell; none on a board without a last move
            assert got[3].tolist() == [_tiles([root[2]]) if root[2] >= 0 else 0]
    finally:
        e.close()


def test_fallback_threshold_and_reported_path(weight_sets):
    sd = weight_sets["synthetic"]
    o, onet = orc.Oracle(N, K, 1), orc.Net(N, sd)
    empty = _root([])
    inner = [3 * N + 3, 3 * N + 10, 10 * N + 3]                  # three disjoint interior 7x7 windows: 147 cells
    at = [inner + [NN - 1, 7 * N + 14],                          # + a corner (16 cells) and an edge window (19 new): 182 cells, 12 tiles -- the last on the delta path
          inner + [10 * N + 10],                                 # four disjoint windows: 196 cells, 13 tiles -- the first in full
          [7 * N + 6 + j for j in range(3)] + [8 * N + 6 + j for j in range(3)] + [9 * N + 6, 9 * N + 7],    # 8 changed cells, clustered: delta
          [7 * N + 6 + j for j in range(3)] + [8 * N + 6 + j for j in range(3)] + [9 * N + 6 + j for j in range(3)]]    # 9: in full
    assert [_tiles(c) for c in at[:2]] == [MAX_TILES, MAX_TILES + 1] and [len(c) for c in at[2:]] == [MAX_CHANGED, MAX_CHANGED + 1]
    leaves = [_leaf(empty, cs) for cs in at]
    boards, players, lasts = _stack(leaves)
    oracle = _oracle_rows(onet, o, leaves)
    e = az.Engine(N, K, 4, 8, model="plain")
    e.load_weights(sd, 0)
    try:
        assert e.delta_eval() and e.delta_max_tiles() == MAX_TILES
        want = e.net_eval(boards, players, lasts)
        got = e.net_eval_delta(empty[0], empty[1], boards, players, lasts)
        _assert_rows(got, want, oracle, "default threshold")
        assert got[3].tolist() == [MAX_TILES, -1, _tiles(at[2]), -1]
        # the threshold moves: 4 tiles take one interior window and nothing more; 15 take everything with at most 8 changed cells
        assert e.delta_max_tiles(4) == 4
        one = [_leaf(empty, [7 * N + 7]), _leaf(empty, [7 * N + 7, 7 * N + 11]), _leaf(empty, [0, NN - 1, N - 1, NN - N])]
        ob, op, ol = _stack(one)
        got4 = e.net_eval_delta(empty[0], empty[1], ob, op, ol)
        _assert_rows(got4, e.net_eval(ob, op, ol), _oracle_rows(onet, o, one), "threshold 4")
        assert got4[3].tolist() == [4, -1, 4]
        assert e.delta_max_tiles(15) == 15
        got15 = e.net_eval_delta(empty[0], empty[1], boards, players, lasts)
        _assert_rows(got15, want, oracle, "threshold 15")
        assert got15[3].tolist() == [MAX_TILES, MAX_TILES + 1, _tiles(at[2]), -1]
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# lock-step plies
# ---------------------------------------------------------------------------------------------------------------------
def _start_positions():
    """three positions hugging a corner, an edge and the opposite corner"""
    pos = [_root([0, 1, N + 1, N]), _root([7 * N, 6 * N, 8 * N + 1, 7 * N + 1]), _root([NN - 1, NN - 2, NN - N - 1])]
    return _stack(pos)


def _lockstep(sd, on, S, slots, G, seed, max_plies, start=None, cache=0, setup=None, **kw):
    e = az.Engine(N, K, S, slots, model="plain", log_table=orc.numpy_log_table(S), **kw)
    try:
        e.load_weights(sd, 0)
        e.set_delta_eval(on)
        if setup:
            setup(e)
        if cache:
            e.set_eval_cache(cache)
        if start is not None:
            e.set_start_positions(*start)
        c = e.selfplay(G, seed0=seed, max_plies=max_plies)
        rec = e.records()
        nply, res = e.games()
        return c, rec, nply, res, e.delta_stats()
    finally:
        e.close()


@pytest.mark.parametrize("cache", [0, 4096])
@pytest.mark.parametrize("started", [False, True])
@pytest.mark.parametrize("tag", ["synthetic", "ring"])
def test_lockstep_plies_equal_switch_off_and_the_oracle(weight_sets, tag, started, cache):
    """"synthetic": shallow searches, everything on the delta path.  "ring": priors so sharp that the 24 simulations dig one line
    14 stones deep -- most leaves have more than 8 changed cells and fall back to the full trunk inside the same launches."""
    S, G, seed = 24, 6, 1509
    sd = weight_sets[tag]
    start = _start_positions() if started else None
    max_plies = 7 if started else 3                              # absolute plies: the positions hold 4, 4 and 3 stones
    c1, rec1, nply1, res1, st1 = _lockstep(sd, True, S, G, G, seed, max_plies, start, cache)
    c0, rec0, nply0, res0, st0 = _lockstep(sd, False, S, G, G, seed, max_plies, start, cache)
    assert nply1.tolist() == nply0.tolist() == ([3, 3, 4, 3, 3, 4] if started else [3] * G) and res1.tolist() == res0.tolist()
    for key in REC_KEYS:
        assert np.array_equal(rec1[key], rec0[key]), f"{key}: switch on and off differ"
    assert np.array_equal(_bits(rec1["pis"]), _bits(rec0["pis"]))
    for key in ("expansions", "simulations", "terminal_hits", "depth_sum", "root_evals", "cache_hits", "trunk_boards"):
        assert c1[key] == c0[key], key
    # the oracle's search of every recorded root, with the game's own tape by absolute ply
    o, onet = orc.Oracle(N, K, S, log_table=orc.numpy_log_table(S)), orc.Net(N, sd)
    T = orc.selfplay_T_table(NN)
    game_of = np.repeat(np.arange(G), nply1)
    tapes = [orc.selfplay_tape(seed + g, N, maxply=max_plies) for g in range(G)]

    def one(i):
        g = int(game_of[i]); m = int(np.count_nonzero(rec1["boards"][i]))
        off = sum(NN - j for j in range(m))
        return o.search(onet, rec1["boards"][i], int(rec1["movers"][i]), int(rec1["lasts"][i]), float(T[m]),
                        tapes[g][0][off:off + NN - m], float(tapes[g][1][m]))
    with ThreadPoolExecutor(max_workers=8) as ex:
        want = list(ex.map(one, range(len(game_of))))
    for i, r in enumerate(want):
        assert np.array_equal(rec1["visits"][i], r["N"]) and np.array_equal(_bits(rec1["pis"][i]), _bits(r["pi"])), f"record {i}"
        assert int(rec1["actions"][i]) == r["action"], f"record {i}"
    assert st0 == dict(delta=0, full=0, tiles=0, base=0)
    assert st1["delta"] + st1["full"] == c1["trunk_boards"] == c1["expansions"] + c1["root_evals"] - c1["cache_hits"]
    assert st1["base"] == 2 * c1["plies"] and 0 < st1["tiles"] <= MAX_TILES * st1["delta"]
    deepest = max(r["maxd"] for r in want)
    if tag == "synthetic":
        # no search of these inputs goes deeper than three stones below its root: at most 3 changed cells and 10 conv3 tiles per
        # leaf, inside both limits -- so every evaluation must have taken the delta path, and the counters must say so
        assert deepest <= 3
        assert st1["full"] == 0 and st1["delta"] >= 0.9 * c1["trunk_boards"] and st1["tiles"] <= 10 * st1["delta"]
    else:
        assert deepest > MAX_CHANGED and st1["full"] > 0 and st1["delta"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# configurations the delta path does not serve: no delta or base evaluation, and the switch changes nothing
# ---------------------------------------------------------------------------------------------------------------------
def _run(on, n, model, sd, setup, arena):
    S, G = 8, 4
    k = 5 if n >= 9 else 4
    e = az.Engine(n, k, S, G, model=model, log_table=orc.numpy_log_table(S))
    try:
        e.load_weights(sd, 0)
        if arena:
            e.load_weights(sd, 1)
        e.set_delta_eval(on)
        if setup:
            setup(e)
        if arena:
            r = e.arena(G, seed0=77)
            out = [r["results"], r["actions"], r["nply"]]
        else:
            e.selfplay(G, seed0=77, max_plies=2)
            rec = e.records()
            out = [rec[key] for key in REC_KEYS]
        return out, e.delta_stats()
    finally:
        e.close()


@pytest.mark.parametrize("what", ["leaf symmetry", "virtual loss 4", "arena", "resnet", "emulated trunk", "9x9"])
def test_out_of_scope_configurations_evaluate_in_full(weight_sets, what):
    n = 9 if what == "9x9" else N
    model = "resnet" if what == "resnet" else "plain"
    sd = synthetic_resnet_state_dict(n) if what == "resnet" else (build_weights(9) if what == "9x9" else weight_sets["synthetic"])
    setup = {"leaf symmetry": lambda e: e.set_leaf_symmetry(True), "virtual loss 4": lambda e: e.set_virtual_loss(4),
             "emulated trunk": lambda e: e.set_trunk_mode("f16x2")}.get(what)
    a, sa = _run(True, n, model, sd, setup, what == "arena")
    b, sb = _run(False, n, model, sd, setup, what == "arena")
    assert sa == sb == dict(delta=0, full=0, tiles=0, base=0), what
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), what
