"""k_trunk_delta<15> with conv1 recomputed on the conv3 tile list and the lean prologue (csrc/az_delta.h).

conv1 no longer copies its window from the base image: it computes every board cell within 3 of a changed cell and the kernel
zeroes the ring positions within 3 itself.  So the leaves here are those where the ring matters (corners, edges, distance 1 to 3
from an edge), the conv1 chunk counts (conv3 tiles 1, 4, 5, 8, 12, 14) and the conv2 tile counts that run the exact-count
instantiations (1, 2, 3, 5, 7), each with a full last tile and with one cell in it where such a leaf exists.  Everything is
compared as uint32 bit patterns: net_eval_delta against net_eval on the same engine and against the CPU oracle; lock-step plies
from an edge position with the switch on against the switch off and the oracle's games."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
import alphazero_piskvorky_amd as az
from tests import delta_cases as dc
from tests.test_delta_eval_gpu import K, MAX_TILES, N, NN, _assert_rows, _bits, _oracle_rows, _stack, _weight_sets
from tests.test_delta_shapes_gpu import _assert_counters, _assert_oracle, _assert_switch, _lockstep, _oracle_games

SLOTS = 6
TAGS = ["ring", "negative"]
C = dc.C


@pytest.fixture(scope="module")
def weight_sets():
    return _weight_sets()


@pytest.fixture(scope="module")
def engines(weight_sets):
    """per weight set: (engine, oracle, oracle net), made once"""
    out = {}
    for tag in TAGS:
        e = az.Engine(N, K, 4, SLOTS, model="plain")
        e.load_weights(weight_sets[tag], 0)
        out[tag] = (e, orc.Oracle(N, K, 1), orc.Net(N, weight_sets[tag]))
    yield out
    for e, _, _ in out.values():
        e.close()


@pytest.fixture(scope="module")
def shape_cases():
    return dc.cases()


def _compare(eng, root, cells_list, what, tiles=15, want_path=None):
    e, o, onet = eng
    leaves = [dc.leaf_of(root, cs) for cs in cells_list]
    boards, players, lasts = _stack(leaves)
    assert e.delta_max_tiles(tiles) == tiles
    got = e.net_eval_delta(root[0], root[1], boards, players, lasts)
    want = e.net_eval(boards, players, lasts)
    _assert_rows(got, want, _oracle_rows(onet, o, leaves), what)
    if want_path is None:
        want_path = [dc.tile_counts(cs)[2] for cs in cells_list]
    assert got[3].tolist() == want_path, f"{what}: path taken"
    return got


def _border_leaves():
    corners = [[0], [N - 1], [NN - N], [NN - 1]]
    edges = [[C(0, 7)], [C(7, 0)], [C(7, N - 1)], [C(N - 1, 7)]]
    near = []
    for k in (1, 2, 3):                              # distance 1, 2, 3 from each edge, and from two edges at once
        near += [[C(k, 7)], [C(7, k)], [C(7, N - 1 - k)], [C(N - 1 - k, 7)], [C(k, k)], [C(N - 1 - k, N - 1 - k)]]
    both = [[0, NN - 1], [C(0, 7), C(N - 1, 7)], [C(1, 1), C(3, 3)], [C(2, N - 1), C(N - 1, 2), C(7, 7)]]
    return corners + edges + near + both


@pytest.mark.parametrize("tag", TAGS)
def test_leaves_at_the_ring(engines, tag):
    for name, root in (("empty", dc.root_of([])), ("second", dc.roots()["second"])):
        cells = [cs for cs in _border_leaves() if all(root[0][c] == 0 for c in cs)]
        assert len(cells) >= 26
        _compare(engines[tag], root, cells, f"{tag}, {name} root, border leaves")


def _fill(count):
    return {0: "full", 1: "one"}.get(count % 16)


@pytest.mark.parametrize("tag", TAGS)
def test_conv1_chunks_and_conv2_tile_counts(engines, shape_cases, tag):
    R = dc.roots()
    picked, seen3, seen2 = {k: [] for k in R}, set(), set()
    for _, k, cells in shape_cases:
        rc, tc = dc.region_counts(cells), dc.tile_counts(cells)
        key3, key2 = (tc[2], _fill(rc[2])), (tc[1], _fill(rc[1]))
        take = False
        if tc[2] in (1, 4, 5, 8, 12, 14) and key3[1] and key3 not in seen3:
            seen3.add(key3); take = True
        if tc[1] in (1, 2, 3, 5, 7) and key2[1] and key2 not in seen2:
            seen2.add(key2); take = True
        if take:
            picked[k].append(cells)
    # the last tile full at every count; one cell in it wherever such a region exists (tests/delta_cases.py says where not:
    # a single tile is at least a corner window, and no leaf with 17 cells was found at conv2 or conv3)
    assert {(t, "full") for t in (1, 4, 5, 8, 12, 14)} <= seen3 and {(t, "one") for t in (4, 5, 8, 12, 14)} <= seen3
    assert {(t, "full") for t in (1, 2, 3, 5, 7)} <= seen2 and {(t, "one") for t in (3, 5, 7)} <= seen2
    for k, cells in picked.items():
        if cells:
            _compare(engines[tag], R[k], cells, f"{tag}, root {k}, tile counts")


def test_no_changed_cell_one_changed_cell_and_nine(engines):
    eng = engines["ring"]
    empty = dc.root_of([])
    _compare(eng, empty, [[]], "the empty board", want_path=[0])
    for root in (dc.root_of([0]), dc.root_of([C(7, 7), NN - 1]), dc.roots()["mid"]):
        _compare(eng, root, [[]], "the root as its own leaf", want_path=[dc.tile_counts([root[2]])[2]])
    nine = [C(7, 6 + j) for j in range(3)] + [C(8, 6 + j) for j in range(3)] + [C(9, 6 + j) for j in range(3)]
    _compare(eng, empty, [nine], "nine changed cells", tiles=MAX_TILES, want_path=[-1])


@pytest.mark.parametrize("tag", TAGS)
def test_full_corner_and_interior_in_one_launch_twice(engines, tag):
    empty = dc.root_of([])
    nine = [C(3, 2 + j) for j in range(3)] + [C(4, 2 + j) for j in range(3)] + [C(5, 2 + j) for j in range(3)]
    cells = [nine, [0], [C(7, 7)], [NN - 1], [C(8, 9), C(7, 5)], [C(0, 7)]]
    assert len(cells) == SLOTS
    path = [-1] + [dc.tile_counts(cs)[2] for cs in cells[1:]]
    a = _compare(engines[tag], empty, cells, f"{tag}, mixed launch", tiles=MAX_TILES, want_path=path)
    # again, and then with the boards in other workgroups: LDS holds another board's values at entry
    b = _compare(engines[tag], empty, cells, f"{tag}, mixed launch again", tiles=MAX_TILES, want_path=path)
    c = _compare(engines[tag], empty, cells[::-1], f"{tag}, mixed launch reversed", tiles=MAX_TILES, want_path=path[::-1])
    for x, y, z in zip(a[:3], b[:3], c[:3]):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z[::-1]))


@pytest.mark.parametrize("tiles", [0, 2])
def test_lockstep_from_an_edge_position(weight_sets, tiles):
    """6 slots x 24 simulations from a position on the left edge, at the default threshold and at 2 tiles (an edge footprint is two
    tiles: border leaves stay on the delta path, the others are evaluated in full by the same launch)"""
    S, G, seed, max_plies = 24, SLOTS, 1514, 7
    sd = weight_sets["ring" if tiles == 0 else "negative"]
    start = _stack([dc.root_of([C(7, 0), C(6, 0), C(8, 1), C(7, 1)])])
    on = _lockstep(sd, True, S, G, G, seed, max_plies, start, tiles)
    off = _lockstep(sd, False, S, G, G, seed, max_plies, start, tiles)
    what = f"edge position, threshold {tiles or MAX_TILES}"
    _assert_switch(on, off, what)
    _assert_oracle(on, _oracle_games(sd, S, start, G, seed, max_plies), what)
    _assert_counters(on, what)
    assert on["st"]["delta"] > 0
    if tiles:
        assert not any(on["st"]["by_tiles"][tiles + 1:])
