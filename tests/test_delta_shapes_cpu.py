"""What tests/delta_cases.py has to contain, as assertions: the tile counts, chunk sequences and last-tile fills of conv1 / conv2 /
conv3 at which tests/test_delta_shapes_gpu.py holds k_trunk_delta<15> (csrc/az_delta.h) to net_eval and the oracle.  No GPU
needed.  The counts come from az_delta_lists, the kernel's own host restatement, and are cross-checked against a plain numpy
union of the clipped windows; a change to the generator that loses a shape fails here, not silently on the GPU."""
import ctypes as C

import numpy as np
import pytest

from alphazero_piskvorky_amd import _capi
from tests import delta_cases as dc

N, NN = dc.N, dc.NN
MAXM, PP = 240, (N + 2) * (N + 2)


def _kernel_counts(changed):
    ch = np.asarray(changed, np.uint8)
    wpos = np.zeros((3, MAXM), np.uint16); cell = np.zeros((3, MAXM), np.uint16)
    halo = np.zeros((2, PP), np.uint16); cnt = np.zeros(5, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _capi.lib().az_delta_lists(N, len(ch), p(ch), p(wpos), p(cell), p(halo), p(cnt)) == 0
    for l in range(3):                                   # the junk lanes fill the last tile and nothing else
        n, t = int(cnt[l]), (int(cnt[l]) + 15) // 16
        assert np.all(cell[l, n:16 * t] == 0xFFFF) and np.all(cell[l, 16 * t:] == 0xEEEE) and not np.any(cell[l, :n] == 0xFFFF)
    return tuple(int(x) for x in cnt[:3])


@pytest.fixture(scope="module")
def shapes():
    """[(root name, cells, (cells of conv1, conv2, conv3), (tiles of conv1, conv2, conv3))] of every case"""
    out = []
    for what, k, cells in dc.cases():
        cnt = _kernel_counts(cells)
        assert cnt == dc.region_counts(cells), f"{what}: az_delta_lists and the numpy union of the windows disagree"
        out.append((k, cells, cnt, tuple((x + 15) // 16 for x in cnt)))
    return out


def test_the_generator_is_deterministic_and_its_leaves_are_legal():
    a, b = dc.cases(), dc.cases()
    assert a == b and len(a) <= 200                      # ... and small enough for a GPU test of a few seconds
    R = dc.roots()
    assert list(R) == ["empty", "mid", "second"]
    assert not R["empty"][0].any() and R["empty"][1:] == (1, -1)
    assert np.count_nonzero(R["mid"][0]) == 30 and R["mid"][1] == 1
    assert R["second"][1] == 2 and np.count_nonzero(R["second"][0]) % 2 == 1
    for what, k, cells in a:
        assert 1 <= len(cells) <= dc.MAX_CHANGED and len(set(cells)) == len(cells), what
        assert all(0 <= c < NN and R[k][0][c] == 0 for c in cells), what
        leaf = dc.leaf_of(R[k], cells)
        assert np.count_nonzero(leaf[0] != R[k][0]) == len(cells) and leaf[2] == cells[-1]
        assert leaf[1] == (R[k][1] if len(cells) % 2 == 0 else 3 - R[k][1])


def test_conv1_tile_counts_and_fills(shapes):
    cnt = {s[2][0] for s in shapes}
    assert {s[3][0] for s in shapes} == {1, 2, 3, 4, 5}                       # t1 = 5: a second chunk behind a chunk of 4
    assert 64 in cnt and 49 in cnt                                            # 4 tiles: mt_cnt == 4, last tile full / one cell
    assert 65 in cnt                                                          # 5 tiles, one cell in the last
    assert max(cnt) <= 72                                                     # 5 full tiles (80 cells) take more than 8 windows of 9
    for t in (1, 2, 3):
        assert 16 * t in cnt
    for t in (2, 3):
        assert 16 * (t - 1) + 1 in cnt


def test_conv2_tile_counts_and_chunk_sequences(shapes):
    t2s = {s[3][1] for s in shapes}
    assert t2s == set(range(1, 14))
    assert max(s[2][1] for s in shapes) == 200                                # eight disjoint 5x5 windows: the most there is
    assert 190 in {s[2][1] for s in shapes}                                   # seven and one two columns into its neighbour: 12 tiles
    seqs = {tuple(dc.conv2_chunks(t)) for t in t2s}
    for t in t2s:
        assert sum(c for _, c in dc.conv2_chunks(t)) == t
    # every last chunk of the loop behind zero, one and two chunks of 4; and a 2-template chunk of 1 behind three (t2 = 13)
    for last in ((4, 3), (4, 4), (2, 1), (2, 2)):
        for before in (0, 1, 2):
            assert tuple([(4, 4)] * before + [last]) in seqs, (before, last)
    assert ((4, 4), (4, 4), (4, 4), (2, 1)) in seqs
    # ... each of the four with a full last tile and with one cell in it
    fills = {(dc.conv2_chunks(s[3][1])[-1], s[2][1] % 16) for s in shapes}
    for last in ((4, 3), (4, 4), (2, 1), (2, 2)):
        assert (last, 0) in fills and (last, 1) in fills, last


def test_conv3_tile_counts_and_fills(shapes):
    assert {s[3][2] for s in shapes} == set(range(1, 15))
    # 15 tiles are out of reach: all 225 cells need nine windows (tests/delta_cases.py, _built); 224 are reached, by the set built for it
    assert max(s[2][2] for s in shapes) == 224
    built = [dc.C(3, 3), dc.C(3, 7), dc.C(3, 11), dc.C(11, 3), dc.C(11, 7), dc.C(11, 11), dc.C(7, 3), dc.C(7, 10)]
    assert any(sorted(s[1]) == sorted(built) and s[2][2] == 224 and s[3][2] == 14 for s in shapes)
    fills = {(dc.conv3_chunks(s[3][2])[-1], s[2][2] % 16) for s in shapes}
    for last in (1, 2, 3, 4):                                                 # the last chunk's template, its last tile full / one cell
        assert (last, 0) in fills and (last, 1) in fills, last
    # behind 0 .. 3 chunks of 4: every shift of the chunk's output pointer
    assert {tuple(dc.conv3_chunks(s[3][2])) for s in shapes} == {tuple([4] * q + ([r] if r else [])) for q in range(4) for r in range(5)
                                                                  if 0 < 4 * q + r <= 14}
    # the thresholds the GPU test moves between: above the default of 12 tiles
    assert {13, 14} <= {s[3][2] for s in shapes if len(s[1]) <= dc.MAX_CHANGED}


def test_changed_cells_parities_and_borders(shapes):
    assert {len(s[1]) for s in shapes} == set(range(1, 9))
    for k in ("empty", "mid", "second"):
        assert {len(s[1]) % 2 for s in shapes if s[0] == k} == {0, 1}, k
        assert sum(1 for s in shapes if s[0] == k) >= 30, k
    corners = {0, N - 1, NN - N, NN - 1}
    edge = lambda c: (c // N in (0, N - 1)) != (c % N in (0, N - 1))
    sides = lambda cs: {("r", c // N) for c in cs if c // N in (0, N - 1)} | {("c", c % N) for c in cs if c % N in (0, N - 1)}
    assert any(corners <= set(s[1]) and len(sides([c for c in s[1] if edge(c)])) == 4 for s in shapes)


def test_distinct_shapes(shapes):
    assert len({s[3] for s in shapes}) >= 60
