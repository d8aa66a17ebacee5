"""Delta evaluation (csrc/az_delta.h): the integer logic that turns a leaf's changed cells into the three lists of
16-cell tiles conv1 / conv2 / conv3 run on, and into the two window lists of the base images copied into LDS -- restated on the
host by az_delta_lists with the functions the kernel uses.  No GPU needed.

For every set of changed cells: region l (l = 0, 1, 2) is the union of the (2l + 3) x (2l + 3) windows round the changed cells,
clipped to the board; every region cell sits in exactly one tile lane at its own padded position; the lanes that fill the last
tile are marked junk and repeat a cell of the region; nothing is written behind the last tile; and the windows hold every
position a listed tile reads (the 3 x 3 neighbourhood of every lane, padding ring included)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from alphazero_piskvorky_amd import _capi

N = 15
NN, PW = N * N, N + 2
MAXM, PP = 240, PW * PW
NEW = ["az_set_delta_eval", "az_get_delta_eval", "az_delta_max_tiles", "az_delta_stats", "az_net_eval_delta", "az_delta_lists"]


def _lists(changed):
    ch = np.asarray(changed, np.uint8)
    wpos = np.zeros((3, MAXM), np.uint16); cell = np.zeros((3, MAXM), np.uint16)
    halo = np.zeros((2, PP), np.uint16); cnt = np.zeros(5, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _capi.lib().az_delta_lists(N, len(ch), p(ch) if len(ch) else None, p(wpos), p(cell), p(halo), p(cnt))
    assert rc == 0
    return wpos, cell, halo, cnt


def _window(changed, radius, lo, hi):
    """positions (r, c) with lo <= r, c <= hi within `radius` (Chebyshev) of a changed cell"""
    out = set()
    for ch in changed:
        r0, c0 = divmod(int(ch), N)
        for r in range(max(lo, r0 - radius), min(hi, r0 + radius) + 1):
            for c in range(max(lo, c0 - radius), min(hi, c0 + radius) + 1):
                out.add((r, c))
    return out


def _check(changed):
    wpos, cell, halo, cnt = _lists(changed)
    regions = []
    for l in range(3):
        want = _window(changed, l + 1, 0, N - 1)
        n = int(cnt[l]); tiles = (n + 15) // 16
        assert n == len(want), (changed, l)
        cells = [int(x) for x in cell[l, :n]]
        assert len(set(cells)) == n and {divmod(x, N) for x in cells} == want, (changed, l)      # every region cell exactly once
        for m in range(n):
            r, c = divmod(cells[m], N)
            assert wpos[l, m] == (r + 1) * PW + c + 1
        for m in range(n, tiles * 16):                                   # junk lanes: marked, and a twin of a region cell
            assert cell[l, m] == 0xFFFF and wpos[l, m] in set(int(x) for x in wpos[l, :n])
        assert np.all(wpos[l, tiles * 16:] == 0xEEEE) and np.all(cell[l, tiles * 16:] == 0xEEEE)
        regions.append(want)
    for h in range(2):                                                   # the windows: padded positions within 3 / 4, ring included
        want = {(r + 1) * PW + c + 1 for r, c in _window(changed, h + 3, -1, N)}
        n = int(cnt[3 + h])
        got = [int(x) for x in halo[h, :n]]
        assert len(set(got)) == n and set(got) == want and np.all(halo[h, n:] == 0xEEEE), (changed, h)
        # ... which is every position the layer's lanes read: conv2 reads the conv1 image, conv3 the conv2 image
        reads = {(r + 1 + dr) * PW + c + 1 + dc for r, c in regions[h + 1] for dr in (-1, 0, 1) for dc in (-1, 0, 1)}
        assert reads <= want
    return cnt


def test_exports():
    L = _capi.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_capi.EXPORTS)


def test_every_single_cell():
    for ch in range(NN):
        cnt = _check([ch])
        r, c = divmod(ch, N)
        side = lambda x, k: min(N - 1, x + k) - max(0, x - k) + 1
        assert [int(x) for x in cnt[:3]] == [side(r, k) * side(c, k) for k in (1, 2, 3)]      # the clipped 3x3 / 5x5 / 7x7 windows


def test_no_changed_cell():
    wpos, cell, halo, cnt = _lists([])
    assert not cnt.any() and np.all(wpos == 0xEEEE) and np.all(cell == 0xEEEE) and np.all(halo == 0xEEEE)


def test_pairs_and_triples():
    rs = np.random.RandomState(1505)
    corners = [0, N - 1, NN - N, NN - 1]
    edges = [7, 7 * N, 7 * N + N - 1, NN - N + 7]
    sets = [list(p) for p in itertools.combinations(corners + edges, 2)]                  # corners and edges, far apart
    sets += [[a, a + d] for a in (0, 16, 7 * N + 7, 7 * N - 8) for d in (1, N, N + 1, 2, 3 * N, 6, 7, 7 * N)]    # adjacent ... just disjoint
    while len(sets) < 150:                                                                # seeded pairs: overlapping and not
        a = int(rs.randint(NN)); r, c = divmod(a, N)
        k = int(rs.choice([1, 2, 3, 6, 7, 14]))
        b = min(N - 1, max(0, r + rs.randint(-k, k + 1))) * N + min(N - 1, max(0, c + rs.randint(-k, k + 1)))
        if b != a:
            sets.append([a, b])
    while len(sets) < 300:                                                                # seeded triples, clustered and scattered
        if rs.rand() < 0.5:
            sets.append([int(x) for x in rs.choice(NN, 3, replace=False)])
        else:
            a = int(rs.randint(NN)); r, c = divmod(a, N)
            near = {min(N - 1, max(0, r + rs.randint(-3, 4))) * N + min(N - 1, max(0, c + rs.randint(-3, 4))) for _ in range(4)} - {a}
            sets.append([a] + sorted(near)[:2])
    for s in sets:
        _check(s)
    _check(list(range(0, 8)))                                                             # the most the path takes: 8 changed cells
    _check([0, N - 1, NN - N, NN - 1, 7 * N + 7, 3 * N + 3, 11 * N + 11, 3 * N + 11])     # ... spread over the board


def test_refuses_what_the_kernel_never_builds():
    z = np.zeros(3 * MAXM, np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cnt = np.zeros(5, np.int32)
    ch = np.arange(9, dtype=np.uint8)
    assert _capi.lib().az_delta_lists(N, 9, p(ch), p(z), p(z), p(z), p(cnt)) != 0         # more than 8 changed cells
    assert _capi.lib().az_delta_lists(9, 1, p(ch), p(z), p(z), p(z), p(cnt)) != 0          # no delta kernels at 9x9
    bad = np.array([NN], np.uint8)
    assert _capi.lib().az_delta_lists(N, 1, p(bad), p(z), p(z), p(z), p(cnt)) != 0         # a cell off the board
