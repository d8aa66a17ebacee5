"""conv1 recomputed on the conv3 tile list (csrc/az_delta.h): the integer facts the kernel relies on, on the host.

Lists: k_trunk_delta<15> runs conv1 on list 2 and zeroes conv1's image at the ring positions within 3 of a changed cell, where it
used to copy list 3 from the base image.  So list 3 must be exactly list 2 (in order) plus those ring positions.
Changed cells: az_delta_changed restates delta_changed, the function of the 16 board words that replaced the kernel's LDS atomic,
and is held to a numpy XOR of the planes.  No GPU needed."""
import ctypes as C
import itertools

import numpy as np

from alphazero_piskvorky_amd import _capi
from tests import delta_cases as dc

N = 15
NN, PW = N * N, N + 2
MAXM, PP = 240, PW * PW
p = lambda a: a.ctypes.data_as(C.c_void_p)


def _lists(changed):
    ch = np.asarray(changed, np.uint8)
    wpos = np.zeros((3, MAXM), np.uint16); cell = np.zeros((3, MAXM), np.uint16)
    halo = np.zeros((2, PP), np.uint16); cnt = np.zeros(5, np.int32)
    assert _capi.lib().az_delta_lists(N, len(ch), p(ch) if len(ch) else None, p(wpos), p(cell), p(halo), p(cnt)) == 0
    return wpos, cell, halo, cnt


def _on_board(pos):
    r, c = divmod(int(pos), PW)
    return 1 <= r <= N and 1 <= c <= N


def _ring_within_3(changed):
    out = set()
    for pos in range(PP):
        r, c = divmod(pos, PW)
        if _on_board(pos):
            continue
        if any(max(abs(r - 1 - ch // N), abs(c - 1 - ch % N)) <= 3 for ch in changed):
            out.add(pos)
    return out


def _check_lists(changed):
    wpos, cell, halo, cnt = _lists(changed)
    l3 = [int(x) for x in halo[0, :cnt[3]]]
    l2 = [int(x) for x in wpos[2, :cnt[2]]]
    assert [x for x in l3 if _on_board(x)] == l2, changed                  # list 3 on the board == list 2, as a set and in order
    assert {x for x in l3 if not _on_board(x)} == _ring_within_3(changed), changed
    assert len(set(l3)) == len(l3)
    # every position conv2's lanes read is a cell conv1 computes or a ring position the kernel zeroes
    reads = {int(x) + dr * PW + dc for x in wpos[1, :cnt[1]] for dr in (-1, 0, 1) for dc in (-1, 0, 1)}
    assert reads <= set(l3), changed


def test_list_3_is_list_2_plus_the_ring_on_every_case():
    for _, _, cells in dc.cases():
        _check_lists(cells)


def test_list_3_is_list_2_plus_the_ring_on_cells_pairs_and_triples():
    for ch in range(NN):
        _check_lists([ch])
    rs = np.random.RandomState(1513)
    sets = []
    while len(sets) < 150:
        a = int(rs.randint(NN)); r, c = divmod(a, N)
        k = int(rs.choice([1, 2, 3, 6, 7, 14]))
        b = min(N - 1, max(0, r + rs.randint(-k, k + 1))) * N + min(N - 1, max(0, c + rs.randint(-k, k + 1)))
        if b != a:
            sets.append([a, b])
    while len(sets) < 300:
        sets.append([int(x) for x in rs.choice(NN, 3, replace=False)])
    for s in sets:
        _check_lists(s)


# ---------------------------------------------------------------------------------------------------------------------
# az_delta_changed
# ---------------------------------------------------------------------------------------------------------------------
def _words(mask):
    """bit c of word c // 64 for every cell of a boolean [NN] mask"""
    w = np.zeros(4, np.uint64)
    for c in np.flatnonzero(mask):
        w[c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return w


def _changed(leaf, root):
    """(rc, count, cells, parity) of a leaf (board, player to move, last) against a root (board, player to move, last)"""
    lb, lpl, llast = leaf
    rb, rpl, _ = root
    lw = np.concatenate([_words(lb == lpl), _words(lb == 3 - lpl)])
    bw = np.concatenate([_words(rb == 1), _words(rb == 2)])
    ch = np.full(8, 0xAA, np.uint8); cnt = np.zeros(1, np.int32); par = np.zeros(1, np.int32)
    rc = _capi.lib().az_delta_changed(N, p(lw), p(bw), int(rpl), int(llast), p(ch), p(cnt), p(par))
    return rc, int(cnt[0]), ch, int(par[0])


def _expect(leaf, root):
    """numpy: the planes of the leaf XOR the root's planes seen from the leaf's side to move, and the last-move cell"""
    lb, lpl, llast = leaf
    rb, rpl, _ = root
    par = (int(np.count_nonzero(lb)) - int(np.count_nonzero(rb))) & 1
    me = rpl if par == 0 else 3 - rpl                     # the colour that is "me" in the base of this parity
    diff = ((lb == lpl) ^ (rb == me)) | ((lb == 3 - lpl) ^ (rb == 3 - me))
    if llast >= 0:
        diff[llast] = True
    return [int(c) for c in np.flatnonzero(diff)], par


def _check_changed(leaf, root):
    rc, cnt, ch, par = _changed(leaf, root)
    cells, wpar = _expect(leaf, root)
    assert rc == 0
    assert cnt == len(cells) and par == wpar, (cells, cnt, par)
    k = min(cnt, 8)
    assert ch[:k].tolist() == cells[:k] and np.all(ch[k:] == 0xFF), (cells, ch)
    return cnt


def test_export():
    assert "az_delta_changed" in _capi.EXPORTS and hasattr(_capi.lib(), "az_delta_changed")


def test_changed_cells_equal_the_numpy_xor_on_every_case():
    R = dc.roots()
    for _, k, cells in dc.cases():
        leaf = dc.leaf_of(R[k], cells)
        cnt = _check_changed(leaf, R[k])
        assert cnt == len(set(cells))                     # the leaf's stones; the last move is one of them


def test_parities_players_and_the_last_move():
    for first in (1, 2):                                  # both players to move at the root
        root = dc.root_of([dc.C(7, 7), dc.C(6, 8), dc.C(8, 6)], first)
        free = [c for c in range(NN) if root[0][c] == 0]
        for depth in range(0, 9):                         # both parities; 0 .. 8 stones
            leaf = dc.leaf_of(root, free[:depth])
            cnt = _check_changed(leaf, root)
            # the root as its own leaf: its last move lies on a stone that did not change -- one changed cell
            assert cnt == (depth if depth else 1)
        b, pl, _ = root
        assert _check_changed((b, pl, -1), root) == 0     # no last move: nothing changed
        # the last move on a changed stone counts once, on an unchanged stone once more
        leaf = dc.leaf_of(root, free[:2])
        assert _check_changed((leaf[0], leaf[1], free[0]), root) == 2
        assert _check_changed((leaf[0], leaf[1], dc.C(7, 7)), root) == 3


def test_counts_0_1_8_and_9():
    root = dc.root_of([])
    assert _check_changed(root, root) == 0
    for count in (1, 8, 9):
        cells = [dc.C(2 + j, 3 + (j * 4) % 11) for j in range(count)]
        leaf = dc.leaf_of(root, cells)
        assert _check_changed(leaf, root) == count        # 9 is reported (the first 8 listed) and selects the full path


def test_cells_in_every_word():
    root = dc.root_of([])
    for cells in ([0], [63], [64], [63, 64], [127, 128], [191, 192], [224], [0, 63, 64, 128, 192, 224], [223, 224]):
        assert _check_changed(dc.leaf_of(root, cells), root) == len(cells)
    mid = dc.roots()["mid"]
    free = [c for c in range(NN) if mid[0][c] == 0]
    for cells in itertools.combinations([free[0], free[-1]] + [c for c in free if c in (63, 64, 65, 127, 128, 191, 192, 193)][:3], 3):
        _check_changed(dc.leaf_of(mid, list(cells)), mid)


def test_bad_arguments():
    L = _capi.lib()
    w = np.zeros(8, np.uint64); ch = np.zeros(8, np.uint8); a = np.zeros(1, np.int32); b = np.zeros(1, np.int32)
    assert L.az_delta_changed(N, p(w), p(w), 1, -1, p(ch), p(a), p(b)) == 0
    assert L.az_delta_changed(9, p(w), p(w), 1, -1, p(ch), p(a), p(b)) != 0           # no delta kernels at 9x9
    assert L.az_delta_changed(N, None, p(w), 1, -1, p(ch), p(a), p(b)) != 0
    assert L.az_delta_changed(N, p(w), None, 1, -1, p(ch), p(a), p(b)) != 0
    assert L.az_delta_changed(N, p(w), p(w), 1, -1, None, p(a), p(b)) != 0
    assert L.az_delta_changed(N, p(w), p(w), 1, -1, p(ch), None, p(b)) != 0
    assert L.az_delta_changed(N, p(w), p(w), 1, -1, p(ch), p(a), None) != 0
    assert L.az_delta_changed(N, p(w), p(w), 0, -1, p(ch), p(a), p(b)) != 0           # players are 1 and 2
    assert L.az_delta_changed(N, p(w), p(w), 3, -1, p(ch), p(a), p(b)) != 0
    assert L.az_delta_changed(N, p(w), p(w), 1, NN, p(ch), p(a), p(b)) != 0           # a last move off the board
    assert L.az_delta_changed(N, p(w), p(w), 1, -2, p(ch), p(a), p(b)) != 0
