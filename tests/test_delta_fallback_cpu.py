"""The lists of a position k_trunk_delta<15> evaluates in full (csrc/az_delta.h, delta_lists_full), restated on the
host by az_delta_lists_full with the functions the kernel uses, against numpy.  No GPU needed."""
import ctypes as C

import numpy as np

from alphazero_piskvorky_amd import _capi

N = 15
NN, PW = N * N, N + 2
MAXM, PP = 240, PW * PW


def _full_lists():
    wpos = np.zeros((3, MAXM), np.uint16); cell = np.zeros((3, MAXM), np.uint16)
    halo = np.zeros((2, PP), np.uint16); cnt = np.zeros(5, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _capi.lib().az_delta_lists_full(N, p(wpos), p(cell), p(halo), p(cnt)) == 0
    return wpos, cell, halo, cnt


def _window_counts(changed):
    ch = np.asarray(changed, np.uint8)
    wpos = np.zeros((3, MAXM), np.uint16); cell = np.zeros((3, MAXM), np.uint16)
    halo = np.zeros((2, PP), np.uint16); cnt = np.zeros(5, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _capi.lib().az_delta_lists(N, len(ch), p(ch), p(wpos), p(cell), p(halo), p(cnt)) == 0
    return int(cnt[3]), int(cnt[4])


def test_window_fragments_a_thread_keeps_in_registers_are_bounded():
    """k_trunk_delta loads the windows with plane = wave and the list positions over the 64 lanes, in 5 rounds: a thread holds at
    most 5 float4 of conv1's image and 2 x 5 = 10 of conv2's, and no list is longer than the rounds reach"""
    from tests import delta_cases as dc
    rounds = lambda n: (n + 63) // 64
    seen = set()
    for what, _, cells in dc.cases():
        n3, n4 = _window_counts(cells)
        assert 0 < n3 <= n4 <= PP and rounds(n3) <= 5 and 2 * rounds(n4) <= 10, what
        seen.add(rounds(n4))
    assert min(seen) <= 2 and max(seen) == 5                          # one changed cell: at most 81 positions; the widest: every round
    # 8 scattered cells: the 9x9 windows cover the whole padded image, 16 x 289 / 512 rounds up to 10 float4 per thread
    scattered = [r * N + c for r in (3, 11) for c in (2, 6, 10, 13)]
    n3, n4 = _window_counts(scattered)
    assert n4 == PP and 2 * rounds(n4) == 10 == -(-16 * PP // 512)
    assert n3 == 14 * 17 and rounds(n3) <= 5                        # the 7x7 windows leave out padded rows 0, 8 and 16


def test_the_export_is_declared_and_refuses_other_sizes():
    assert "az_delta_lists_full" in _capi.EXPORTS and hasattr(_capi.lib(), "az_delta_lists_full")
    z = np.zeros(2 * PP, np.uint16); cnt = np.zeros(5, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _capi.lib().az_delta_lists_full(9, p(z), p(z), p(z), p(cnt)) != 0
    assert _capi.lib().az_delta_lists_full(N, None, p(z), p(z), p(cnt)) != 0


def test_every_layer_lists_the_225_cells_in_ascending_position():
    wpos, cell, halo, cnt = _full_lists()
    assert cnt.tolist() == [NN, NN, NN, 0, 0]                         # no window of the base images is read
    assert [(int(c) + 15) // 16 for c in cnt[:3]] == [15, 15, 15]
    r, c = np.divmod(np.arange(NN), N)
    want = ((r + 1) * PW + (c + 1)).astype(np.uint16)
    assert np.all(np.diff(want.astype(np.int64)) > 0)
    for l in range(3):
        assert np.array_equal(wpos[l, :NN], want), l
        assert np.array_equal(cell[l, :NN], np.arange(NN, dtype=np.uint16)), l


def test_the_last_tile_holds_one_cell_and_fifteen_junk_lanes():
    wpos, cell, halo, cnt = _full_lists()
    assert NN % 16 == 1 and MAXM - NN == 15
    last = (N * PW + N)                                               # cell (14, 14)
    for l in range(3):
        assert wpos[l, NN - 1] == last
        assert np.all(wpos[l, NN:] == last), l                        # junk lanes repeat the last position ...
        assert np.all(cell[l, NN:] == 0xFFFF), l                      # ... and are marked
        assert not np.any(cell[l, :NN] == 0xFFFF)
    assert np.all(halo == 0xEEEE)                                     # the window lists are not written
