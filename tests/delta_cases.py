"""The shapes k_trunk_delta<15> is tested at (csrc/az_delta.h): a deterministic set of (root, leaf cells) cases for
net_eval_delta.  A leaf is a root plus 1 to 8 stones played alternately; its changed cells are those stones, and the kernel runs
conv1 / conv2 / conv3 on the 16-cell tiles of their clipped 3x3 / 5x5 / 7x7 windows, conv1 in chunks of 4 tiles, conv2 in chunks of
4 (template 4) or 1 .. 2 (template 2), conv3 in chunks of 4 / 3 / 2 / 1.

The cases are built against conditions, not sampled: a fixed list of targets (a layer and the cell counts its region may have),
each met by a seeded local search over sets of at most 8 free cells of a root, and a few sets built by hand whose structure says
why they are extreme (12 and 13 conv2 tiles, the 224-cell maximum of conv3, corners and edges at once).  tests/test_delta_shapes_cpu.py states the conditions as
assertions on the finished set.  No GPU and no engine needed: the search counts with integer bit masks, region_counts (what the
tests use) with a plain numpy union."""
import numpy as np

N = 15
NN = N * N
MAX_CHANGED = 8                       # az_delta.h: DELTA_MAX_CHANGED
C = lambda r, c: r * N + c


# ---------------------------------------------------------------------------------------------------------------------
# positions
# ---------------------------------------------------------------------------------------------------------------------
def root_of(cells, first=1):
    """the position after `cells` were played alternately, `first` moving first: (board, player to move, last)"""
    b = np.zeros(NN, np.uint8)
    for j, c in enumerate(cells):
        b[c] = first if j % 2 == 0 else 3 - first
    return b, first if len(cells) % 2 == 0 else 3 - first, (cells[-1] if cells else -1)


def leaf_of(root, cells):
    """the root plus `cells` played alternately by the root's mover and the opponent"""
    b, pl, last = root[0].copy(), root[1], root[2]
    for c in cells:
        assert b[c] == 0
        b[c] = pl
        pl, last = 3 - pl, c
    return b, pl, last


def roots():
    """the empty board, the 30-stone mid-game root of tests/test_delta_eval_gpu.py (player 1 to move), and a five-stone root
    with player 2 to move"""
    mid = root_of([int(c) for c in np.random.RandomState(1507).permutation(NN)[:30]])
    return {"empty": root_of([]), "mid": mid, "second": root_of([C(7, 7), C(6, 8), C(8, 6), C(2, 12), C(12, 1)])}


# ---------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------
def region_counts(cells):
    """cells of the conv1 / conv2 / conv3 regions of a leaf whose changed cells are `cells`: the union of the clipped windows"""
    out = []
    for radius in (1, 2, 3):
        m = np.zeros((N, N), bool)
        for ch in cells:
            r, c = divmod(int(ch), N)
            m[max(0, r - radius):r + radius + 1, max(0, c - radius):c + radius + 1] = True
        out.append(int(m.sum()))
    return tuple(out)


def tile_counts(cells):
    return tuple((x + 15) // 16 for x in region_counts(cells))


def conv2_chunks(t2):
    """k_trunk_delta's conv2 loop: [(template, tiles of the chunk), ...]"""
    out, t0 = [], 0
    while t0 < t2:
        c = t2 - t0
        if c > 2:
            out.append((4, min(c, 4))); t0 += 4
        else:
            out.append((2, c)); t0 += 2
    return out


def conv3_chunks(t3):
    """... and its conv3 loop: the template is the chunk's tile count"""
    return [min(4, t3 - t0) for t0 in range(0, t3, 4)]


def _window_masks():
    out = []
    for radius in (1, 2, 3):
        row = []
        for ch in range(NN):
            r0, c0 = divmod(ch, N)
            m = 0
            for r in range(max(0, r0 - radius), min(N - 1, r0 + radius) + 1):
                for c in range(max(0, c0 - radius), min(N - 1, c0 + radius) + 1):
                    m |= 1 << (r * N + c)
            row.append(m)
        out.append(row)
    return out


_WIN = _window_masks()


def _count(cells, layer):
    m = 0
    for ch in cells:
        m |= _WIN[layer][ch]
    return bin(m).count("1")


# ---------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------
def _search(rs, free, layer, want, restarts=60, steps=600):
    """at most 8 cells of `free` whose region of `layer` has a cell count in `want`, or None: local search from seeded starts.
    A step moves a cell anywhere or to a neighbouring cell, adds one or drops one, and is kept unless it leads away."""
    free_set, lo, hi = set(free), min(want), max(want)
    score = lambda cells: (lambda n: 0 if n in want else min(abs(n - lo), abs(n - hi)))(_count(cells, layer))
    for _ in range(restarts):
        cur = [int(c) for c in rs.choice(free, int(rs.randint(1, MAX_CHANGED + 1)), replace=False)]
        s = score(cur)
        for _ in range(steps):
            if s == 0:
                return cur
            new, move = list(cur), int(rs.randint(4))
            i = int(rs.randint(len(new)))
            if move == 0:
                new[i] = int(rs.choice(free))
            elif move == 1:
                r, c = divmod(new[i], N)
                r, c = r + int(rs.randint(-2, 3)), c + int(rs.randint(-2, 3))
                if not (0 <= r < N and 0 <= c < N):
                    continue
                new[i] = r * N + c
            elif move == 2 and len(new) < MAX_CHANGED:
                new.append(int(rs.choice(free)))
            elif move == 3 and len(new) > 1:
                del new[i]
            else:
                continue
            if len(set(new)) != len(new) or not set(new) <= free_set:
                continue
            t = score(new)
            if t <= s:
                cur, s = new, t
        if s == 0:
            return cur
    return None


def _targets():
    """[(what, layer, cell counts)]: every tile count the search serves, and the fills of the last tile -- `full` = no junk lane
    (cells % 16 == 0), `one` = fifteen junk lanes (cells % 16 == 1).  The fills that are missing:
      a single tile holding one cell, at every layer: the smallest window is a corner's, 4 / 9 / 16 cells;
      conv1: 5 full tiles are 80 cells, 8 windows hold at most 8 x 9 = 72;
      conv2: 13 full tiles are 208 cells, 8 windows hold at most 8 x 25 = 200; 17 cells (two tiles, one cell in the last) were
             found by no search, this one at 300 restarts included;
      conv3: 17 cells likewise; 14 full tiles are 224 cells, the most there is (_built), 15 tiles are out of reach."""
    out = []
    for layer, name, tmax, full, one in ((0, "conv1", 5, range(1, 5), range(2, 6)), (1, "conv2", 13, range(1, 13), range(3, 14)),
                                         (2, "conv3", 14, range(1, 15), range(3, 15))):
        for t in range(2 if layer == 2 else 1, tmax + 1):               # (one conv3 tile is a corner window: 16 cells, full)
            out.append((f"{name}: {t} tiles, the last one in part", layer, set(range(16 * (t - 1) + 2, 16 * t))))
        out += [(f"{name}: {t} tiles, the last one full", layer, {16 * t}) for t in full]
        out += [(f"{name}: {t} tiles, one cell in the last", layer, {16 * (t - 1) + 1}) for t in one]
    return out


def _built():
    """sets built by hand: [(what, cells)]"""
    grid = [C(r, c) for r in (2, 7, 12) for c in (2, 7, 12)]                 # nine disjoint 5x5 windows tile the board
    return [
        # conv3's maximum with 8 changed cells: rows 0, 7 and 14 need windows centred in three disjoint row bands, and a row
        # takes three windows of 7 columns to span 15, so all 225 cells need nine.  Two full rows of three and two windows on
        # row 7 leave out the cell (7, 14): 224 cells, 14 tiles, the last one full.
        ("conv3: 224 cells, the most 8 changed cells reach", [C(3, 3), C(3, 7), C(3, 11), C(11, 3), C(11, 7), C(11, 11), C(7, 3), C(7, 10)]),
        ("conv2: 13 tiles, eight disjoint 5x5 windows, the centre one left out", [c for c in grid if c != C(7, 7)]),
        ("conv2: 13 tiles, eight disjoint 5x5 windows, a corner one left out", [c for c in grid if c != C(2, 2)]),
        ("conv2: 12 tiles, seven disjoint 5x5 windows and one two columns into its neighbour",
         [c for c in grid if c not in (C(12, 7), C(12, 12))] + [C(12, 5)]),
        ("all four corners and all four edges", [0, N - 1, NN - N, NN - 1, C(0, 7), C(7, 0), C(7, N - 1), C(N - 1, 7)]),
        ("all four corners", [0, N - 1, NN - N, NN - 1]),
    ]


TRIPLES = 64                          # distinct (t1, t2, t3) the set is filled up to


def cases(seed=1511):
    """[(what, root name, leaf cells)], the same list on every call"""
    rs = np.random.RandomState(seed)
    R = roots()
    names = list(R)
    free = {k: [c for c in range(NN) if R[k][0][c] == 0] for k in names}
    out = []
    for what, cells in _built():                                            # on every root that has the cells free
        out += [(what, k, cells) for k in names if all(R[k][0][c] == 0 for c in cells)]
    for i, (what, layer, want) in enumerate(_targets()):                    # the roots in turn; the next one where a search finds nothing
        for j in range(len(names)):
            k = names[(i + j) % len(names)]
            cells = _search(rs, free[k], layer, want)
            if cells is not None:
                out.append((what, k, cells))
                break
        else:
            raise AssertionError(f"no set of at most {MAX_CHANGED} cells found for: {what}")
    for k in names:                                                         # every depth and so both parities from every root
        for depth in range(1, MAX_CHANGED + 1):
            a = int(rs.choice(free[k])); r, c = divmod(a, N)
            near = [x for x in free[k] if x != a and max(abs(x // N - r), abs(x % N - c)) <= 3 + depth % 4]
            out.append((f"depth {depth}", k, [a] + [int(x) for x in rs.choice(near, depth - 1, replace=False)]))
    seen = {tile_counts(cells) for _, _, cells in out}
    for i in range(100000):                                                 # distinct shapes: seeded sets that bring a new triple
        if len(seen) >= TRIPLES:
            break
        k = names[i % len(names)]
        cells = [int(c) for c in rs.choice(free[k], int(rs.randint(2, MAX_CHANGED + 1)), replace=False)]
        if i % 2:                                                           # ... half of them pulled together
            r, c = divmod(cells[0], N)
            near = [x for x in free[k] if max(abs(x // N - r), abs(x % N - c)) <= 4]
            cells = [int(x) for x in rs.choice(near, min(len(cells), len(near)), replace=False)]
        if tile_counts(cells) not in seen:
            seen.add(tile_counts(cells))
            out.append(("a shape of its own", k, cells))
    return out
