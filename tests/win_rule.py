"""The win rules (az_set_win_rule), restated in numpy for the tests.

Written from the definition in include/az_engine.h, not from the kernels.  FREESTYLE: the stone just placed wins when a run of k
OR MORE of the mover's stones goes through it.  EXACT (standard Gomoku): it wins when, in at least one of the four directions,
the MAXIMAL run through it is exactly k long; board edges end a run like an empty cell; an overline wins nothing.

The searches of tests/forced.py (plain and virtual-loss batches) and tests/solver.py (solver search, brute-force minimax) call a
module-level `wins_through`; `use_rule` points that name at the rule's test on both modules (solver.py imports the name), which
gives the exact-rule restatements without editing either file."""
import numpy as np

from oracle import oracle as orc
from tests import forced, solver
from tests.forced import wins_through as wins_freestyle        # the original, whatever the modules' name points at later

DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))
RULES = ("freestyle", "exact")


def run_through(board, a, n, dr, dc):
    """length of the maximal run of board[a]'s colour through cell a along (dr, dc)"""
    p, r, c = board[a], a // n, a % n
    cnt = 1
    for sgn in (1, -1):
        rr, cc = r + sgn * dr, c + sgn * dc
        while 0 <= rr < n and 0 <= cc < n and board[rr * n + cc] == p:
            cnt += 1
            rr, cc = rr + sgn * dr, cc + sgn * dc
    return cnt


def wins_exact(board, a, n, k):
    """the stone at cell a lies in a maximal run of exactly k in at least one direction"""
    return any(run_through(board, a, n, dr, dc) == k for dr, dc in DIRS)


def wins_fn(rule):
    assert rule in RULES
    return wins_exact if rule == "exact" else wins_freestyle


def use_rule(monkeypatch, rule):
    """the restatements of tests/forced.py and tests/solver.py under `rule` until the test ends (or the next call)"""
    fn = wins_fn(rule)
    monkeypatch.setattr(forced, "wins_through", fn)
    monkeypatch.setattr(solver, "wins_through", fn)
    return fn


def winner_scan(board, n, k, rule):
    """the whole board: 1 / 2 when that colour holds a winning run, 3 for a full board without one, 0 otherwise, -1 when both
    colours hold one.  Every maximal run is measured from its first stone."""
    assert rule in RULES
    board = np.asarray(board).reshape(-1)
    won = set()
    for a in np.flatnonzero(board):
        a = int(a)
        r, c = divmod(a, n)
        for dr, dc in DIRS:
            pr, pc = r - dr, c - dc
            if 0 <= pr < n and 0 <= pc < n and board[pr * n + pc] == board[a]:
                continue                                         # not the first stone of its run
            length = run_through(board, a, n, dr, dc)
            if (length == k) if rule == "exact" else (length >= k):
                won.add(int(board[a]))
    if len(won) == 2:
        return -1
    if won:
        return won.pop()
    return 0 if (board == 0).any() else 3


def replay(actions, n, k, rule):
    """Gomoku.apply_action / is_terminal / get_game_result for one action list (-1 ends it) from the empty board, X first, the
    winner sticky: (term_before bool[len], board uint8[nn], side to move, result)"""
    wins = wins_fn(rule)
    board, pl, res, term = np.zeros(n * n, np.uint8), 1, 0, []
    for a in actions:
        a = int(a)
        if a < 0:
            break
        term.append(res != 0)
        assert board[a] == 0
        board[a] = pl
        if res == 0:
            res = pl if wins(board, a, n, k) else (3 if not (board == 0).any() else 0)
        pl = 3 - pl
    return np.array(term, bool), board, pl, res


def result_after(board, player, actions, n, k, rule):
    """a game continued from `board` with `player` to move by `actions`: (plies until it ended, result); (len, 0) = not over"""
    wins = wins_fn(rule)
    b, pl = np.array(board, np.uint8), int(player)
    for i, a in enumerate(actions):
        a = int(a)
        assert b[a] == 0
        b[a] = pl
        if wins(b, a, n, k):
            return i + 1, pl
        if not (b == 0).any():
            return i + 1, 3
        pl = 3 - pl
    return len(actions), 0


def random_position(n, k, stones, seed):
    """tests.forced.random_position under the freestyle rule whatever the modules' name points at: a position without any run of
    k or more, so unfinished under both rules"""
    rs = np.random.RandomState(seed)
    while True:
        board, player, last = np.zeros(n * n, np.uint8), 1, -1
        for _ in range(stones):
            a = int(rs.choice(np.flatnonzero(board == 0)))
            board[a] = player
            if wins_freestyle(board, a, n, k):
                break
            player, last = 3 - player, a
        else:
            return board, player, last


def far_cells(n, count, avoid_rows):
    """`count` cells for the other colour, no two adjacent in any direction and none in `avoid_rows` or beside them"""
    rows = [r for r in (0, n - 1, 2, n - 3) if all(abs(r - x) >= 2 for x in avoid_rows)]
    out = []
    for i, r in enumerate(dict.fromkeys(rows)):
        out += [r * n + c for c in range(i % 2, n, 2)]
    assert len(out) >= count, (n, count, avoid_rows)
    return out[:count]


def gap_position(n, k, gap_at=None):
    """the mover (X) holds k of the k + 1 cells of a segment of row n // 2 that starts at column 0, the cell at index gap_at
    (default k // 2) empty; the opponent's k stones are far away.  Filling the gap makes a run of k + 1: a win under FREESTYLE,
    nothing under EXACT.  (board, player, last, gap cell)"""
    assert n >= k + 1
    gap_at = k // 2 if gap_at is None else gap_at
    r = n // 2
    board = np.zeros(n * n, np.uint8)
    for c in range(k + 1):
        if c != gap_at:
            board[r * n + c] = 1
    opp = far_cells(n, k, (r,))
    board[opp] = 2
    for a in np.flatnonzero(board):
        assert not wins_freestyle(board, int(a), n, k)
    return board, 1, opp[-1], r * n + gap_at


def overline_position(n, k):
    """legal under EXACT only: the mover (X) already holds the k + 1 cells at columns 0 .. k of row n // 2, an overline, and
    column k + 1 is empty.  Playing it makes k + 2 with k + 1 stones on ONE side of the new stone: the side's count reaches k.
    (board, player, last, the cell)"""
    assert n >= k + 2
    r = n // 2
    board = np.zeros(n * n, np.uint8)
    board[r * n:r * n + k + 1] = 1
    opp = far_cells(n, k + 1, (r,))
    board[opp] = 2
    assert winner_scan(board, n, k, "exact") == 0
    return board, 1, opp[-1], r * n + k + 1


def gap_logits(n, cells, level=4.0):
    lg = np.zeros(n * n, np.float32)
    lg[list(cells)] = level
    return lg


def opening(n, k):
    """a start position with gap patterns for both colours: X segments of k + 1 cells (index k // 2 empty) in rows 0, 4, ..,
    O segments in rows 2, 6, ..; one pattern each at n < 9, two each from 9x9 on.  (board, player, last, gap cells)"""
    assert n >= k + 1
    per = 1 if n < 9 else 2
    board, gaps = np.zeros(n * n, np.uint8), []
    last = -1
    for colour, row0 in ((1, 0), (2, 2)):
        for j in range(per):
            r = row0 + 4 * j
            assert r < n
            for c in range(k + 1):
                if c == k // 2:
                    gaps.append(r * n + c)
                else:
                    board[r * n + c] = colour
                    last = r * n + c if colour == 2 else last
    for a in np.flatnonzero(board):
        assert not wins_freestyle(board, int(a), n, k)
    return board, 1, last, gaps


def selfplay_from(evaluate, n, kwin, S, seed, board, player, last, L=1):
    """tests.forced.selfplay_game started from a position (az_set_start_positions): everything indexed by ply keeps the absolute
    ply = the stones on the board -- the temperature table, the noise offset and u.  Runs under the rule the modules' name
    points at (use_rule)."""
    nn = n * n
    noise, us = orc.selfplay_tape(seed, n)
    T = orc.selfplay_T_table(nn)
    board = np.array(board, np.uint8)
    m = int((board != 0).sum())
    off = sum(nn - j for j in range(m))
    out = dict(boards=[], movers=[], lasts=[], actions=[], pis=[], visits=[])
    while True:
        r = forced.search_move(evaluate, n, kwin, S, board, player, last, T[m], noise[off:off + nn - m], us[m], L=L)
        a = r["action"]
        out["boards"].append(board.copy()); out["movers"].append(player); out["lasts"].append(last); out["actions"].append(a)
        out["pis"].append(r["pi"]); out["visits"].append(r["N"])
        board = board.copy()
        board[a] = player
        res = player if forced.wins_through(board, a, n, kwin) else (3 if not (board == 0).any() else 0)
        last, player, off, m = a, 3 - player, off + nn - m, m + 1
        if res:
            break
    movers = np.array(out["movers"], np.int64)
    g = dict(boards=np.array(out["boards"], np.uint8), movers=movers.astype(np.uint8), lasts=np.array(out["lasts"], np.int16),
             actions=np.array(out["actions"], np.int16), pis=np.array(out["pis"], np.float32), visits=np.array(out["visits"], np.int32),
             result=res, nply=len(movers))
    g["z"] = (np.zeros(len(movers)) if res == 3 else np.where(movers == res, 1, -1)).astype(np.int8)
    return g


def line_cases(n, k):
    """crafted X sequences for az_rules_replay, O on far filler cells: for each direction a run of exactly k touching the edges
    and corners, completed at an end and in the middle (a win under both rules); k + 1 cells with the middle one last and
    2k - 1 cells with the middle one last (overlines: a win under FREESTYLE only), each followed by more moves; 2k + 1 cells with
    the middle one last ("long": the k-th stone of either half already makes exactly k, so it is a win under both rules before
    the middle is reached, and the winner stays); an overline crossing an exact run at the last stone (a win under both); and
    index runs that are lines only if the board wrapped.
    -> list of (name, action list)"""
    cases = []

    def seq_of(xs, extra=0):
        taken = set(xs)
        fill = [c for c in range(n * n - 1, -1, -1) if c not in taken and (c // n + 2 * (c % n)) % 5 == 0]
        if len(fill) < len(xs) - 1:
            return None
        s = []
        for i, x in enumerate(xs):
            s.append(x)
            if i < len(xs) - 1:
                s.append(fill[i])
        free = [c for c in range(n * n - 1, -1, -1) if c not in taken and c not in s]
        return s + free[:extra] if len(free) >= extra else None   # the game goes on: O, X, O ..

    def add(name, xs, extra=0):
        if not (all(0 <= x < n * n for x in xs) and len(set(xs)) == len(xs)):
            return
        for ex in sorted({extra, min(extra, 1), 0}, reverse=True):
            s = seq_of(xs, ex)
            # the moves after an overline must not end the game themselves: fewer of them where the board is small
            if s is not None and (not name.startswith("over") or replay(s, n, k, "exact")[3] == 0):
                cases.append((name, s))
                return

    def cells_of(r0, c0, dr, dc, m):
        cs = [(r0 + i * dr, c0 + i * dc) for i in range(m)]
        return [r * n + c for r, c in cs] if all(0 <= r < n and 0 <= c < n for r, c in cs) else None

    for dr, dc in DIRS:
        for r0 in (0, n - k if dr else n - 1):
            for c0 in ((0, n - k) if dc == 1 else ((k - 1, n - 1) if dc == -1 else (0, n - 1))):
                xs = cells_of(r0, c0, dr, dc, k)
                if xs:
                    add(f"exact-end {dr}{dc}", xs)
                    add(f"exact-mid {dr}{dc}", xs[:k // 2] + xs[k // 2 + 1:] + [xs[k // 2]])
        for m, name in ((k + 1, "over"), (2 * k - 1, "over2"), (2 * k + 1, "long")):
            xs = cells_of(0, 0 if dc >= 0 else n - 1, dr, dc, m) if dr else cells_of(1, 0, dr, dc, m)
            if xs:
                mid = xs.pop(m // 2)
                add(f"{name} {dr}{dc}", xs + [mid], extra=3)
    # an overline along a row crossing an exact run down a column at the last stone
    if n >= k + 1:
        row = cells_of(0, 0, 0, 1, k + 1)
        col = cells_of(0, k // 2, 1, 0, k)
        cross = row[k // 2]
        add("cross", [x for x in row if x != cross] + [x for x in col if x != cross] + [cross])
    for start in (n - 2, n - 1, 2 * n - 3):
        xs = [start + i for i in range(k)]
        if len({x // n for x in xs}) > 1:
            add(f"wrap-row {start}", xs)
    for start, step in ((n - 2, n + 1), (1, n - 1), (n + 1, n - 1)):
        xs = [start + i * step for i in range(k)]
        cols = [x % n for x in xs]
        if max(xs) < n * n and any(abs(cols[i + 1] - cols[i]) != 1 for i in range(k - 1)):
            add(f"wrap-diag {start}", xs)
    return cases
