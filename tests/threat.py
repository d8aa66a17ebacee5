"""The root threat search (az_set_threat_search), restated in numpy for the tests.

Written from the rule in include/az_engine.h, not from the library: win sets by the definition of the two win rules (the maximal
run through the stone, counted cell by cell), T(P, d) as the recursion the header states, every set taken over the whole board.
Beside it a depth-limited brute-force minimax that knows nothing of fours, and the solver's search of tests/solver.py taken with
premarked root statuses (tests/solver.py itself is imported, not changed)."""
import numpy as np

from tests import solver as sv
from tests.forced import mix_noise, pi_action  # noqa: F401  (re-exported for the tests)

UNKNOWN, WIN, LOSS, DRAW = 0, 1, 2, 3
DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))
RULES = ("freestyle", "exact")


def run_len(board, a, n, colour, dr, dc):
    """length of the maximal run of `colour` through cell a along (dr, dc), cell a itself counted as that colour"""
    r, c = divmod(a, n)
    cnt = 1
    for sgn in (1, -1):
        rr, cc = r + sgn * dr, c + sgn * dc
        while 0 <= rr < n and 0 <= cc < n and board[rr * n + cc] == colour:
            cnt += 1
            rr, cc = rr + sgn * dr, cc + sgn * dc
    return cnt


def stone_wins(board, a, n, k, rule, colour):
    """a stone of `colour` on cell a wins at once under `rule`"""
    for dr, dc in DIRS:
        length = run_len(board, a, n, colour, dr, dc)
        if (length == k) if rule == "exact" else (length >= k):
            return True
    return False


def wins_after(rule):
    """wins_through(board, a, n, k) of tests/solver.py's searches under `rule`: the stone already on cell a"""
    return lambda board, a, n, k: stone_wins(board, a, n, k, rule, int(board[a]))


def win_mask(boards, n, k, rule, colour):
    """win(P, c) of many positions at once: boards uint8[E, nn] -> bool[E, nn].  The same definition as stone_wins, with the run
    lengths of every cell counted by n - 1 array steps per direction and side (tests/test_threat_cpu.py holds it to stone_wins)."""
    B = np.asarray(boards, np.uint8).reshape(-1, n, n)
    s = (B == colour).astype(np.int32)
    win = np.zeros(B.shape, bool)
    for dr, dc in DIRS:
        total = np.ones(B.shape, np.int32)
        for sgn in (1, -1):
            g = np.zeros((len(B), n + 2, n + 2), np.int32)       # g[r, c]: the run of `colour` that starts at (r, c) and goes on along the side
            lo_r, lo_c = 1 + sgn * dr, 1 + sgn * dc
            for _ in range(n - 1):
                g[:, 1:n + 1, 1:n + 1] = s * (1 + g[:, lo_r:lo_r + n, lo_c:lo_c + n])
            total += g[:, lo_r:lo_r + n, lo_c:lo_c + n]
        win |= (total == k) if rule == "exact" else (total >= k)
    return (win & (B == 0)).reshape(len(B), n * n)


def win_set(board, n, k, rule, colour):
    """win(P, c): the empty cells where a stone of colour c wins at once, ascending"""
    return [int(a) for a in np.flatnonzero(win_mask(board[None], n, k, rule, colour)[0])]


class _Exhausted(Exception):
    pass


def _T(board, n, k, rule, A, d, ctr, budget):
    """(found, move, depth)"""
    D = 3 - A
    Wa = win_set(board, n, k, rule, A)
    if Wa:
        return True, Wa[0], 1
    if d <= 1:
        return False, -1, 0
    Wd = win_set(board, n, k, rule, D)
    if len(Wd) >= 2:
        return False, -1, 0
    cands = Wd if len(Wd) == 1 else [int(a) for a in np.flatnonzero(board == 0)]
    after = np.repeat(board[None], len(cands), 0)                # P' of every candidate; its W does not depend on the node counter
    after[np.arange(len(cands)), cands] = A
    Ws = win_mask(after, n, k, rule, A)
    for i, x in enumerate(cands):
        W = [int(a) for a in np.flatnonzero(Ws[i])]
        if not W:
            continue
        ctr[0] += 1
        if ctr[0] > budget:
            raise _Exhausted()
        if win_set(after[i], n, k, rule, D):
            continue
        if len(W) >= 2:
            return True, x, 2
        nxt = after[i].copy()
        nxt[W[0]] = D
        found, _, depth = _T(nxt, n, k, rule, A, d - 1, ctr, budget)
        if found:
            return True, x, depth + 1
    return False, -1, 0


def solve(board, n, k, rule, player, max_depth, node_budget):
    """dict(status, move, depth, nodes, edges int8[nn]) of one root, as az_threat_solve reports it"""
    board = np.array(board, np.uint8).reshape(-1)
    A, D = int(player), 3 - int(player)
    Wa, Wd = win_set(board, n, k, rule, A), win_set(board, n, k, rule, D)
    ctr = [0]
    try:
        found, move, depth = _T(board.copy(), n, k, rule, A, max_depth, ctr, node_budget)
    except _Exhausted:
        found, move, depth = False, -1, 0
    edges = np.zeros(n * n, np.int8)
    status = UNKNOWN
    if found:
        status = WIN
        edges[Wa if depth == 1 else [move]] = WIN
    elif Wd:
        edges[board == 0] = LOSS
        if len(Wd) == 1:
            edges[Wd[0]] = UNKNOWN
        else:
            status = LOSS
    return dict(status=status, move=move, depth=depth, nodes=ctr[0], edges=edges, Wa=Wa, Wd=Wd)


def forced_win_within(board, n, k, rule, player, plies):
    """brute force: the side to move wins within `plies` plies against any defence (no notion of fours)"""
    if plies <= 0:
        return False
    opp = 3 - player
    empty = [int(a) for a in np.flatnonzero(board == 0)]
    for a in empty:
        if stone_wins(board, a, n, k, rule, player):
            return True
    if plies < 3:
        return False
    for a in empty:
        board[a] = player
        ok = True
        replies = [int(b) for b in np.flatnonzero(board == 0)]
        if not replies:
            ok = False                                           # the board is full: a draw
        for b in replies:
            if stone_wins(board, b, n, k, rule, opp):
                ok = False
                break
        if ok:
            for b in replies:
                board[b] = opp
                ok = forced_win_within(board, n, k, rule, player, plies - 2)
                board[b] = 0
                if not ok:
                    break
        board[a] = 0
        if ok:
            return True
    return False


def random_position(n, k, rule, stones, rs):
    """stones placed alternately (X first) on random empty cells; positions already won under `rule` are rejected.  -> (board, player)"""
    while True:
        board, player = np.zeros(n * n, np.uint8), 1
        for _ in range(stones):
            a = int(rs.choice(np.flatnonzero(board == 0)))
            board[a] = player
            if stone_wins(board, a, n, k, rule, player):
                break
            player = 3 - player
        else:
            return board, player


def positions(n, k, rule, stones, count, seed):
    rs = np.random.RandomState(seed)
    out = [random_position(n, k, rule, stones, rs) for _ in range(count)]
    return np.stack([b for b, _ in out]), np.array([p for _, p in out], np.uint8)


def last_of(board, player):
    """a last move for a given position: the highest cell of the side that moved, -1 on a board without its stones"""
    cells = np.flatnonzero(np.asarray(board) == 3 - player)
    return int(cells[-1]) if len(cells) else -1


# ---------------------------------------------------------------------------------------------------------------------
# the solver's search with premarked root statuses
# ---------------------------------------------------------------------------------------------------------------------
def search(evaluate, n, kwin, S, board, player, last, noise=None, rule="freestyle", premark=None, c_puct=2.0, w=0.25, info=None):
    """tests/solver.py's search(solver=True) under `rule`, whose root row and root start from premark = (edges int8[nn], root
    status) instead of UNKNOWN.  premark=None: the solver alone.  info receives "stops", "terminals" and "evals"."""
    wins = wins_after(rule)
    board = np.asarray(board, np.uint8)
    P0, _ = evaluate(board, player, last)
    if noise is not None:
        P0 = mix_noise(P0, board, noise, w)
    rows = [sv._Row(P0)]
    root_status = UNKNOWN
    if premark is not None:
        rows[0].st[:] = np.asarray(premark[0], np.int8)
        root_status = int(premark[1])
    stops = terminals = 0
    evals = 1
    for total in range(S):
        b, pl, la, row, npar, path, occs = board.copy(), player, last, 0, total, [], []
        mark = UNKNOWN
        while True:
            r = rows[row]
            with np.errstate(divide="ignore", invalid="ignore"):
                Q = np.where(r.N > 0, r.W / r.N, 0.0)
            sc = Q + ((c_puct * r.P) * np.sqrt(npar + 1e-8)) / (1 + r.N).astype(np.float64)
            legal = b == 0
            sc = np.where(r.st == WIN, np.inf, sc)
            if (legal & (r.st != LOSS)).any():
                sc = np.where(r.st == LOSS, -np.inf, sc)
            sc = np.where(legal, sc, -np.inf)
            a = int(np.argmax(sc))
            path.append((row, a))
            occs.append(legal.copy())
            b[a] = pl
            pl, la = 3 - pl, a
            if wins(b, a, n, kwin):
                value, kind, mark = -1.0, "term", WIN
                break
            if not (b == 0).any():
                value, kind, mark = 0.0, "term", DRAW
                break
            if r.st[a] != UNKNOWN:
                value, kind = -sv.VALUE[int(r.st[a])], "stop"
                break
            if r.child[a] == 0:
                Pn, v = evaluate(b, pl, la)
                evals += 1
                r.child[a] = len(rows)
                rows.append(sv._Row(Pn))
                value, kind = float(np.float32(v)), "expand"
                break
            npar, row = int(r.N[a]), int(r.child[a])
        val = -value
        for prow, pa in reversed(path):
            rows[prow].N[pa] += 1
            rows[prow].W[pa] += val
            val = -val
        stops += kind == "stop"
        terminals += kind == "term"
        if kind == "term" and rows[path[-1][0]].st[path[-1][1]] == UNKNOWN:
            status = mark
            for lvl in range(len(path) - 1, -1, -1):
                prow, pa = path[lvl]
                rows[prow].st[pa] = status
                ns = sv.node_status(rows[prow].st, occs[lvl])
                if ns == UNKNOWN:
                    break
                if lvl == 0:
                    root_status = ns
                else:
                    status = sv.NEGATE[ns]
    if info is not None:
        info["stops"], info["terminals"], info["evals"] = stops, terminals, evals
    legal = board == 0
    r = rows[0]
    return dict(N=np.where(legal, r.N, 0).astype(np.int32), W=np.where(legal, r.W, 0.0),
                P=np.where(legal, r.P, 0.0).astype(np.float32), st=np.where(legal, r.st, 0).astype(np.int8), root=int(root_status))


def threat_search(evaluate, n, kwin, S, board, player, last, noise, rule, max_depth, node_budget, info=None):
    """the search of one root with the option on: the threat search's marks, then the solver's search from them"""
    t = solve(board, n, kwin, rule, player, max_depth, node_budget)
    r = search(evaluate, n, kwin, S, board, player, last, noise, rule, (t["edges"], t["status"]), info=info)
    r["threat"] = t
    return r


# ---------------------------------------------------------------------------------------------------------------------
# crafted positions: (board, player) on an n x n board, X = 1 to move unless said otherwise
# ---------------------------------------------------------------------------------------------------------------------
def _board(n, xs=(), os=()):
    b = np.zeros(n * n, np.uint8)
    for r, c in xs:
        b[r * n + c] = 1
    for r, c in os:
        b[r * n + c] = 2
    return b


def crafted_double_four(n=9):
    """X holds row 4 columns 2..4 (O on (4, 1)) and column 5 rows 1..3 (O on (0, 5)): X at (4, 5) makes a four in the row and one
    in the column, each with a single completion.  -> (board, player, the move)"""
    return _board(n, [(4, 2), (4, 3), (4, 4), (1, 5), (2, 5), (3, 5)], [(4, 1), (0, 5), (0, 0), (0, 2), (8, 1), (8, 3)]), 1, 4 * n + 5


def crafted_overline_four(n=9):
    """X holds row 4 columns 0, 1, 2 and 5.  X at (4, 3) leaves only (4, 4) to complete, which makes a run of six: a four under
    freestyle, nothing under the exact rule.  -> (board, player, the move)"""
    return _board(n, [(4, 0), (4, 1), (4, 2), (4, 5)], [(0, 0), (0, 2), (8, 1), (8, 3)]), 1, 4 * n + 3


def crafted_single_block(n=9):
    """O holds row 4 columns 1..4 with X on (4, 0): X must block at (4, 5), and that is no four of its own.  -> (board, player, block)"""
    return _board(n, [(4, 0), (0, 0), (0, 2), (8, 1)], [(4, 1), (4, 2), (4, 3), (4, 4)]), 1, 4 * n + 5


def crafted_two_completions(n=9):
    """O holds an open four, row 4 columns 1..4: two completions, every move of X loses.  -> (board, player, the completions)"""
    return _board(n, [(0, 0), (0, 2), (8, 1), (8, 3)], [(4, 1), (4, 2), (4, 3), (4, 4)]), 1, (4 * n, 4 * n + 5)


def crafted_block_is_four(n=9):
    """O threatens (4, 5) (row 4 columns 1..4, X on (4, 0)); X holds column 5 rows 1..3: the block at (4, 5) is X's own open four
    in column 5, and the win follows.  -> (board, player, the move)"""
    return _board(n, [(4, 0), (1, 5), (2, 5), (3, 5)], [(4, 1), (4, 2), (4, 3), (4, 4)]), 1, 4 * n + 5


def crafted_depth3(n=9):
    """A win of depth 3 on an n x n board (n >= 9, k = 5), r = n // 2, c = n // 2 - 2.  X holds row r columns c..c+2 (O on
    (r, c-1)) and column c+4 rows r-2, r-1.  The four at (r, c+3) forces (r, c+4) and leads nowhere; the four at (r, c+4) forces
    (r, c+3), after which (r-3, c+4) is an open four in the column.  -> (board, player, the move (r, c+4))"""
    r, c = n // 2, n // 2 - 2
    xs = [(r, c), (r, c + 1), (r, c + 2), (r - 1, c + 4), (r - 2, c + 4)]
    os = [(r, c - 1), (0, 0), (0, 2), (n - 1, 1), (n - 1, 3)]
    return _board(n, xs, os), 1, r * n + c + 4
