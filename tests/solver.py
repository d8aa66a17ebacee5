"""MCTS-Solver (az_set_solver), restated in numpy for the tests.

Written from the rule in include/az_engine.h, not from the kernels: the float64 tree search of tests/forced.py (row-major
expansion, the engine's PUCT expression and operation order, W accumulated in backup order, the root noise mixed as float32
multiply, float64 add, float32 store) with one status per edge, the masked selection, the stop on a proven edge, the marking
walk after a real terminal, the count vector N' and the exact value.  Any evaluate(board uint8[nn], player, last) ->
(P float32[nn], v) serves as the evaluator.  With solver=False it is the plain search (tests/test_solver_cpu.py holds it to
Oracle.search)."""
import numpy as np

from oracle import oracle as orc
from tests.forced import mix_noise, pi_action, random_position, wins_through  # noqa: F401  (re-exported for the tests)

UNKNOWN, WIN, LOSS, DRAW = 0, 1, 2, 3
NEGATE = {WIN: LOSS, LOSS: WIN, DRAW: DRAW}
VALUE = {WIN: 1.0, LOSS: -1.0, DRAW: 0.0}        # of the side the status belongs to


class _Row:
    def __init__(self, P):
        nn = len(P)
        self.P = np.asarray(P, np.float32).astype(np.float64)     # the float32 prior, widened on use
        self.N = np.zeros(nn, np.int64)
        self.W = np.zeros(nn, np.float64)
        self.child = np.zeros(nn, np.int64)                        # 0 = not expanded
        self.st = np.zeros(nn, np.int8)                            # status of every edge, seen from the side that makes the move


def node_status(st, legal):
    """the status of a node, seen from its side to move, from its edges' statuses over its legal cells"""
    s = np.asarray(st)[np.asarray(legal, bool)]
    if (s == WIN).any():
        return WIN
    if len(s) and (s != UNKNOWN).all():
        return DRAW if (s == DRAW).any() else LOSS
    return UNKNOWN


def search(evaluate, n, kwin, S, board, player, last, noise=None, solver=True, c_puct=2.0, w=0.25, info=None):
    """MCTS.run's tree (mcts.py:101-141) -> dict(N int32[nn], W float64[nn], P float32[nn], st int8[nn], root int) of the root,
    zeros on occupied cells.  info (a dict): receives "stops", the simulations that ended on a proven edge, and "terminals"."""
    board = np.asarray(board, np.uint8)
    P0, _ = evaluate(board, player, last)
    if noise is not None:
        P0 = mix_noise(P0, board, noise, w)
    rows = [_Row(P0)]
    root_status = UNKNOWN
    stops = terminals = 0

    for total in range(S):
        b, pl, la, row, npar, path = board.copy(), player, last, 0, total, []
        occs = []                                                  # the occupancy of every path level, for the marking walk
        mark = UNKNOWN
        while True:
            r = rows[row]
            with np.errstate(divide="ignore", invalid="ignore"):
                Q = np.where(r.N > 0, r.W / r.N, 0.0)
            sc = Q + ((c_puct * r.P) * np.sqrt(npar + 1e-8)) / (1 + r.N).astype(np.float64)
            legal = b == 0
            if solver:
                sc = np.where(r.st == WIN, np.inf, sc)
                if (legal & (r.st != LOSS)).any():
                    sc = np.where(r.st == LOSS, -np.inf, sc)
            sc = np.where(legal, sc, -np.inf)
            a = int(np.argmax(sc))                                 # the first maximum in row-major order
            path.append((row, a))
            occs.append(legal.copy())
            b[a] = pl
            pl, la = 3 - pl, a
            if wins_through(b, a, n, kwin):                        # the real terminal tests come first
                value, kind = -1.0, "term"
                mark = WIN
                break
            if not (b == 0).any():
                value, kind = 0.0, "term"
                mark = DRAW
                break
            if solver and r.st[a] != UNKNOWN:                      # a proven edge: no evaluation, no row
                value, kind = -VALUE[int(r.st[a])], "stop"
                break
            if r.child[a] == 0:
                Pn, v = evaluate(b, pl, la)
                r.child[a] = len(rows)
                rows.append(_Row(Pn))
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
        if solver and kind == "term" and rows[path[-1][0]].st[path[-1][1]] == UNKNOWN:
            status = mark
            for lvl in range(len(path) - 1, -1, -1):
                prow, pa = path[lvl]
                rows[prow].st[pa] = status
                ns = node_status(rows[prow].st, occs[lvl])
                if ns == UNKNOWN:
                    break
                if lvl == 0:
                    root_status = ns
                else:
                    status = NEGATE[ns]
    if info is not None:
        info["stops"], info["terminals"] = stops, terminals
    legal = board == 0
    r = rows[0]
    return dict(N=np.where(legal, r.N, 0).astype(np.int32), W=np.where(legal, r.W, 0.0),
                P=np.where(legal, r.P, 0.0).astype(np.float32), st=np.where(legal, r.st, 0).astype(np.int8), root=int(root_status))


def solver_counts(N, st):
    """N' of one root row of legal children (raw counts, statuses), by the definition"""
    N, st = np.asarray(N, np.int64), np.asarray(st, np.int64)
    if (st == WIN).any():
        return np.where(st == WIN, N, 0).astype(np.int32)
    if ((st != LOSS) & (N > 0)).any():
        return np.where(st == LOSS, 0, N).astype(np.int32)
    return N.astype(np.int32)


def search_move(evaluate, n, kwin, S, board, player, last, T, noise, u, solver=True, c_puct=2.0, log_table=None, counts_fn=None):
    """one ply: the tree, then pi and the action from N' and the value (exact when the root is proven)"""
    r = search(evaluate, n, kwin, S, board, player, last, noise, solver, c_puct)
    legal = np.flatnonzero(np.asarray(board) == 0)
    counts = r["N"][legal]
    if solver:
        counts = (counts_fn or solver_counts)(counts, r["st"][legal])
    r["Np"] = np.zeros(n * n, np.int32)
    r["Np"][legal] = counts
    r["pi"], r["action"] = pi_action(counts, board, T, u, orc.numpy_log_table(S) if log_table is None else log_table)
    astar = int(np.argmax(r["N"]))
    if r["root"] != UNKNOWN:
        r["value"] = np.float32(VALUE[r["root"]])
    else:
        r["value"] = np.float32(np.float64(r["W"][astar]) / np.float64(r["N"][astar]))
    return r


def selfplay_game(evaluate, n, kwin, S, seed, solver=True, cap=None, full_fn=None, resign=None):
    """one self-play game from the empty board with the game's own tape (oracle.selfplay_tape) and temperature schedule.
    cap = (fast_sims, permille) with full_fn(seed, ply, permille) -> bool: FAST plies get fast_sims simulations and no noise.
    resign = (threshold, min_ply): the mover resigns when the ply's value is below -threshold (no exempt games here)."""
    nn = n * n
    noise, us = orc.selfplay_tape(seed, n)
    T = orc.selfplay_T_table(nn)
    board, player, last, m, off = np.zeros(nn, np.uint8), 1, -1, 0, 0
    out = dict(boards=[], movers=[], lasts=[], actions=[], pis=[], visits=[], values=[], proofs=[])
    while True:
        full = cap is None or bool(full_fn(seed, m, cap[1]))
        r = search_move(evaluate, n, kwin, S if full else cap[0], board, player, last, T[m], noise[off:off + nn - m] if full else None,
                        us[m], solver)
        a = r["action"]
        out["boards"].append(board.copy()); out["movers"].append(player); out["lasts"].append(last); out["actions"].append(a)
        out["pis"].append(r["pi"]); out["visits"].append(r["N"]); out["values"].append(r["value"]); out["proofs"].append(r["root"])
        board = board.copy()
        board[a] = player
        res = player if wins_through(board, a, n, kwin) else (3 if not (board == 0).any() else 0)
        if not res and resign is not None and m >= resign[1] and float(r["value"]) < -resign[0]:
            res = 3 - player
        last, player, off, m = a, 3 - player, off + nn - m, m + 1
        if res:
            break
    movers = np.array(out["movers"], np.int64)
    g = dict(boards=np.array(out["boards"], np.uint8), movers=movers.astype(np.uint8), lasts=np.array(out["lasts"], np.int16),
             actions=np.array(out["actions"], np.int16), pis=np.array(out["pis"], np.float32), visits=np.array(out["visits"], np.int32),
             values=np.array(out["values"], np.float32), proofs=np.array(out["proofs"], np.int8), result=res, nply=m)
    g["z"] = (np.zeros(m) if res == 3 else np.where(movers == res, 1, -1)).astype(np.int8)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# brute-force minimax, and the crafted positions
# ---------------------------------------------------------------------------------------------------------------------
def minimax(board, player, n, kwin, memo=None):
    """the game-theoretic status of the side to move: WIN, LOSS or DRAW"""
    memo = {} if memo is None else memo
    key = (bytes(board), player)
    if key in memo:
        return memo[key]
    best = LOSS
    for a in np.flatnonzero(board == 0):
        board[a] = player
        if wins_through(board, int(a), n, kwin):
            res = WIN
        elif not (board == 0).any():
            res = DRAW
        else:
            res = NEGATE[minimax(board, 3 - player, n, kwin, memo)]
        board[a] = 0
        if res == WIN:
            best = WIN
            break
        if res == DRAW:
            best = DRAW
    memo[key] = best
    return best


def minimax_edge(board, player, a, n, kwin, memo=None):
    """the status of the move a for the mover"""
    b = np.array(board, np.uint8)
    b[a] = player
    if wins_through(b, int(a), n, kwin):
        return WIN
    if not (b == 0).any():
        return DRAW
    return NEGATE[minimax(b, 3 - player, n, kwin, memo)]


def crafted_a(n, k):
    """the mover (X) has k - 1 stones at row n // 2, columns 0 .. k - 2: one winning cell.  (board, player, last, winning cell)"""
    board = np.zeros(n * n, np.uint8)
    r = n // 2
    for c in range(k - 1):
        board[r * n + c] = 1
    opp = [(0, 0), (0, 2), (n - 1, 1), (n - 1, 3)][:k - 1]      # the opponent's stones, nowhere near a line
    for rr, cc in opp:
        board[rr * n + cc] = 2
    return board, 1, opp[-1][0] * n + opp[-1][1], r * n + k - 1


def crafted_b(n, k):
    """the opponent (O) has an open k - 1 at row n // 2, columns 1 .. k - 1; the mover (X) has stones on the edge rows: every
    move loses.  (board, player, last, the two ends)"""
    board = np.zeros(n * n, np.uint8)
    r = n // 2
    for c in range(1, k):
        board[r * n + c] = 2
    for rr, cc in [(0, 0), (0, 2), (n - 1, 1), (n - 1, 3)][:k - 1]:
        board[rr * n + cc] = 1
    return board, 1, r * n + k - 1, (r * n, r * n + k)


def constant_eval(n, logits=None):
    """a constant net: softmax of the given logits (uniform by default), value 0"""
    lg = np.zeros(n * n, np.float32) if logits is None else np.asarray(logits, np.float32)
    e = np.exp(lg - lg.max())
    P = (e / e.sum(dtype=np.float32)).astype(np.float32)
    return lambda b, pl, la: (P, 0.0)
