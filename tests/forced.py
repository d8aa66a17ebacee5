"""Forced playouts and policy target pruning (az_set_forced_playouts), restated in numpy for the tests.

Written from the rule in include/az_engine.h, not from the kernels: a float64 tree search with row-major expansion, the
engine's PUCT expression and operation order, W accumulated in backup order and the root noise mixed as float32 multiply,
float64 add, float32 store; the pruning by its definition (a linear scan, where the engine bisects); and pi and the
RandomState.choice step (mcts.py:144-177) from integer counts.  Any evaluate(board uint8[nn], player, last) -> (P float32[nn],
v) serves as the evaluator.  With k = 0 the search is the plain one (tests/test_forced_playouts_cpu.py holds it to
Oracle.search); with L > 1 it runs the virtual-loss batches the way include/az_engine.h describes them."""
import numpy as np

from oracle import oracle as orc


# ---------------------------------------------------------------------------------------------------------------------
# rules
# ---------------------------------------------------------------------------------------------------------------------
def wins_through(board, a, n, k):
    """the stone at cell a is part of k or more in a row (games.py:133-166)"""
    p, r, c = board[a], a // n, a % n
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        cnt = 1
        for sgn in (1, -1):
            rr, cc = r + sgn * dr, c + sgn * dc
            while 0 <= rr < n and 0 <= cc < n and board[rr * n + cc] == p:
                cnt += 1
                rr, cc = rr + sgn * dr, cc + sgn * dc
        if cnt >= k:
            return True
    return False


def random_position(n, k, stones, seed):
    """a legal, unfinished position with `stones` stones, X to move first: (board, player, last)"""
    rs = np.random.RandomState(seed)
    while True:
        board, player, last = np.zeros(n * n, np.uint8), 1, -1
        for _ in range(stones):
            a = int(rs.choice(np.flatnonzero(board == 0)))
            board[a] = player
            if wins_through(board, a, n, k):
                break
            player, last = 3 - player, a
        else:
            return board, player, last


# ---------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------
class _Row:
    def __init__(self, P):
        nn = len(P)
        self.P = np.asarray(P, np.float32).astype(np.float64)     # the float32 prior, widened on use
        self.N = np.zeros(nn, np.int64)
        self.W = np.zeros(nn, np.float64)
        self.fl = np.zeros(nn, np.int64)                           # in-flight visits of the current batch
        self.child = np.zeros(nn, np.int64)                        # 0 = not expanded


def mix_noise(P, board, noise, w):
    """mcts.py:113-116 as the engine computes it: float32 multiply, float64 add, float32 store, legal cells in row-major order"""
    P = np.asarray(P, np.float32).copy()
    om = np.float32(1.0 - w)
    legal = np.flatnonzero(board == 0)
    scaled = (om * P[legal]).astype(np.float32)
    P[legal] = (scaled.astype(np.float64) + w * np.asarray(noise, np.float64)).astype(np.float32)
    return P


def search(evaluate, n, kwin, S, board, player, last, noise=None, forced_k=0.0, c_puct=2.0, w=0.25, L=1):
    """MCTS.run's tree (mcts.py:101-141) -> dict(N int32[nn], W float64[nn], P float32[nn]) of the root, zeros on occupied cells.
    forced_k > 0 and noise given: a root child with n visits (in-flight ones included) scores +inf while n^2 < (k P) total.
    L > 1: virtual-loss batches of L leaves."""
    nn = n * n
    board = np.asarray(board, np.uint8)
    P0, _ = evaluate(board, player, last)
    if noise is not None:
        P0 = mix_noise(P0, board, noise, w)
    rows = [_Row(P0)]
    forced = forced_k > 0.0 and noise is not None

    def select(total):
        """one descent: (path [(row, cell)], kind, leaf board, side to move, last, terminal value)"""
        b, pl, la, row, npar, path = board.copy(), player, last, 0, total, []
        while True:
            r = rows[row]
            nv = r.N + r.fl
            wv = r.W - r.fl.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                Q = np.where(nv > 0, wv / nv, 0.0)
            sc = Q + ((c_puct * r.P) * np.sqrt(npar + 1e-8)) / (1 + nv).astype(np.float64)
            if forced and row == 0:
                nd = nv.astype(np.float64)
                sc = np.where(nd * nd < (forced_k * r.P) * float(total), np.inf, sc)
            sc = np.where(b == 0, sc, -np.inf)
            a = int(np.argmax(sc))                                 # the first maximum in row-major order
            path.append((row, a))
            b[a] = pl
            pl, la = 3 - pl, a
            if wins_through(b, a, n, kwin):
                return path, "term", b, pl, la, -1.0               # the side to move has lost
            if not (b == 0).any():
                return path, "term", b, pl, la, 0.0
            if r.child[a] == 0:
                return path, "expand", b, pl, la, None
            npar, row = int(nv[a]), int(r.child[a])

    def backup(path, value):
        val = -value
        for row, a in reversed(path):
            rows[row].N[a] += 1
            rows[row].W[a] += val
            val = -val

    done = 0
    while done < S:
        nb = min(L, S - done)
        items = []
        for j in range(nb):
            path, kind, b, pl, la, tv = select(done + j)
            dup = None
            if kind == "expand":
                for i, it in enumerate(items):
                    if it["kind"] == "expand" and it["path"][-1] == path[-1]:
                        kind, dup = "dup", i
                        break
            for row, a in path:
                rows[row].fl[a] += 1
            items.append(dict(path=path, kind=kind, b=b, pl=pl, la=la, tv=tv, dup=dup))
        for it in items:
            if it["kind"] == "expand":
                it["P"], it["v"] = evaluate(it["b"], it["pl"], it["la"])
        for it in items:
            for row, a in it["path"]:
                rows[row].fl[a] -= 1
            if it["kind"] == "term":
                value = it["tv"]
            elif it["kind"] == "expand":
                row, a = it["path"][-1]
                rows[row].child[a] = len(rows)
                rows.append(_Row(it["P"]))
                value = float(np.float32(it["v"]))
            else:
                value = float(np.float32(items[it["dup"]]["v"]))
            backup(it["path"], value)
        done += nb
    legal = board == 0
    r = rows[0]
    return dict(N=np.where(legal, r.N, 0).astype(np.int32), W=np.where(legal, r.W, 0.0),
                P=np.where(legal, r.P, 0.0).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# pruning, pi and the sampled action
# ---------------------------------------------------------------------------------------------------------------------
def prune(k, c_puct, N, W, P, info=None):
    """N' of one root row of legal children (int counts, float64 W, float32 priors), by the definition.  info (a dict): receives
    "single", the number of children that were left with a single playout and so emptied"""
    N = [int(x) for x in N]
    W = [float(x) for x in W]
    P = [float(np.float32(x)) for x in P]
    total = sum(N)
    sq = float(np.sqrt(total + 1e-8))
    star = max(range(len(N)), key=lambda c: (N[c], -c))           # the most visited child, the lowest on ties

    def score(c, m):
        return W[c] / float(N[c]) + ((c_puct * P[c]) * sq) / float(1 + m)

    target = score(star, N[star])
    out, single = list(N), 0
    for c in range(len(N)):
        if c == star or N[c] == 0:
            continue
        thr = (k * P[c]) * float(total)
        F = 0
        while float(F) * float(F) < thr:
            F += 1
        m = N[c]
        if score(c, N[c]) < target:
            m = next(x for x in range(max(0, N[c] - F), N[c] + 1) if score(c, x) < target)
        if m == 1 and m < N[c]:
            m = 0
            single += 1
        out[c] = m
    if info is not None:
        info["single"] = single
    return np.array(out, np.int32)


def pi_action(counts, board, T, u, log_table):
    """mcts.py:144-177 from the integer counts of the legal cells (row-major): (pi float32[nn], action)"""
    board = np.asarray(board, np.uint8)
    legal = np.flatnonzero(board == 0)
    counts = np.asarray(counts, np.int64)
    assert len(counts) == len(legal)
    lg = np.asarray(log_table, np.float32)[counts]
    if T <= 1e-7:
        y = lg / np.float32(1e-7)
        y = y - y.max()
        with np.errstate(under="ignore"):
            y = np.where(y == 0, np.float32(1.0), np.exp(y)).astype(np.float32)
        e = (y / y.sum(dtype=np.float32)).astype(np.float64)
    else:
        e = lg.astype(np.float64) / T
        e = np.exp(e - e.max())
        s = 0.0 + e.sum()
        e = np.full(len(e), 1.0 / len(e)) if (s < 1e-8 or s != s) else e / s
    pi = np.zeros(len(board), np.float32)
    pi[legal] = e.astype(np.float32)
    cdf = e.cumsum()
    cdf /= cdf[-1]
    idx = min(int(cdf.searchsorted(u, side="right")), len(legal) - 1)
    return pi, int(legal[idx])


def search_move(evaluate, n, kwin, S, board, player, last, T, noise, u, forced_k=0.0, do_prune=True, c_puct=2.0, L=1,
                log_table=None, pruner=None):
    """one ply: the tree, then pi and the action from the pruned counts when the rule applies (forced_k > 0, a noised root and
    do_prune), else from the raw ones.  pruner(k, c_puct, N, W, P) -> N': the pruning to use, default prune above."""
    r = search(evaluate, n, kwin, S, board, player, last, noise, forced_k, c_puct, L=L)
    legal = np.flatnonzero(np.asarray(board) == 0)
    counts = r["N"][legal]
    if forced_k > 0.0 and noise is not None and do_prune:
        counts = (pruner or prune)(forced_k, c_puct, counts, r["W"][legal], r["P"][legal])
    r["Np"] = np.zeros(n * n, np.int32)
    r["Np"][legal] = counts
    r["pi"], r["action"] = pi_action(counts, board, T, u, orc.numpy_log_table(S) if log_table is None else log_table)
    astar = int(np.argmax(r["N"]))
    r["value"] = np.float32(np.float64(r["W"][astar]) / np.float64(r["N"][astar]))
    return r


def selfplay_game(evaluate, n, kwin, S, seed, forced_k=0.0, do_prune=True, cap=None, full_fn=None, L=1, pruner=None):
    """one self-play game from the empty board with the game's own tape (oracle.selfplay_tape) and temperature schedule.
    cap = (fast_sims, permille) with full_fn(seed, ply, permille) -> bool: FAST plies get fast_sims simulations, no noise and so
    no rule."""
    nn = n * n
    noise, us = orc.selfplay_tape(seed, n)
    T = orc.selfplay_T_table(nn)
    board, player, last, m, off = np.zeros(nn, np.uint8), 1, -1, 0, 0
    out = dict(boards=[], movers=[], lasts=[], actions=[], pis=[], visits=[], values=[], pruned=[])
    while True:
        full = cap is None or bool(full_fn(seed, m, cap[1]))
        r = search_move(evaluate, n, kwin, S if full else cap[0], board, player, last, T[m], noise[off:off + nn - m] if full else None,
                        us[m], forced_k, do_prune, L=L, pruner=pruner)
        a = r["action"]
        out["boards"].append(board.copy()); out["movers"].append(player); out["lasts"].append(last); out["actions"].append(a)
        out["pis"].append(r["pi"]); out["visits"].append(r["N"]); out["values"].append(r["value"])
        out["pruned"].append(int(r["N"].sum() - r["Np"].sum()))
        board = board.copy()
        board[a] = player
        res = player if wins_through(board, a, n, kwin) else (3 if not (board == 0).any() else 0)
        last, player, off, m = a, 3 - player, off + nn - m, m + 1
        if res:
            break
    movers = np.array(out["movers"], np.int64)
    g = dict(boards=np.array(out["boards"], np.uint8), movers=movers.astype(np.uint8), lasts=np.array(out["lasts"], np.int16),
             actions=np.array(out["actions"], np.int16), pis=np.array(out["pis"], np.float32), visits=np.array(out["visits"], np.int32),
             values=np.array(out["values"], np.float32), pruned=np.array(out["pruned"], np.int64), result=res, nply=m)
    g["z"] = (np.zeros(m) if res == 3 else np.where(movers == res, 1, -1)).astype(np.int8)
    return g
