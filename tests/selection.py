"""The selection rule (az_set_selection) restated in numpy for the tests: first-play urgency and visit-dependent c_puct.

Written from the rule in include/az_engine.h, not from the kernels: the float64 tree search of tests/forced.py (row-major
expansion, W accumulated in backup order, the root noise mixed as float32 multiply, float64 add, float32 store, virtual-loss
batches of L leaves, forced playouts) with the child's score taken from the rule: an unvisited child is worth V_X - r_X *
mass_table[idx] and c_puct is cpuct_table[parent count].  The two tables come from the library (_capi.selection_tables), so
that the restatement reads the host's log instead of guessing it; tests/test_selection_cpu.py holds them to their formulas.
With sel=None the search is forced.search, and so Oracle.search.

Every search counts the selections whose argmax differs from the plain rule's on the same tree state, at the root and below
it (info["root_diff"], info["below_diff"]): a case in which both stay 0 shows nothing.

The win test is looked up in tests/forced.py at call time, so tests/win_rule.py's use_rule() serves this module as well."""
import numpy as np

from oracle import oracle as orc
from tests import forced
from tests.forced import _Row, mix_noise, pi_action

from alphazero_piskvorky_amd import _capi

MASS_ONE = 1 << 24           # a prior of 1.0 as the integer the mass sums
MASS_SHIFT, MASS_STEPS = 12, 4096

# the parameter sets of the GPU tests
SETS = {
    "a": dict(fpu=0.2, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0),
    "b": dict(fpu=0.0, fpu_root=0.0, cpuct_base=50.0, cpuct_factor=1.0),
    "c": dict(fpu=0.2, fpu_root=0.1, cpuct_base=50.0, cpuct_factor=1.0),
    "d": dict(fpu=0.0, fpu_root=0.0, cpuct_base=19652.0, cpuct_factor=0.0),
}


C_PUCT = 3.0                 # at 2.0 sets (b) and (d) leave the un-noised 5x5 empty-board search at S = 64 as it is
SIZES = ((5, 4), (9, 5), (15, 5))
# seeds of the 6-stone and 11-stone positions, the first ones at which every parameter set changes the search with and without noise
POSITION_SEEDS = {5: (2, 2), 9: (2, 2), 15: (3, 3)}
_POSITIONS = {}


def positions(n, k):
    """the empty board, a 6-stone and an 11-stone position, each with its Dirichlet sample, uniform and temperature"""
    if (n, k) not in _POSITIONS:
        out = []
        for i, (stones, seed) in enumerate(((0, 1),) + tuple(zip((6, 11), POSITION_SEEDS[n]))):
            board, player, last = forced.random_position(n, k, stones, seed)
            rs = np.random.RandomState(1000 * n + i)
            noise = rs.dirichlet([0.3] * int((board == 0).sum()))
            out.append(dict(board=board, player=player, last=last, noise=noise, u=float(rs.random_sample()), T=(1.0, 0.5, 1e-9)[i]))
        _POSITIONS[(n, k)] = tuple(out)
    return _POSITIONS[(n, k)]


def tables(c_puct, sel, S):
    """(cpuct_table float64[S + 2], mass_table float64[4097]) as an engine with S simulations uploads them"""
    return _capi.selection_tables(c_puct, sel["cpuct_base"], sel["cpuct_factor"], S)


def visited_mass(P, visited):
    """sum over the visited children of (uint32) floor((double)P * 2^24): P the float32 priors widened to float64"""
    return int(np.floor(np.asarray(P, np.float64)[visited] * float(MASS_ONE)).astype(np.int64).sum())


def scores(r, b, npar, vx, at_root, c_puct, sel, tabs):
    """(scores of the row's children before forcing and the legality mask, their Q): the rule of include/az_engine.h"""
    nv = r.N + r.fl
    wv = r.W - r.fl.astype(np.float64)
    visited = nv > 0
    sq = np.sqrt(npar + 1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        if sel is None:
            Q = np.where(visited, wv / nv, 0.0)
            c = c_puct
        else:
            cpuct, mass_table = tabs
            mass = visited_mass(r.P, visited & (b == 0))
            idx = min(mass >> MASS_SHIFT, MASS_STEPS)
            red = (sel["fpu_root"] if at_root else sel["fpu"]) * mass_table[idx]
            Q = np.where(visited, wv / nv, vx - red)
            c = cpuct[npar]
    return Q + ((c * r.P) * sq) / (1 + nv).astype(np.float64), Q


def search(evaluate, n, kwin, S, board, player, last, noise=None, forced_k=0.0, c_puct=2.0, w=0.25, L=1, sel=None, info=None,
           table_S=None):
    """forced.search with the selection rule `sel` (a dict over fpu, fpu_root, cpuct_base, cpuct_factor; None = the plain rule).
    table_S: the simulations of the engine whose tables are used (a FAST ply of the playout cap searches fewer).  info (a dict)
    receives root_diff / below_diff, the selections whose argmax differs from the plain rule's on the same tree state."""
    board = np.asarray(board, np.uint8)
    P0, v0 = evaluate(board, player, last)
    root_value = float(np.float32(v0))                         # the float32 value the root's evaluation gave, widened
    if noise is not None:
        P0 = mix_noise(P0, board, noise, w)
    rows = [_Row(P0)]
    forced_on = forced_k > 0.0 and noise is not None
    tabs = None if sel is None else tables(c_puct, sel, S if table_S is None else table_S)
    diff = dict(root_diff=0, below_diff=0)

    def pick(sc, r, b, row, total):
        if forced_on and row == 0:
            nd = (r.N + r.fl).astype(np.float64)
            sc = np.where(nd * nd < (forced_k * r.P) * float(total), np.inf, sc)
        return int(np.argmax(np.where(b == 0, sc, -np.inf)))   # the first maximum in row-major order

    def select(total):
        b, pl, la, row, npar, path, vx = board.copy(), player, last, 0, total, [], root_value
        while True:
            r = rows[row]
            sc, Q = scores(r, b, npar, vx, row == 0, c_puct, sel, tabs)
            a = pick(sc, r, b, row, total)
            if sel is not None:
                plain = pick(scores(r, b, npar, vx, row == 0, c_puct, None, None)[0], r, b, row, total)
                diff["root_diff" if row == 0 else "below_diff"] += int(plain != a)
            path.append((row, a))
            b[a] = pl
            pl, la = 3 - pl, a
            if forced.wins_through(b, a, n, kwin):
                return path, "term", b, pl, la, -1.0
            if not (b == 0).any():
                return path, "term", b, pl, la, 0.0
            if r.child[a] == 0:
                return path, "expand", b, pl, la, None
            vx = -float(Q[a])                                  # the node below, for its side to move
            npar, row = int((r.N + r.fl)[a]), int(r.child[a])

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
    if info is not None:
        info.update(diff)
    legal = board == 0
    r = rows[0]
    return dict(N=np.where(legal, r.N, 0).astype(np.int32), W=np.where(legal, r.W, 0.0),
                P=np.where(legal, r.P, 0.0).astype(np.float32), root_value=np.float32(v0))


def prune_c(c_puct, sel, S, total):
    """the c_puct the pruning pass takes: c(total), the count its sqrt takes"""
    return c_puct if sel is None else float(tables(c_puct, sel, S)[0][int(total)])


def search_move(evaluate, n, kwin, S, board, player, last, T, noise, u, forced_k=0.0, do_prune=True, c_puct=2.0, L=1, sel=None,
                log_table=None, pruner=None, info=None, table_S=None):
    """one ply, as forced.search_move: the tree, then pi and the action from the pruned counts when forced playouts apply (the
    pruning's score uses c(total)), else from the raw ones"""
    tS = S if table_S is None else table_S
    r = search(evaluate, n, kwin, S, board, player, last, noise, forced_k, c_puct, L=L, sel=sel, info=info, table_S=tS)
    legal = np.flatnonzero(np.asarray(board) == 0)
    counts = r["N"][legal]
    if forced_k > 0.0 and noise is not None and do_prune:
        counts = (pruner or forced.prune)(forced_k, prune_c(c_puct, sel, tS, counts.sum()), counts, r["W"][legal], r["P"][legal])
    r["Np"] = np.zeros(n * n, np.int32)
    r["Np"][legal] = counts
    r["pi"], r["action"] = pi_action(counts, board, T, u, orc.numpy_log_table(tS) if log_table is None else log_table)
    astar = int(np.argmax(r["N"]))
    r["value"] = np.float32(np.float64(r["W"][astar]) / np.float64(r["N"][astar]))
    return r


def selfplay_game(evaluate, n, kwin, S, seed, sel=None, forced_k=0.0, do_prune=True, cap=None, full_fn=None, L=1, board=None,
                  player=1, last=-1, ply0=0, c_puct=C_PUCT):
    """forced.selfplay_game with the selection rule: one self-play game with the game's own tape (oracle.selfplay_tape) and
    temperature schedule.  cap = (fast_sims, permille) with full_fn(seed, ply, permille): a FAST ply gets fast_sims simulations
    and no noise; its root uses fpu_root like any root.  board / player / last / ply0: the game continues this position at
    absolute ply ply0 (the tape is the game's, read from that ply on)."""
    nn = n * n
    noise, us = orc.selfplay_tape(seed, n)
    T = orc.selfplay_T_table(nn)
    board = np.zeros(nn, np.uint8) if board is None else np.asarray(board, np.uint8).copy()
    m = ply0
    off = sum(nn - i for i in range(m))
    out = dict(boards=[], movers=[], lasts=[], actions=[], pis=[], visits=[], values=[], root=[], below=[])
    while True:
        full = cap is None or bool(full_fn(seed, m, cap[1]))
        info = {}
        r = search_move(evaluate, n, kwin, S if full else cap[0], board, player, last, T[m], noise[off:off + nn - m] if full else None,
                        us[m], forced_k, do_prune, c_puct=c_puct, L=L, sel=sel, info=info, table_S=S)
        a = r["action"]
        out["boards"].append(board.copy()); out["movers"].append(player); out["lasts"].append(last); out["actions"].append(a)
        out["pis"].append(r["pi"]); out["visits"].append(r["N"]); out["values"].append(r["value"])
        out["root"].append(info.get("root_diff", 0)); out["below"].append(info.get("below_diff", 0))
        board = board.copy()
        board[a] = player
        res = player if forced.wins_through(board, a, n, kwin) else (3 if not (board == 0).any() else 0)
        last, player, off, m = a, 3 - player, off + nn - m, m + 1
        if res:
            break
    movers = np.array(out["movers"], np.int64)
    g = dict(boards=np.array(out["boards"], np.uint8), movers=movers.astype(np.uint8), lasts=np.array(out["lasts"], np.int16),
             actions=np.array(out["actions"], np.int16), pis=np.array(out["pis"], np.float32), visits=np.array(out["visits"], np.int32),
             values=np.array(out["values"], np.float32), root_diff=int(sum(out["root"])), below_diff=int(sum(out["below"])),
             result=res, nply=m - ply0)
    g["z"] = (np.zeros(len(movers)) if res == 3 else np.where(movers == res, 1, -1)).astype(np.int8)
    return g
