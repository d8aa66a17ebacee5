"""Candidate moves (az_set_candidates) restated in numpy for the tests.

Written from the rule in include/az_engine.h, not from the kernels: the float64 tree search of tests/forced.py (row-major
expansion, W accumulated in backup order, virtual-loss batches of L leaves, forced playouts) with
  - the candidate set of a position by its definition, a brute-force Chebyshev test against every stone (candidate_mask);
  - every expansion made from the evaluator's raw output: logits go through the softmax over the candidates (masked_softmax: the
    oracle's exp, orc_test_expf, and the canonical wave sum, wave_sum), the un-normalised priors of the synthetic evaluator
    keep their value on candidates and become 0 elsewhere;
  - the root noise cut down to the candidates and renormalised by its float64 canonical wave sum (mix_noise);
  - the argmax of every level over the candidates of that level's position.
An evaluator here is evaluate(board uint8[nn], player, last) -> (kind, x float32[nn], v) with kind "logits" or "priors"
(net_evaluator, synth_evaluator).  With radius 0 the rule is off: the expansion is the oracle's own P (softmax over all n*n
logits) and the argmax runs over the empty cells, which is forced.search and so Oracle.search (tests/test_candidates_cpu.py).

A search can report how many of its root visits lie outside a given radius' set (info["info_radius"] -> info["outside"]): for a
plain search that is what the rule would have cut, and a case in which it is 0 and the counts are equal shows nothing.

The win test is looked up in tests/forced.py at call time, so tests/win_rule.py's use_rule() serves this module as well."""
import numpy as np

from oracle import oracle as orc
from tests import forced
from tests.forced import _Row, pi_action

C_PUCT = 2.0
SIZES = ((5, 4), (9, 5), (15, 5))
# (stones, seed) of forced.random_position: the empty board, one stone, six and eleven
POSITION_SPECS = ((0, 1), (1, 5), (6, 2), (11, 3))
_POSITIONS = {}


def positions(n, k):
    """the four positions of a size, each with its Dirichlet sample (RandomState(7)), uniform and temperature"""
    if (n, k) not in _POSITIONS:
        out = []
        for i, (stones, seed) in enumerate(POSITION_SPECS):
            board, player, last = forced.random_position(n, k, stones, seed)
            rs = np.random.RandomState(7)
            noise = rs.dirichlet([0.3] * int((board == 0).sum()))
            out.append(dict(board=board, player=player, last=last, noise=noise, u=float(rs.random_sample()), T=(1.0, 0.5, 1e-9, 1.0)[i]))
        _POSITIONS[(n, k)] = tuple(out)
    return _POSITIONS[(n, k)]


def one_stone(n, cell):
    """X has played `cell`, O to move"""
    board = np.zeros(n * n, np.uint8)
    board[cell] = 1
    rs = np.random.RandomState(7)
    return dict(board=board, player=2, last=int(cell), noise=rs.dirichlet([0.3] * (n * n - 1)), u=float(rs.random_sample()), T=1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def candidate_mask(board, n, radius):
    """C of a position, by the definition: bool[nn].  radius 0 = the option off: the empty cells."""
    b = np.asarray(board).reshape(n, n) != 0
    if radius == 0:
        return ~b.reshape(-1)
    if not b.any():
        return np.ones(n * n, bool)
    rr, cc = np.nonzero(b)
    idx = np.arange(n)
    near = (np.abs(idx[:, None, None] - rr) <= radius) & (np.abs(idx[None, :, None] - cc) <= radius)    # [row, col, stone]
    return (near.any(axis=2) & ~b).reshape(-1)


def wave_sum(vals, cells, dtype):
    """the canonical wave sum over `cells` (ascending): lane l adds its cells j = l (mod 64) in ascending order, then
    v[l] = v[l] + v[l ^ msk] for msk = 32, 16, 8, 4, 2, 1"""
    v = np.zeros(64, dtype)
    for j in cells:
        v[j & 63] = v[j & 63] + dtype(vals[j])
    lanes = np.arange(64)
    for msk in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ msk]).astype(dtype)
    return v[0]


def masked_softmax(logits, C):
    """P of an expansion from logits: the softmax over the cells of C, 0.0 elsewhere (float32)"""
    x = np.asarray(logits, np.float32)
    cells = np.flatnonzero(C)
    m = x[cells].max()
    expf = orc.lib().orc_test_expf
    e = np.zeros(len(x), np.float32)
    for j in cells:
        e[j] = expf(float(np.float32(x[j] - m)))
    s = wave_sum(e, cells, np.float32)
    P = np.zeros(len(x), np.float32)
    P[cells] = e[cells] / s
    return P


def expand(kind, x, board, n, radius, oracle_P=None):
    """the priors of a new row"""
    if radius == 0:
        return np.asarray(oracle_P if kind == "logits" else x, np.float32)
    C = candidate_mask(board, n, radius)
    if kind == "logits":
        return masked_softmax(x, C)
    return np.where(C, np.asarray(x, np.float32), np.float32(0.0)).astype(np.float32)


def mix_noise(P, board, n, radius, noise, w):
    """the noised root priors: float32 multiply, float64 divide and add, float32 store, over the candidates"""
    if radius == 0:
        return forced.mix_noise(P, board, noise, w)
    P = np.asarray(P, np.float32).copy()
    nz = np.zeros(len(P), np.float64)
    nz[np.flatnonzero(np.asarray(board) == 0)] = np.asarray(noise, np.float64)      # nz_c = noise[legal_rank(c)]
    cells = np.flatnonzero(candidate_mask(board, n, radius))
    t = wave_sum(nz, cells, np.float64)
    scaled = (np.float32(1.0 - w) * P[cells]).astype(np.float32)
    P[cells] = (scaled.astype(np.float64) + w * (nz[cells] / t)).astype(np.float32)
    return P


# ---------------------------------------------------------------------------------------------------------------------
# evaluators
# ---------------------------------------------------------------------------------------------------------------------
def synth_evaluator(n, k):
    ev = orc.Oracle(n, k, 1, synthetic=True).synth_eval

    def evaluate(board, player, last):
        P, v = ev(board, player, last)
        return "priors", P, v, None
    return evaluate


def net_evaluator(n, k, onet):
    o = orc.Oracle(n, k, 1)

    def evaluate(board, player, last):
        logits, P, v = onet.eval(o.encode(board, player, last))
        return "logits", logits, v, P
    return evaluate


# ---------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------
def search(evaluate, n, kwin, S, board, player, last, noise=None, forced_k=0.0, c_puct=C_PUCT, w=0.25, L=1, radius=0, info=None):
    """forced.search under the rule -> dict(N, W, P) of the root, zeros on occupied cells.  info (a dict) receives "cand", the
    size of the root's candidate set, and "outside", the root visits that went outside candidate_mask(board, n, info_radius)
    when info["info_radius"] is given (for a plain search: what the rule would have cut)."""
    board = np.asarray(board, np.uint8)
    kind, x, v0, oP = evaluate(board, player, last)
    P0 = expand(kind, x, board, n, radius, oP)
    if noise is not None:
        P0 = mix_noise(P0, board, n, radius, noise, w)
    rows = [_Row(P0)]
    forced_on = forced_k > 0.0 and noise is not None

    def select(total):
        b, pl, la, row, npar, path = board.copy(), player, last, 0, total, []
        while True:
            r = rows[row]
            nv = r.N + r.fl
            wv = r.W - r.fl.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                Q = np.where(nv > 0, wv / nv, 0.0)
            sc = Q + ((c_puct * r.P) * np.sqrt(npar + 1e-8)) / (1 + nv).astype(np.float64)
            if forced_on and row == 0:
                nd = nv.astype(np.float64)
                sc = np.where(nd * nd < (forced_k * r.P) * float(total), np.inf, sc)
            sc = np.where(candidate_mask(b, n, radius), sc, -np.inf)
            a = int(np.argmax(sc))                                 # the first maximum in cell order
            path.append((row, a))
            b[a] = pl
            pl, la = 3 - pl, a
            if forced.wins_through(b, a, n, kwin):
                return path, "term", b, pl, la, -1.0
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
            path, kind_, b, pl, la, tv = select(done + j)
            dup = None
            if kind_ == "expand":
                for i, it in enumerate(items):
                    if it["kind"] == "expand" and it["path"][-1] == path[-1]:
                        kind_, dup = "dup", i
                        break
            for row, a in path:
                rows[row].fl[a] += 1
            items.append(dict(path=path, kind=kind_, b=b, pl=pl, la=la, tv=tv, dup=dup))
        for it in items:
            if it["kind"] == "expand":
                ek, ex, it["v"], eP = evaluate(it["b"], it["pl"], it["la"])
                it["P"] = expand(ek, ex, it["b"], n, radius, eP)
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
    out = dict(N=np.where(legal, r.N, 0).astype(np.int32), W=np.where(legal, r.W, 0.0), P=np.where(legal, r.P, 0.0).astype(np.float32))
    if info is not None:
        info["cand"] = int(candidate_mask(board, n, radius).sum())
        if "info_radius" in info:
            info["outside"] = int(out["N"][~candidate_mask(board, n, info["info_radius"])].sum())
    return out


def search_move(evaluate, n, kwin, S, board, player, last, T, noise, u, forced_k=0.0, do_prune=True, c_puct=C_PUCT, L=1, radius=0,
                log_table=None, table_S=None):
    """one ply: the tree, then pi and the action as forced.search_move makes them (k_move keeps its definition: pi runs over
    the legal cells, a cell without a visit gets what log_table[0] gives it)"""
    r = search(evaluate, n, kwin, S, board, player, last, noise, forced_k, c_puct, L=L, radius=radius)
    legal = np.flatnonzero(np.asarray(board) == 0)
    counts = r["N"][legal]
    if forced_k > 0.0 and noise is not None and do_prune:
        counts = forced.prune(forced_k, c_puct, counts, r["W"][legal], r["P"][legal])
    r["Np"] = np.zeros(n * n, np.int32)
    r["Np"][legal] = counts
    tS = S if table_S is None else table_S
    r["pi"], r["action"] = pi_action(counts, board, T, u, orc.numpy_log_table(tS) if log_table is None else log_table)
    astar = int(np.argmax(r["N"]))
    r["value"] = np.float32(np.float64(r["W"][astar]) / np.float64(r["N"][astar]))
    return r


def selfplay_game(evaluate, n, kwin, S, seed, radius=0, forced_k=0.0, do_prune=True, cap=None, full_fn=None, L=1, board=None,
                  player=1, last=-1, ply0=0, c_puct=C_PUCT, max_plies=0):
    """one self-play game with the game's own tape (oracle.selfplay_tape) and temperature schedule, as tests/selection.py plays
    it.  cap = (fast_sims, permille) with full_fn(seed, ply, permille): a FAST ply gets fast_sims simulations and no noise.
    board / player / last / ply0: the game continues this position at absolute ply ply0.  max_plies > 0: the game is cut after
    that many plies (result 0, z = 99 as the records have it)."""
    nn = n * n
    noise, us = orc.selfplay_tape(seed, n)
    T = orc.selfplay_T_table(nn)
    board = np.zeros(nn, np.uint8) if board is None else np.asarray(board, np.uint8).copy()
    m = ply0
    off = sum(nn - i for i in range(m))
    out = dict(boards=[], movers=[], lasts=[], actions=[], pis=[], visits=[], values=[])
    res = 0
    while not res and (max_plies <= 0 or m - ply0 < max_plies):
        full = cap is None or bool(full_fn(seed, m, cap[1]))
        r = search_move(evaluate, n, kwin, S if full else cap[0], board, player, last, T[m], noise[off:off + nn - m] if full else None,
                        us[m], forced_k, do_prune, c_puct=c_puct, L=L, radius=radius, table_S=S)
        a = r["action"]
        out["boards"].append(board.copy()); out["movers"].append(player); out["lasts"].append(last); out["actions"].append(a)
        out["pis"].append(r["pi"]); out["visits"].append(r["N"]); out["values"].append(r["value"])
        board = board.copy()
        board[a] = player
        res = player if forced.wins_through(board, a, n, kwin) else (3 if not (board == 0).any() else 0)
        last, player, off, m = a, 3 - player, off + nn - m, m + 1
    movers = np.array(out["movers"], np.int64)
    g = dict(boards=np.array(out["boards"], np.uint8), movers=movers.astype(np.uint8), lasts=np.array(out["lasts"], np.int16),
             actions=np.array(out["actions"], np.int16), pis=np.array(out["pis"], np.float32), visits=np.array(out["visits"], np.int32),
             values=np.array(out["values"], np.float32), result=res, nply=m - ply0)
    g["z"] = (np.full(len(movers), 99) if res == 0 else np.zeros(len(movers)) if res == 3 else np.where(movers == res, 1, -1)).astype(np.int8)
    return g


def moves_lie_in_candidates(boards, actions, n, radius):
    """every recorded move is a candidate of the position it was made in"""
    return all(candidate_mask(b, n, radius)[int(a)] for b, a in zip(boards, actions))
