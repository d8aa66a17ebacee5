"""The Gumbel root search (az_set_gumbel), restated in numpy for the tests.

Written from the rule in include/az_engine.h, not from the kernels: the sequential-halving schedule, a float64 tree search that
is PUCT below the root (tests/forced.py's rows and rules) and the equal-N gate with g + logit + sigma(q) at the root, the move,
and the policy target softmax(logit + sigma(completed q)) with np.exp and numpy's own sums.  Any
evaluate(board uint8[nn], player, last) -> (logits float32[nn], P float32[nn], v) serves as the evaluator.  With m = 0, or
without draws, the search is the plain one (tests/test_gumbel_cpu.py holds it to Oracle.search)."""
import numpy as np

from oracle import oracle as orc
from tests import forced
from tests.forced import random_position, wins_through     # noqa: F401  (the positions of the tests)


# ---------------------------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------------------------
def schedule(k, S):
    """seq_k[0 .. S): the visit count a root child must have to be selectable at simulation t"""
    if k <= 1:
        return np.arange(S, dtype=np.int32)
    L = int(np.ceil(np.log2(k)))
    visits, c, out = [0] * k, k, []
    while len(out) < S:
        extra = max(1, S // (L * c))
        for _ in range(extra):
            out.extend(visits[:c])
            for i in range(c):
                visits[i] += 1
        c = max(2, c // 2)
    return np.array(out[:S], np.int32)


def schedule_visits(k, S):
    """the sorted positive visit counts the schedule leaves at the root: child i of the schedule's order is taken once for every
    entry that names it"""
    if k <= 1:
        return [S]
    L = int(np.ceil(np.log2(k)))
    visits, c, n = [0] * k, k, 0
    while n < S:
        extra = max(1, S // (L * c))
        for _ in range(extra):
            for i in range(c):
                if n < S:
                    visits[i] += 1
                    n += 1
        c = max(2, c // 2)
    return sorted(v for v in visits if v > 0)


def sigma(c_visit, c_scale, max_n):
    return (c_visit + float(max_n)) * c_scale


# ---------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------
def search(evaluate, n, kwin, S, board, player, last, g=None, m=0, c_visit=50.0, c_scale=1.0, c_puct=2.0, noise=None, w=0.25,
           mutate=None):
    """MCTS.run's tree -> dict(N, W, P over the cells, zeros on occupied ones; logits float32[nn]; v0; g).  g (one float64 per
    legal cell, row-major) and m > 0: the Gumbel root.  Otherwise the plain search, with `noise` mixed in as Dirichlet noise.
    mutate: a wrong rule for the tests' own teeth ("ge": gate N >= seq, "nomax": sigma without max N)."""
    board = np.asarray(board, np.uint8)
    legal0 = np.flatnonzero(board == 0)
    logits0, P0, v0 = evaluate(board, player, last)
    logits0 = np.asarray(logits0, np.float32)
    gum = m > 0 and g is not None
    if noise is not None and not gum:
        P0 = forced.mix_noise(P0, board, noise, w)
    rows = [forced._Row(P0)]
    if gum:
        seq = schedule(min(m, len(legal0)), S)
        h = np.full(n * n, -np.inf)
        h[legal0] = np.asarray(g, np.float64) + logits0[legal0].astype(np.float64)

    def select(total):
        b, pl, la, row, npar, path = board.copy(), player, last, 0, total, []
        while True:
            r = rows[row]
            with np.errstate(divide="ignore", invalid="ignore"):
                Q = np.where(r.N > 0, r.W / r.N, 0.0)
            if gum and row == 0:
                sig = sigma(c_visit, c_scale, 0 if mutate == "nomax" else r.N[legal0].max())
                sc = h + sig * Q
                gate = (r.N >= seq[total]) if mutate == "ge" else (r.N == seq[total])
                sc = np.where((b == 0) & gate, sc, -np.inf)
                assert np.isfinite(sc).any() or mutate, "no selectable child"
            else:
                sc = Q + ((c_puct * r.P) * np.sqrt(npar + 1e-8)) / (1 + r.N).astype(np.float64)
                sc = np.where(b == 0, sc, -np.inf)
            a = int(np.argmax(sc))                                 # the first maximum in row-major order
            path.append((row, a))
            b[a] = pl
            pl, la = 3 - pl, a
            if wins_through(b, a, n, kwin):
                return path, b, pl, la, -1.0                       # the side to move has lost
            if not (b == 0).any():
                return path, b, pl, la, 0.0
            if r.child[a] == 0:
                return path, b, pl, la, None
            npar, row = int(r.N[a]), int(r.child[a])

    for t in range(S):
        path, b, pl, la, tv = select(t)
        if tv is None:
            _, P, v = evaluate(b, pl, la)
            row, a = path[-1]
            rows[row].child[a] = len(rows)
            rows.append(forced._Row(P))
            tv = float(np.float32(v))
        val = -tv
        for row, a in reversed(path):
            rows[row].N[a] += 1
            rows[row].W[a] += val
            val = -val
    legal = board == 0
    r = rows[0]
    return dict(N=np.where(legal, r.N, 0).astype(np.int32), W=np.where(legal, r.W, 0.0), P=np.where(legal, r.P, 0.0).astype(np.float32),
                logits=logits0, v0=np.float32(v0), g=None if g is None else np.asarray(g, np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# the move and the policy target of one root row of legal children
# ---------------------------------------------------------------------------------------------------------------------
def v_mix(N, W, P, v0):
    N = np.asarray(N, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(N > 0, np.asarray(W, np.float64) / N, 0.0)
    Pd = np.where(N > 0, np.asarray(P, np.float32).astype(np.float64), 0.0)
    pv = np.add.reduce(np.ascontiguousarray(Pd))
    pq = np.add.reduce(np.ascontiguousarray(Pd * q))
    sumN = float(N.sum())
    return (float(np.float32(v0)) + (sumN / pv) * pq) / (1.0 + sumN)


def target(logits, g, N, W, P, v0, c_visit=50.0, c_scale=1.0, mutate=None):
    """(pi float64[count] before the float32 store, index of the move, v_mix).  mutate: "v0" (v0 in place of v_mix), "most"
    (the move = the most visited child)"""
    N = np.asarray(N, np.int64)
    lg = np.asarray(logits, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(N > 0, np.asarray(W, np.float64) / N, 0.0)
    sig = sigma(c_visit, c_scale, N.max())
    score = (np.asarray(g, np.float64) + lg) + sig * q
    action = int(np.argmax(np.where(N == N.max(), score, -np.inf)))
    if mutate == "most":
        action = int(np.argmax(N))
    vm = v_mix(N, W, P, v0)
    qh = np.where(N > 0, q, float(np.float32(v0)) if mutate == "v0" else vm)
    y = lg + sig * qh
    e = np.exp(y - y.max())
    return e / np.add.reduce(e), action, vm


def search_move(evaluate, n, kwin, S, board, player, last, T, draws, u, m=0, c_visit=50.0, c_scale=1.0, c_puct=2.0):
    """one ply: the tree, then the move and pi -- the Gumbel ones when the rule applies (m > 0 and draws given, which are then
    Gumbel draws), else mcts.py:144-177 from the visit counts (draws = Dirichlet noise or None)"""
    board = np.asarray(board, np.uint8)
    gum = m > 0 and draws is not None
    r = search(evaluate, n, kwin, S, board, player, last, g=draws if gum else None, m=m if gum else 0, c_visit=c_visit,
               c_scale=c_scale, c_puct=c_puct, noise=None if gum else draws)
    legal = np.flatnonzero(board == 0)
    if gum:
        pi, a, vm = target(r["logits"][legal], draws, r["N"][legal], r["W"][legal], r["P"][legal], r["v0"], c_visit, c_scale)
        r["pi64"] = np.zeros(n * n)
        r["pi64"][legal] = pi
        r["pi"] = r["pi64"].astype(np.float32)
        r["action"], r["v_mix"] = int(legal[a]), vm
    else:
        r["pi"], r["action"] = forced.pi_action(r["N"][legal], board, T, u, orc.numpy_log_table(S))
    astar = int(np.argmax(r["N"]))
    r["value"] = np.float32(np.float64(r["W"][astar]) / np.float64(r["N"][astar]))
    return r


def selfplay_tape(seed, n, maxply=None):
    """the per-game tape under the option, from numpy's own legacy RNG: per ply p, gumbel(size = nn - p) then one uniform"""
    nn = n * n
    rs = np.random.RandomState(seed)
    noise, us = [], []
    for p in range(nn if maxply is None else maxply):
        noise.append(rs.gumbel(size=nn - p))
        us.append(rs.random_sample())
    return np.concatenate(noise), np.array(us, np.float64)


def selfplay_game(evaluate, n, kwin, S, tape, m, c_visit=50.0, c_scale=1.0, cap=None, full_fn=None, seed=0):
    """one self-play game from the empty board on the given tape (noise, us).  cap = (fast_sims, permille) with
    full_fn(seed, ply, permille) -> bool: FAST plies get fast_sims simulations of the plain search without noise."""
    nn = n * n
    noise, us = tape
    T = orc.selfplay_T_table(nn)
    board, player, last, p, off = np.zeros(nn, np.uint8), 1, -1, 0, 0
    out = dict(boards=[], movers=[], lasts=[], actions=[], pis=[], pis64=[], visits=[], values=[], full=[])
    while True:
        full = cap is None or bool(full_fn(seed, p, cap[1]))
        r = search_move(evaluate, n, kwin, S if full else cap[0], board, player, last, T[p], noise[off:off + nn - p] if full else None,
                        us[p], m, c_visit, c_scale)
        a = r["action"]
        out["boards"].append(board.copy()); out["movers"].append(player); out["lasts"].append(last); out["actions"].append(a)
        out["pis"].append(r["pi"]); out["pis64"].append(r.get("pi64", r["pi"].astype(np.float64)))
        out["visits"].append(r["N"]); out["values"].append(r["value"]); out["full"].append(full)
        board = board.copy()
        board[a] = player
        res = player if wins_through(board, a, n, kwin) else (3 if not (board == 0).any() else 0)
        last, player, off, p = a, 3 - player, off + nn - p, p + 1
        if res:
            break
    movers = np.array(out["movers"], np.int64)
    game = dict(boards=np.array(out["boards"], np.uint8), movers=movers.astype(np.uint8), lasts=np.array(out["lasts"], np.int16),
                actions=np.array(out["actions"], np.int16), pis=np.array(out["pis"], np.float32), pis64=np.array(out["pis64"]),
                visits=np.array(out["visits"], np.int32), values=np.array(out["values"], np.float32),
                full=np.array(out["full"], bool), result=res, nply=p)
    game["z"] = (np.zeros(p) if res == 3 else np.where(movers == res, 1, -1)).astype(np.int8)
    return game


def within_one_float32_step(got, want64):
    """got float32 against the float64 value it should be the rounding of: at most one float32 spacing away from float32(want)"""
    got = np.asarray(got, np.float32)
    want = np.asarray(want64, np.float64).astype(np.float32)
    return bool(np.all((got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))))
