"""Independent numpy reference for the training-data path: packed records -> (state, pi, z) examples.

Written from the record layout documented in include/az_engine.h (and above k_pack in csrc/az_engine.hip) and from the
reference's definition of an example (games.py:106-129 encode, self_play.py:71 label, self_play.py:94-108 augmentation),
not from the kernels: symmetries are np.rot90 / [..., ::-1], never an index formula.

A "records" value is a dict of per-position arrays:
    me, opp  uint8 [R, n*n]   1 where the mover / the opponent has a stone
    pi       float32 [R, n*n]
    last     int16 [R]        cell of the previous move, -1 at the first ply
    mover    uint8 [R]        1 or 2
    z        int8 [R]         +1 mover won, -1 mover lost, 0 draw, CUT for a game cut by max_plies
"""
import numpy as np

CUT = 99                      # label of a game that max_plies ended before it was decided
FIELDS = ("me", "opp", "pi", "last", "mover", "z")


def record_bytes(n):
    """[8 x u64 planes: mover words 0..3, opponent words 4..7][pi f32 x n*n][last i16][mover u8][z i8], padded to 8 bytes."""
    return (64 + 4 * n * n + 4 + 7) // 8 * 8


def unpack(packed_bytes, n):
    """Packed bytes (whole records, padded stride) -> records."""
    nn, rb = n * n, record_bytes(n)
    a = np.ascontiguousarray(packed_bytes, dtype=np.uint8).reshape(-1, rb)
    words = np.ascontiguousarray(a[:, :64]).view("<u8")                          # [R, 8]
    cell = np.arange(nn)
    word, bit = cell >> 6, (cell & 63).astype(np.uint64)
    tail = 64 + 4 * nn
    return dict(me=((words[:, word] >> bit) & np.uint64(1)).astype(np.uint8),
                opp=((words[:, 4 + word] >> bit) & np.uint64(1)).astype(np.uint8),
                pi=np.ascontiguousarray(a[:, 64:tail]).view("<f4"),
                last=np.ascontiguousarray(a[:, tail:tail + 2]).view("<i2")[:, 0],
                mover=a[:, tail + 2].copy(),
                z=a[:, tail + 3].copy().view(np.int8))


def _records(boards, movers, lasts, pis, z):
    boards = np.asarray(boards, np.uint8)
    movers = np.asarray(movers, np.uint8)
    return dict(me=(boards == movers[:, None]).astype(np.uint8), opp=(boards == 3 - movers[:, None]).astype(np.uint8),
                pi=np.asarray(pis, np.float32), last=np.asarray(lasts, np.int16), mover=movers, z=np.asarray(z, np.int8))


def label(result, movers):
    """self_play.py:71: 0 for a draw (result 3), +1 where the mover is the winner (result 1 / 2), else -1; CUT for result 0."""
    movers = np.asarray(movers, np.int64)
    if result == 0:
        return np.full(len(movers), CUT, np.int8)
    if result == 3:
        return np.zeros(len(movers), np.int8)
    return np.where(movers == result, 1, -1).astype(np.int8)


def expected_records(oracle_games):
    """Records of an episode from the CPU oracle's selfplay_game results, game-major then ply."""
    gs = list(oracle_games)
    n2 = gs[0]["boards"].shape[1]
    cat = lambda key, shape, dt: np.concatenate([np.asarray(g[key], dt).reshape((-1,) + shape) for g in gs])
    z = np.concatenate([label(g["result"], g["movers"]) for g in gs])
    return _records(cat("boards", (n2,), np.uint8), cat("movers", (), np.uint8), cat("lasts", (), np.int16),
                    cat("pis", (n2,), np.float32), z)


def records_from_host(rec):
    """Engine.records() (absolute boards) re-expressed as records."""
    return _records(rec["boards"], rec["movers"], rec["lasts"], rec["pis"], rec["z"])


def take(records, idx):
    idx = np.asarray(idx, np.int64)
    return {k: records[k][idx] for k in FIELDS}


def same(a, b):
    """Names of the fields in which two records values differ (pi by its bits)."""
    bad = []
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "pi":
            x, y = np.ascontiguousarray(x, np.float32).view(np.uint32), np.ascontiguousarray(y, np.float32).view(np.uint32)
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(k)
    return bad


def states_of(records, n):
    """games.py:106-129: plane 0 the mover's stones, 1 the opponent's, 2 the last move (empty at the first ply), 3 empty."""
    R = len(records["z"])
    s = np.zeros((R, 4, n * n), np.float32)
    s[:, 0] = records["me"]
    s[:, 1] = records["opp"]
    has = np.flatnonzero(records["last"] >= 0)
    s[has, 2, records["last"][has].astype(np.int64)] = 1.0
    return s.reshape(R, 4, n, n)


def _sym(x, k):
    """Dihedral symmetry k of the last two axes: k < 4 rot90 k times, k >= 4 rot90(fliplr, k - 4)."""
    a, b = x.ndim - 2, x.ndim - 1
    return np.rot90(x, k, (a, b)) if k < 4 else np.rot90(x[..., ::-1], k - 4, (a, b))


def expected_examples(records, n, aug):
    """(states [R*aug, 4, n, n], pis [R*aug, n, n], z [R*aug]) in (record, k) order.  aug 1: identity; aug 4: the reference's
    _augment_symmetries (state rot90 k times, pi rot90 exactly ONCE for every k); aug 8: the dihedral group on both."""
    assert aug in (1, 4, 8)
    R = len(records["z"])
    s0 = states_of(records, n)
    p0 = np.asarray(records["pi"], np.float32).reshape(R, n, n)
    st = np.empty((R, aug, 4, n, n), np.float32)
    pi = np.empty((R, aug, n, n), np.float32)
    for k in range(aug):
        st[:, k] = _sym(s0, k)
        pi[:, k] = np.rot90(p0, 1, (1, 2)) if aug == 4 else _sym(p0, k)
    z = np.repeat(records["z"].astype(np.float32), aug)
    return st.reshape(R * aug, 4, n, n), pi.reshape(R * aug, n, n), z


def expected_gather(records, n, idx, sym, reference_pi):
    """Example i = symmetry sym[i] (0..7) of record idx[i]; reference_pi: pi rotated once whatever the symmetry."""
    idx, sym = np.asarray(idx, np.int64), np.asarray(sym, np.int64)
    sub = take(records, idx)
    B = len(idx)
    s0 = states_of(sub, n)
    p0 = np.asarray(sub["pi"], np.float32).reshape(B, n, n)
    st = np.empty((B, 4, n, n), np.float32)
    pi = np.empty((B, n, n), np.float32)
    for k in range(8):
        m = np.flatnonzero(sym == k)
        if len(m):
            st[m] = _sym(s0[m], k)
            pi[m] = np.rot90(p0[m], 1, (1, 2)) if reference_pi else _sym(p0[m], k)
    return st, pi, sub["z"].astype(np.float32)


def bits(x):
    """float32 array -> its bit patterns, so that comparisons are exact and NaN-safe."""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def pack(records, n, fill=0):
    """records -> packed bytes (the inverse of unpack; padding bytes = fill).  For tests that feed the kernels hand-made records."""
    nn, rb = n * n, record_bytes(n)
    R = len(records["z"])
    out = np.full((R, rb), fill, np.uint8)
    words = np.zeros((R, 8), np.uint64)
    cell = np.arange(nn)
    for c in cell:
        words[:, c >> 6] |= records["me"][:, c].astype(np.uint64) << np.uint64(c & 63)
        words[:, 4 + (c >> 6)] |= records["opp"][:, c].astype(np.uint64) << np.uint64(c & 63)
    tail = 64 + 4 * nn
    out[:, :64] = words.view(np.uint8)
    out[:, 64:tail] = np.ascontiguousarray(records["pi"], "<f4").view(np.uint8).reshape(R, 4 * nn)
    out[:, tail:tail + 2] = np.ascontiguousarray(records["last"], "<i2").view(np.uint8).reshape(R, 2)
    out[:, tail + 2] = records["mover"]
    out[:, tail + 3] = np.asarray(records["z"], np.int8).view(np.uint8)
    return out.reshape(-1)


# ---- shared by the ring tests (CPU stand-in and device) ----
def random_records(rs, n, R):
    """R hand-made positions: random stones anywhere on the board, a random pi, every label, first-ply records now and then."""
    nn = n * n
    cells = rs.randint(0, 3, (R, nn))
    return dict(me=(cells == 1).astype(np.uint8), opp=(cells == 2).astype(np.uint8),
                pi=rs.random_sample((R, nn)).astype(np.float32), last=rs.randint(-1, nn, R).astype(np.int16),
                mover=rs.randint(1, 3, R).astype(np.uint8), z=rs.choice([-1, 0, 1, CUT], R).astype(np.int8))


def rows(states, pis, zs):
    """Multiset of examples: one bytes key per example."""
    import collections
    s, p, z = (np.asarray(x) for x in (states, pis, zs))
    B = len(z)
    if B == 0:
        return collections.Counter()
    m = np.concatenate([bits(s).reshape(B, -1), bits(p).reshape(B, -1), bits(z).reshape(B, 1)], axis=1)
    return collections.Counter(r.tobytes() for r in m)


def check_ring(buf, model, pool, n, aug, sample=None):
    """A DeviceReplayBuffer against the reference's buffer, a deque of record ids into `pool`: len, the order of
    export_examples, and a sample_batch (default: more than the ring holds, i.e. every example exactly once)."""
    import torch
    want = expected_examples(take(pool, list(model)), n, aug)
    total = len(model) * aug
    assert len(buf) == total
    ex = buf.export_examples()
    assert len(ex) == total
    if total:
        assert all(isinstance(e[0], torch.Tensor) and isinstance(e[1], np.ndarray) and isinstance(e[2], int) for e in ex[:3])
        assert np.array_equal(bits(np.stack([e[0].numpy() for e in ex])), bits(want[0])), "export_examples: states"
        assert np.array_equal(bits(np.stack([e[1] for e in ex])), bits(want[1])), "export_examples: pis"
        assert [e[2] for e in ex] == want[2].astype(np.int64).tolist(), "export_examples: z"
    b = total + 5 if sample is None else sample
    s, p, z = buf.sample_batch(b)
    k = min(b, total)
    assert tuple(s.shape) == (k, 4, n, n) and tuple(p.shape) == (k, n, n) and tuple(z.shape) == (k,)
    assert s.dtype == p.dtype == z.dtype == torch.float32
    got, all_rows = rows(s.cpu(), p.cpu(), z.cpu()), rows(*want)
    if k == total:
        assert got == all_rows, "sample_batch: not every example exactly once"
    else:
        assert not got - all_rows, "sample_batch: an example that is not in the ring"
