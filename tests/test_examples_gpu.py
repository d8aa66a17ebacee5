"""The training-data path on every board size and record shape: k_move's record buffers -> k_pack (az_selfplay_pack) ->
k_examples (az_examples_from_packed) / k_examples_gather (az_examples_gather, DeviceReplayBuffer) -> (state, pi, z).

Everything is compared EXACTLY (bytes, float bit patterns, labels) with tests/examples_ref.py, an independent numpy
reference written from the documented record layout and the reference's definition of an example, fed with the CPU oracle's
games.  The search is not under test here: synthetic evaluator, a handful of simulations."""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import examples_ref as ref
from tests.util import weights_from_fixture

import alphazero_piskvorky_amd as az

S = 8
DEV = "cuda:0"
GUARD = 4096                      # floats (bytes for packed records) of canary behind every output buffer
# (n, k, games, slots, max_plies): every size 3..15 with complete games and more games than slots (slots are refilled);
# 3x3 and 4x4 for the draws; two cut episodes (8x8 two plane words and a padded stride, 14x14 four words and a padded stride)
EPISODES = [(3, 3, 12, 4, 0), (4, 4, 8, 3, 0), (5, 4, 6, 4, 0), (6, 5, 6, 4, 0), (7, 5, 6, 4, 0), (8, 5, 6, 4, 0),
            (8, 5, 6, 4, 7), (9, 5, 6, 4, 0), (10, 5, 6, 4, 0), (11, 5, 6, 4, 0), (12, 5, 6, 4, 0), (13, 5, 6, 4, 0),
            (14, 5, 6, 4, 0), (14, 5, 6, 4, 5), (15, 5, 6, 4, 0)]


def _seed0(n):
    return 900 + n


@functools.lru_cache(maxsize=None)
def _oracle_games(n, k, sims, G, seed0, cut, net_tag=None):
    o = orc.Oracle(n, k, sims, synthetic=net_tag is None)
    net = None if net_tag is None else orc.Net(n, weights_from_fixture(n, net_tag))
    out = []
    for g in range(G):
        noise, us = orc.selfplay_tape(seed0 + g, n, maxply=cut or None)
        out.append(o.selfplay_game(net, noise, us, maxply=cut or None))
    return out


def _engine(n, k, sims, slots, **kw):
    kw.setdefault("synthetic", True)
    return az.Engine(n, k, sims, slots, log_table=orc.numpy_log_table(sims), **kw)


def _packed(e, R):
    """The episode's packed records as numpy bytes; the canary behind the last record must survive."""
    rb = e.record_bytes
    buf = torch.full((R * rb + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    e.pack_into(buf.data_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[R * rb:] == 0xEE).all(), "az_selfplay_pack wrote behind the last record"
    return buf, host[:R * rb]


class _Out:
    """NaN-filled output buffers for B examples with a NaN canary behind them."""

    def __init__(self, B, n):
        self.B, self.n, nn = B, n, n * n
        nan = float("nan")
        self.st = torch.full((B * 4 * nn + GUARD,), nan, dtype=torch.float32, device=DEV)
        self.pi = torch.full((B * nn + GUARD,), nan, dtype=torch.float32, device=DEV)
        self.z = torch.full((B + GUARD,), nan, dtype=torch.float32, device=DEV)

    def ptrs(self):
        return self.st.data_ptr(), self.pi.data_ptr(), self.z.data_ptr()

    def read(self, what):
        """(states, pis, z) on the host; every cell written, nothing behind the last example touched."""
        torch.cuda.synchronize()
        B, n, nn = self.B, self.n, self.n * self.n
        out = []
        for name, t, per in (("states", self.st, 4 * nn), ("pis", self.pi, nn), ("z", self.z, 1)):
            h = t.cpu().numpy()
            assert not np.isnan(h[:B * per]).any(), f"{what}: {name} cells left unwritten"
            assert np.isnan(h[B * per:]).all(), f"{what}: {name} written behind the last example"
            out.append(h[:B * per])
        return out[0].reshape(B, 4, n, n), out[1].reshape(B, n, n), out[2]

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in (self.st, self.pi, self.z))


def _equal(got, want, what):
    for name, g, w in zip(("states", "pis", "z"), got, want):
        assert g.shape == w.shape, f"{what}: {name} shape"
        assert np.array_equal(ref.bits(g), ref.bits(w)), f"{what}: {name} differ in {int((ref.bits(g) != ref.bits(w)).sum())} cells"


def _from_packed(e, buf, R, aug):
    out = _Out(R * aug, e.n)
    e.examples_from_packed(buf.data_ptr(), R, aug, *out.ptrs())
    return out.read(f"examples_from_packed aug={aug}")


def _gather(e, buf, idx, sym, reference_pi):
    out = _Out(len(idx), e.n)
    ti = torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int64, device=DEV)
    ts = torch.as_tensor(np.ascontiguousarray(sym), dtype=torch.int32, device=DEV)
    e.examples_gather(buf.data_ptr(), ti.data_ptr(), ts.data_ptr(), len(idx), reference_pi, *out.ptrs())
    return out.read(f"examples_gather reference_pi={reference_pi}")


# ---- a. every size ----
@pytest.mark.parametrize("n,k,G,slots,cut", EPISODES)
def test_every_size_packed_records_and_examples_equal_the_reference(n, k, G, slots, cut):
    games = _oracle_games(n, k, S, G, _seed0(n), cut)
    want = ref.expected_records(games)
    # the helper's label (from result and mover) is the oracle's own z
    assert np.array_equal(want["z"], np.concatenate([g["z"] for g in games]))
    e = _engine(n, k, S, slots)
    assert e.record_bytes == ref.record_bytes(n)
    c = e.selfplay(G, seed0=_seed0(n), max_plies=cut)
    R = c["records"]
    assert R == len(want["z"]) and R > slots
    buf, host = _packed(e, R)
    got = ref.unpack(host, n)
    assert not ref.same(got, want), f"packed records differ from the oracle's games in {ref.same(got, want)}"
    raw = ref.records_from_host(e.records())
    assert not ref.same(got, raw), f"az_selfplay_pack and az_selfplay_records disagree in {ref.same(got, raw)}"
    for aug in (1, 4, 8):
        _equal(_from_packed(e, buf, R, aug), ref.expected_examples(want, n, aug), f"n={n} aug={aug}")
    rs = np.random.RandomState(n)
    # dihedral pi, all eight symmetries, indices with repetition and in no order, more examples than records
    idx, sym = rs.randint(0, R, R + 37), rs.randint(0, 8, R + 37)
    assert len(set(idx.tolist())) < len(idx) and set(sym.tolist()) == set(range(8))
    _equal(_gather(e, buf, idx, sym, 0), ref.expected_gather(want, n, idx, sym, 0), f"n={n} gather dihedral")
    # the ring's reference mode: rotations only, pi rotated once
    idx, sym = rs.permutation(R)[:min(R, 50)], rs.randint(0, 4, min(R, 50))
    _equal(_gather(e, buf, idx, sym, 1), ref.expected_gather(want, n, idx, sym, 1), f"n={n} gather reference")
    # nothing to do: no buffer is touched
    out = _Out(4, n)
    e.examples_from_packed(buf.data_ptr(), 0, 8, *out.ptrs())
    ti = torch.zeros(4, dtype=torch.int64, device=DEV); ts = torch.zeros(4, dtype=torch.int32, device=DEV)
    e.examples_gather(buf.data_ptr(), ti.data_ptr(), ts.data_ptr(), 0, 0, *out.ptrs())
    assert out.untouched()
    e.close()


# ---- b. every label occurs ----
def test_the_episodes_contain_every_label_and_every_plane_word():
    """Asserted on the oracle's results, so that a later change of seeds or sizes cannot silently drop a case."""
    results, cut_results, first_ply = collections.Counter(), collections.Counter(), 0
    for n, k, G, slots, cut in EPISODES:
        games = _oracle_games(n, k, S, G, _seed0(n), cut)
        (cut_results if cut else results).update(g["result"] for g in games)
        rec = ref.expected_records(games)
        first_ply += int((rec["last"] == -1).sum())
        assert int((rec["last"] == -1).sum()) == G
        if not cut:
            # stones of both sides in the LAST plane word of the size (word 0 alone is all that 5x5 ever used)
            top = ((n * n - 1) >> 6) << 6
            assert rec["me"][:, top:].any() and rec["opp"][:, top:].any(), f"n={n}: no stone in plane word {top >> 6}"
            assert set(np.unique(rec["z"]).tolist()) <= {-1, 0, 1}
        else:
            assert set(g["result"] for g in games) == {0} and (rec["z"] == ref.CUT).all()
    assert results[3] >= 3 and results[1] >= 10 and results[2] >= 10        # draws, wins of each colour
    assert set(results) == {1, 2, 3} and cut_results[0] == 12 and first_ply > 0
    assert {n for n, *_ in EPISODES} == set(range(3, 16))
    assert {n for n, *_, cut in EPISODES if cut} == {8, 14}                  # both cut episodes have a padded stride


# ---- c. the cut-game label is a decision: 99, as include/az_engine.h says ----
@pytest.mark.parametrize("n,k,cut", [(8, 5, 7), (14, 5, 5)])
def test_cut_games_carry_z_99_through_both_example_kernels(n, k, cut):
    e = _engine(n, k, S, 2)
    c = e.selfplay(3, seed0=_seed0(n), max_plies=cut)
    R = c["records"]
    assert R == 3 * cut and (e.games()[1] == 0).all()
    assert (e.records()["z"] == 99).all()
    buf, host = _packed(e, R)
    assert (ref.unpack(host, n)["z"] == 99).all()
    for aug in (1, 4, 8):
        z = _from_packed(e, buf, R, aug)[2]
        assert z.dtype == np.float32 and len(z) == R * aug and (z == np.float32(99.0)).all()
    z = _gather(e, buf, np.arange(R)[::-1], np.arange(R) % 8, 0)[2]
    assert len(z) == R and (z == np.float32(99.0)).all()
    e.close()


# ---- d. lanes, refill and compaction ----
@pytest.mark.parametrize("compact", ["1", "0"])
@pytest.mark.parametrize("n,k,sims,G,slots,cut,net", [(9, 5, 6, 10, 6, 0, None), (15, 5, 6, 14, 6, 6, None), (15, 5, 8, 8, 5, 3, "seeded")])
def test_packed_records_with_lanes_refill_and_compaction(n, k, sims, G, slots, cut, net, compact, monkeypatch):
    """az_selfplay_pack reads lane 0's view of the record buffers and orders by game id: three lanes, fewer slots than games,
    games of different lengths (9x9 plays to the end) and slot compaction on and off must all give the oracle's episode --
    once with the real net and the seeded weights, so that pi is not the synthetic evaluator's."""
    monkeypatch.setenv("AZ_COMPACT", compact)
    seed0 = 4000 + n
    games = _oracle_games(n, k, sims, G, seed0, cut, net)
    want = ref.expected_records(games)
    e = _engine(n, k, sims, slots, engines=3, synthetic=net is None)
    assert e.lanes() == 3
    if net:
        e.load_weights(weights_from_fixture(n, net), 0)
    c = e.selfplay(G, seed0=seed0, max_plies=cut)
    R = c["records"]
    assert R == len(want["z"])
    if not cut:
        assert len({g["nply"] for g in games}) > 3         # slots really empty at different plies
    buf, host = _packed(e, R)
    got = ref.unpack(host, n)
    assert not ref.same(got, ref.records_from_host(e.records()))
    assert not ref.same(got, want), f"packed records differ from the oracle's games in {ref.same(got, want)}"
    _equal(_from_packed(e, buf, R, 8), ref.expected_examples(want, n, 8), f"n={n} lanes")
    e.close()


# ---- e. DeviceReplayBuffer on the device ----
@pytest.mark.parametrize("n,aug,capacity", [(14, 4, 40), (14, 1, 10), (14, 8, 80), (14, 4, 43), (9, 4, 40), (9, 1, 10), (9, 8, 80),
                                            (9, 8, 83)])
def test_device_replay_ring_follows_a_deque(n, aug, capacity):
    """A scripted life of the ring (14x14: padded 856-byte stride, four plane words) against collections.deque(maxlen):
    empty, a few records, across the wrap at a non-zero head, nothing, more than the capacity, and on."""
    from alphazero_piskvorky_amd.device_replay import DeviceReplayBuffer
    e = _engine(n, 5, 4, 1)
    cap = capacity // aug
    assert cap == 10
    buf = DeviceReplayBuffer(e, capacity=capacity, aug=aug, device=DEV, seed=n + aug)
    assert buf.cap == cap and buf.ring.numel() == cap * ref.record_bytes(n)
    rs = np.random.RandomState(capacity)
    model = collections.deque(maxlen=cap)
    pool = ref.random_records(rs, n, 0)
    # an empty ring gives three empty tensors of the right shapes (the reference's sample_batch returns nothing)
    s, p, z = buf.sample_batch(16)
    assert tuple(s.shape) == (0, 4, n, n) and tuple(p.shape) == (0, n, n) and tuple(z.shape) == (0,)
    ref.check_ring(buf, model, pool, n, aug)
    heads = []
    for R in (4, 9, 0, 23, 3, 10):
        new = ref.random_records(rs, n, R)
        first = len(pool["z"])
        pool = {key: np.concatenate([pool[key], new[key]]) for key in ref.FIELDS}
        packed = torch.from_numpy(ref.pack(new, n, fill=0xA5)).to(DEV)      # junk in the padding bytes
        heads.append(buf.head)
        buf.extend_packed(packed, R)
        model.extend(range(first, first + R))
        ref.check_ring(buf, model, pool, n, aug)
        ref.check_ring(buf, model, pool, n, aug, sample=7)
    assert heads[1] == 4 and heads[1] + 9 > cap          # the second extend wrapped at a non-zero head
    e.close()


# ---- f. the seam ----
@functools.lru_cache(maxsize=None)
def _seam_games(n, sims, G, seed):
    from alphazero_piskvorky_amd import constants
    from alphazero_piskvorky_amd.mcts import numpy_log_table
    from alphazero_piskvorky_amd.self_play import default_temperature_schedule
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    k = min(constants.WIN_LENGTH, n)
    o = orc.Oracle(n, k, sims, c_puct=constants.SELF_PLAY_EXPLORATION_CONSTANT, log_table=numpy_log_table(sims))
    net = orc.Net(n, synthetic_state_dict(n))
    T = np.array([float(default_temperature_schedule(m)) for m in range(n * n + 1)], dtype=np.float64)
    out = []
    for g in range(G):
        noise, us = orc.selfplay_tape(seed + g, n)
        out.append(o.selfplay_game(net, noise, us, T_table=T))
    return out


@pytest.mark.parametrize("aug", [4, 8])
@pytest.mark.parametrize("n", [6, 9])
def test_generate_self_play_returns_the_reference_examples(n, aug):
    """SelfPlayManager.generate_self_play at an even size (padded stride) and at 9x9 (two plane words): the tuples are the
    reference's examples of the oracle's games in (game, ply, k) order, z a Python int."""
    from alphazero_piskvorky_amd.controller import NeuralNetworkController
    from alphazero_piskvorky_amd.net import GomokuNet
    from alphazero_piskvorky_amd.self_play import SelfPlayManager
    from alphazero_piskvorky_amd.weights import synthetic_state_dict
    sims, G, seed = 8, 4, 500 + n
    m = GomokuNet(board_size=n)
    m.load_state_dict({key: torch.tensor(v) for key, v in synthetic_state_dict(n).items()})
    m.eval()
    mgr = SelfPlayManager(NeuralNetworkController(m, device=DEV), DEV, mcts_params={"num_simulations": sims}, concurrent_games=3,
                          augmentation=aug, seed=seed)
    data = mgr.generate_self_play(G)
    want = ref.expected_examples(ref.expected_records(_seam_games(n, sims, G, seed)), n, aug)
    assert len(data) == len(want[2]) and len(data) > 0
    assert all(isinstance(s, torch.Tensor) and s.device.type == "cpu" and isinstance(p, np.ndarray) and type(z) is int for s, p, z in data)
    _equal((np.stack([s.numpy() for s, _, _ in data]), np.stack([p for _, p, _ in data]), np.array([z for _, _, z in data], np.float32)),
           want, f"generate_self_play n={n} aug={aug}")
    assert [z for _, _, z in data] == want[2].astype(np.int64).tolist()
    mgr._engine.close()
