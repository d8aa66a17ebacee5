"""The engine at extreme net magnitudes (tests/numeric.py): confident nets, exact rescalings, the emulated trunks against
the float64 bound.

  * G10 (netgame_confident_5x4.npz, the reference's games under C_{5,4}): on every ply the engine's visit counts equal the
    reference's, P is 0 exactly where torch's softmax is 0, and equals the oracle's bit for bit.  Without the gradual
    underflow of az_expf, record 100 (game 5, ply 14) gets other visit counts;
  * confident nets (C_{p,v}: zero and subnormal priors, values of exactly +-1) bit-exact against the oracle on the fused
    and the split trunk, self-play on the persistent kernel and the lock-step pipeline, cut 9x9 / 15x15 games, the
    ResidualBlock net, leaf symmetry, the eval cache, subtree reuse, virtual loss and the arena;
  * T_a (an exact power-of-two rescaling of the trunk) changes no bit of net_eval (fused, split, bf16x3) or of an episode;
  * the bf16x3 and f16x2 trunks stay within their mode's float64 error bound.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import numeric as nm
from tests.util import load, weights_from_fixture

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd.net import fold_resnet_state_dict
from alphazero_piskvorky_amd.weights import synthetic_resnet_state_dict

SPLIT_MODES = ["0", "1000000"]     # AZ_SPLIT_MAX: fused trunk only | split (low-latency) trunk forced


def _engine(monkeypatch, n, k, S, slots, split=None, persist=None, model="plain"):
    if split is not None:
        monkeypatch.setenv("AZ_SPLIT_MAX", split)
    if persist is not None:
        monkeypatch.setenv("AZ_PERSIST", persist)
    return az.Engine(n, k, S, slots, log_table=orc.numpy_log_table(S), model=model)


def _positions(n, count, seed):
    rs = np.random.RandomState(seed)
    nn = n * n
    boards = np.zeros((count, nn), np.uint8); players = np.zeros(count, np.uint8); lasts = -np.ones(count, np.int16)
    for i in range(count):
        m = int(rs.randint(0, (2 * nn) // 3))
        cells = rs.permutation(nn)[:m]
        boards[i, cells[0::2]] = 1; boards[i, cells[1::2]] = 2
        players[i] = 1 + (m & 1)
        lasts[i] = cells[-1] if m else -1
    return boards, players, lasts


def _planes(n, boards, players, lasts):
    o = orc.Oracle(n, 5, 1)
    return np.array([o.encode(boards[i], int(players[i]), int(lasts[i])) for i in range(len(boards))])


def _weights(n, tag, kind=None, arg=None):
    """(engine weights, oracle net, model, float64 forward) of a net under a transform ('T', a) / ('C', (p, v))."""
    res = tag == "resnet"
    sd = synthetic_resnet_state_dict(n) if res else weights_from_fixture(n, tag)
    if kind == "T":
        sd = (nm.resnet_scale_invariance if res else nm.scale_invariance)(sd, arg)
    elif kind == "C":
        sd = nm.confidence(sd, *arg)
    if res:
        t = fold_resnet_state_dict(sd)
        return t, orc.Net(n, resnet_tensors=t), "resnet", (lambda x, mode="f32": nm.resnet_forward(t, x, mode))
    return sd, orc.Net(n, sd), "plain", (lambda x, mode="f32": nm.gomoku_forward(sd, x, mode))


# ------------------------------------------------------------------ G10
@pytest.mark.parametrize("split", SPLIT_MODES)
def test_confident_net_games_vs_reference(monkeypatch, split):
    z = load("netgame_confident_5x4.npz")
    n, k, S = int(z["n"]), int(z["k"]), int(z["S"])
    p, v = (int(c) for c in z["confidence"])
    sd = nm.confidence(weights_from_fixture(n, str(z["weights"])), p, v)
    e = _engine(monkeypatch, n, k, S, 4, split=split)
    e.load_weights(sd, 0)
    o = orc.Oracle(n, k, S); onet = orc.Net(n, sd)
    nn = n * n
    for g in np.unique(z["game"]):
        sel = np.where(z["game"] == g)[0]
        tape, us = orc.selfplay_tape(int(z["seed0"]) + int(g), n)
        off = 0
        for idx in sel:
            ply = int(z["ply"][idx]); A = nn - ply
            noise = tape[off:off + A]; off += A
            args = (z["board"][idx], int(z["player"][idx]), int(z["last"][idx]), float(z["T"][idx]), noise, us[ply])
            r = e.search(*args)
            assert np.array_equal(r["N"], z["N"][idx]), f"visit counts differ from the reference: record {idx} (game {g} ply {ply})"
            assert np.array_equal(r["P"] == 0, z["P"][idx] == 0), f"zero pattern of P differs: record {idx}"
            assert np.all(np.abs(r["P"] - z["P"][idx]) <= nm.p_bar(z["P"][idx], p)), f"P: record {idx}"
            assert r["action"] == int(z["action"][idx])
            ro = o.search(onet, *args)
            assert np.array_equal(r["P"], ro["P"]) and np.array_equal(r["W"], ro["W"]) and np.array_equal(r["pi"], ro["pi"])
    e.close()


# ------------------------------------------------------------------ confident nets, bit for bit
@pytest.mark.parametrize("split", SPLIT_MODES)
@pytest.mark.parametrize("n,tag", [(5, "ckpt_saved"), (9, "seeded"), (15, "seeded"), (9, "resnet")])
def test_confident_net_eval_bit_exact_vs_oracle(monkeypatch, n, tag, split):
    boards, players, lasts = _positions(n, 24, 31 + n)
    planes = _planes(n, boards, players, lasts)
    for conf in ((5, 4), (7, 6)):
        sd, onet, model, fwd = _weights(n, tag, "C", conf)
        nm.assert_sane(fwd(planes))                    # finite and in range before the launch
        e = _engine(monkeypatch, n, 5 if n > 5 else 4, 8, 32, split=split, model=model)
        e.load_weights(sd, 0)
        lg, P, v = e.net_eval(boards, players, lasts)
        e.close()
        zero = sub = sat = 0
        for i in range(len(boards)):
            ol, oP, ov = onet.eval(planes[i])
            assert np.array_equal(lg[i], ol), f"C{conf} board {i}: logits differ from the oracle"
            assert np.array_equal(P[i], oP), f"C{conf} board {i}: priors differ from the oracle"
            assert v[i] == np.float32(ov), f"C{conf} board {i}: value differs from the oracle"
            zero += int((P[i] == 0).sum()); sub += int(((P[i] > 0) & (P[i] < 2.0 ** -126)).sum()); sat += int(abs(v[i]) == 1)
        if conf == (7, 6):
            assert sub > 0 and zero > 0 and sat > 0, (sub, zero, sat)


def _selfplay_vs_oracle(e, o, onet, G, seed0, cut=0):
    e.selfplay(G, seed0=seed0, max_plies=cut)
    rec = e.records(); nply, res = e.games()
    off = 0
    for g in range(G):
        noise, us = orc.selfplay_tape(seed0 + g, o.n)
        r = o.selfplay_game(onet, noise, us, maxply=cut or None, game=seed0 + g)
        L = int(nply[g]); sl = slice(off, off + L)
        assert L == r["nply"], f"game {g}: length differs from the oracle"
        if not cut:
            assert int(res[g]) == r["result"]
        for key in ("actions", "boards", "visits", "pis", "z"):
            assert np.array_equal(rec[key][sl], r[key]), f"game {g}: {key} differs from the oracle"
        off += L


@pytest.mark.parametrize("persist", ["1", "0"])
def test_confident_selfplay_5x5_vs_oracle(monkeypatch, persist):
    sd, onet, _, _ = _weights(5, "ckpt_saved", "C", (5, 4))
    e = _engine(monkeypatch, 5, 4, 100, 6, persist=persist)
    e.load_weights(sd, 0)
    _selfplay_vs_oracle(e, orc.Oracle(5, 4, 100), onet, 10, 950)
    assert (e.persistent() > 0) == (persist == "1")
    e.close()


@pytest.mark.parametrize("n,k,S,G,cut,tag", [(9, 5, 32, 4, 8, "seeded"), (15, 5, 16, 2, 4, "seeded"), (9, 5, 24, 3, 6, "resnet")])
def test_confident_cut_games_vs_oracle(monkeypatch, n, k, S, G, cut, tag):
    sd, onet, model, _ = _weights(n, tag, "C", (6, 5))
    e = _engine(monkeypatch, n, k, S, 3, model=model)
    e.load_weights(sd, 0)
    _selfplay_vs_oracle(e, orc.Oracle(n, k, S), onet, G, 4343, cut)
    e.close()


@pytest.mark.parametrize("feature", ["leaf_sym", "cache", "reuse", "vl8"])
def test_confident_search_upgrades_vs_oracle(monkeypatch, feature):
    n, k, S, G, cut = 9, 5, 40, 4, 8
    sd, onet, _, _ = _weights(n, "seeded", "C", (6, 5))
    e = _engine(monkeypatch, n, k, S, 4)
    e.load_weights(sd, 0)
    kw = {}
    if feature == "leaf_sym":
        e.set_leaf_symmetry(True); kw["leaf_sym"] = True
    elif feature == "cache":
        e.set_eval_cache(4096)          # the cache returns the stored evaluation: results equal the uncached oracle's
    elif feature == "reuse":
        e.set_subtree_reuse(True); kw["reuse"] = True
    else:
        e.set_virtual_loss(8); kw["virtual_loss"] = 8
    _selfplay_vs_oracle(e, orc.Oracle(n, k, S, **kw), onet, G, 5151, cut)
    e.close()


def test_confident_arena_vs_oracle(monkeypatch):
    n, k, S, G, seed0 = 5, 4, 40, 4, 4000
    cand, oc, _, _ = _weights(n, "ckpt_saved", "C", (5, 4))
    base, ob, _, _ = _weights(n, "ckpt_0802")
    e = _engine(monkeypatch, n, k, S, 4)
    e.load_weights(cand, 0); e.load_weights(base, 1)
    r = e.arena(G, seed0=seed0, temperature_table=orc.arena_T_table(n * n))
    e.close()
    o = orc.Oracle(n, k, S)
    for g in range(G):
        us = np.random.RandomState(seed0 + g).random_sample(n * n)
        ro = o.arena_game(oc, ob, g, us)
        assert int(r["nply"][g]) == ro["nply"] and int(r["results"][g]) == ro["result"]
        assert np.array_equal(r["actions"][g][:ro["nply"]], ro["actions"])


# ------------------------------------------------------------------ T_a: an exact rescaling changes no bit
SCALES = [-30, -12, 12, 30]


@pytest.mark.parametrize("n,tag", [(5, "ckpt_saved"), (15, "seeded"), (9, "resnet")])
def test_rescaled_net_eval_is_bit_identical(monkeypatch, n, tag):
    boards, players, lasts = _positions(n, 20, 77 + n)
    planes = _planes(n, boards, players, lasts)
    sd0, _, model, fwd0 = _weights(n, tag)
    nm.assert_sane(fwd0(planes))
    for split in SPLIT_MODES:
        monkeypatch.setenv("AZ_SPLIT_MAX", split)
        e = az.Engine(n, 5 if n > 5 else 4, 8, 24, model=model)
        e.load_weights(sd0, 0)
        base = e.net_eval(boards, players, lasts)
        e.set_trunk_mode("bf16x3")
        base_bf = e.net_eval(boards, players, lasts)
        for a in SCALES:
            sd, _, _, fwd = _weights(n, tag, "T", a)
            nm.assert_sane(fwd(planes))
            e.set_trunk_mode("f32")
            e.load_weights(sd, 0)
            got = e.net_eval(boards, players, lasts)
            for x, y in zip(got, base):
                assert np.array_equal(x, y), f"T_{a} ({'split' if split != '0' else 'fused'}) changed the float32 outputs"
            e.set_trunk_mode("bf16x3")
            got = e.net_eval(boards, players, lasts)
            for x, y in zip(got, base_bf):
                assert np.array_equal(x, y), f"T_{a} changed the bf16x3 outputs"
            e.load_weights(sd0, 0)
        e.close()


@pytest.mark.parametrize("n,k,S,G,cut,persist", [(5, 4, 60, 6, 0, "1"), (9, 5, 32, 3, 6, "0")])
def test_rescaled_episodes_are_identical(monkeypatch, n, k, S, G, cut, persist):
    tag = "ckpt_saved" if n == 5 else "seeded"
    monkeypatch.setenv("AZ_PERSIST", persist)
    runs = []
    for a in [0] + SCALES:
        sd = _weights(n, tag, "T", a)[0] if a else _weights(n, tag)[0]
        e = az.Engine(n, k, S, 4, log_table=orc.numpy_log_table(S))
        e.load_weights(sd, 0)
        e.selfplay(G, seed0=616, max_plies=cut)
        runs.append((e.records(), e.games()))
        assert (e.persistent() > 0) == (persist == "1")
        e.close()
    for a, (rec, games) in zip(SCALES, runs[1:]):
        for key in ("actions", "boards", "visits", "pis", "z"):
            assert np.array_equal(rec[key], runs[0][0][key]), f"T_{a}: {key} changed"
        assert all(np.array_equal(x, y) for x, y in zip(games, runs[0][1]))


# ------------------------------------------------------------------ emulated trunks against the float64 bound
@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("n,tag,kind,arg", [(5, "seeded", None, None), (15, "seeded", None, None), (5, "ckpt_saved", None, None),
                                            (5, "ckpt_saved", "C", (5, 4)), (9, "seeded", "C", (7, 6)),
                                            (5, "ckpt_saved", "T", -6), (9, "seeded", "T", 6), (9, "resnet", None, None)])
def test_emulated_trunk_within_float64_bound(n, tag, kind, arg, mode):
    boards, players, lasts = _positions(n, 24, 5 + n)
    planes = _planes(n, boards, players, lasts)
    sd, _, model, fwd = _weights(n, tag, kind, arg)
    ref = fwd(planes, mode)
    amax, wmax, _ = nm.assert_sane(ref)
    if mode == "f16x2":
        assert amax < nm.F16_MAX and wmax < nm.F16_MAX, "outside the f16x2 window"
    e = az.Engine(n, 5 if n > 5 else 4, 8, 24, model=model)
    e.load_weights(sd, 0)
    e.set_trunk_mode(mode)
    lg, P, v = e.net_eval(boards, players, lasts)
    e.close()
    for key, got in (("logits", lg), ("P", P), ("v", v)):
        r = nm.bound_ratio(got, ref[key], ref["E_" + key])
        print(f"error/bound {mode} {n} {tag} {kind}{arg or ''} {key}: {r:.3g}")
        assert r <= 1.0, f"{mode}: {key} outside the mode's float64 bound (ratio {r:.3g})"
