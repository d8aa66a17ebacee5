"""Constant nets: evaluators whose priors tie (no reference imports; shared by tests/golden/make_golden.py `ties`, the oracle's
CPU test and tests/test_ties_gpu.py).

Every tensor of a constant net is zero except policy_fc.bias (= `levels`) and value_fc2.bias (= `vbias`).  Zero convolutions and
zero FC weights make every activation exactly 0 on every trunk path, so for EVERY position the logits are exactly `levels` and the
value is exactly tanh(vbias): the search sees one prior table with a few discrete levels, many cells share a PUCT score, and the
order rule of mcts.py:70-74 (max returns the first maximal child in row-major legal order) decides the whole search.
"""
import numpy as np

PLAIN_SHAPES = [
    ("conv1.weight", (32, 4, 3, 3)), ("conv1.bias", (32,)),
    ("conv2.weight", (64, 32, 3, 3)), ("conv2.bias", (64,)),
    ("conv3.weight", (128, 64, 3, 3)), ("conv3.bias", (128,)),
    ("policy_conv.weight", (4, 128, 1, 1)), ("policy_conv.bias", (4,)),
    ("policy_fc.weight", None), ("policy_fc.bias", None),
    ("value_conv.weight", (2, 128, 1, 1)), ("value_conv.bias", (2,)),
    ("value_fc1.weight", None), ("value_fc1.bias", (64,)),
    ("value_fc2.weight", (1, 64)), ("value_fc2.bias", (1,)),
]

# fixture sizes: 9 / 49 / 64 / 81 / 169 / 225 cells, 1 / 1 / 1 / 2 / 3 / 4 cells per lane of a tree row (nn = 64 fills the wave
# exactly, 7x7 is the largest board of the persistent kernel)
TIE_SIZES = [(3, 3), (7, 4), (8, 5), (9, 5), (13, 5), (15, 5)]
VBIAS = (0.0, -0.5, 0.25)
MIRROR_PAIRS = (5, 12)          # cells j and j + 64 of these j carry the single highest level of the mirror pattern


def constant_state_dict(n, levels, vbias):
    """GomokuNet state dict (net.py:37-53 layout): logits == levels and value == tanh(vbias) for every position."""
    nn = n * n
    levels = np.asarray(levels, np.float32)
    assert levels.shape == (nn,)
    own = {"policy_fc.weight": (nn, 4 * nn), "policy_fc.bias": (nn,), "value_fc1.weight": (64, 2 * nn)}
    sd = {name: np.zeros(shp or own[name], np.float32) for name, shp in PLAIN_SHAPES}
    sd["policy_fc.bias"] = levels.copy()
    sd["value_fc2.bias"] = np.array([vbias], np.float32)
    return sd


def constant_resnet_tensors(n, levels, vbias):
    """The same for the ResidualBlock net: the 24 folded tensors of az_load_weights_resnet, all zero except the policy_fc bias
    (index 19) and the value_fc2 bias (index 23)."""
    nn = n * n
    levels = np.asarray(levels, np.float32)
    assert levels.shape == (nn,)
    shapes = [(64, 4, 3, 3), (64,)] + [(64, 64, 3, 3), (64,)] * 6 + [(2, 64), (2,), (1, 64), (1,),
                                                                      (nn, 2 * nn), (nn,), (64, nn), (64,), (64,), (1,)]
    t = [np.zeros(s, np.float32) for s in shapes]
    assert len(t) == 24
    t[19] = levels.copy()
    t[23] = np.array([vbias], np.float32)
    return t


def levels_of(pattern, n, seed=0):
    """The prior patterns: a few discrete logit levels (float32[n*n])."""
    nn = n * n
    j = np.arange(nn)
    if pattern == "uniform":
        lv = np.zeros(nn)
    elif pattern == "three":
        lv = np.random.RandomState(seed).randint(0, 3, nn) * 0.5
    elif pattern == "checker":
        lv = (j % 2) * 1.0
    elif pattern == "mirror":
        # cells j and j + 64 (one lane of a tree row) share a level, neighbours differ; the pairs of MIRROR_PAIRS alone hold the
        # highest level, so the deciding tie is between two cells of ONE lane
        assert nn > 64 + max(MIRROR_PAIRS)
        lv = ((j % 64) % 3) * 0.5
        for p in MIRROR_PAIRS:
            lv[p] = lv[p + 64] = 1.5
    else:
        raise ValueError(pattern)
    return lv.astype(np.float32)


def temperature(ply, noise):
    """self_play.py:24-26 with root noise, evaluator.py:14-19 without (as make_golden's tree fixtures)"""
    return float((np.exp(-ply / 100) + 0.01) / 1.01) if noise else float(0.3 * np.exp(-ply / 4))
