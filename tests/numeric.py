"""Float64 reference forwards of GomokuNet and the ResidualBlock net, with a propagated a-priori error bound.

A plain test helper (no fixtures, no reference imports).  The forwards are written from the layer definitions in
alphazero_piskvorky_amd/net.py, independently of the oracle's C code, and take the state-dict layout; the
ResidualBlock net takes the 24 folded tensors of fold_resnet_state_dict, which are what the engine and the oracle load.

Error bound
-----------
For a layer y = W x + b computed in floating point with a K-term dot product (any summation order, one rounding per
product-add) and the bias added once, the standard bound is

    |fl(y) - y| <= gamma_{K+1} (|W| |x| + |b|),        gamma_K = K u / (1 - K u),   u = 2^-24  (float32).

If the layer input itself carries an error E_{l-1}, the exact W x moves by at most |W| E_{l-1}.  ReLU and tanh are
1-Lipschitz, so they pass an error through unchanged.  Hence, per layer,

    E_l = |W_l| E_{l-1} + gamma_{K+1} (|W_l| |x_{l-1}| + |b_l|) + delta |W_l| |x_{l-1}| + eta (|W_l| 1 + 1_W |x_{l-1}|),

where |x_{l-1}| is the float64 activation, 1_W is the 0/1 pattern of W (the same window as |W|), and delta and eta are
the per-product terms of the emulated trunks (zero for the canonical float32 trunk).  A residual add contributes the
skip input's error plus one more rounding, covered by gamma_{K+2} with |skip| in the bracket.  The bound is scaled by
(1 + 2^-10) to absorb the float64 reference's own rounding.

Per-product terms, from the header of csrc/az_net_emul.h (convolutions only; the FC layers are float32 in every mode):
  bf16x3  x = hi + mid + lo + r with |x - hi| <= 2^-8 |x|, |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|, |r| <= 2^-24 |x|.
          The dropped products w_mid a_lo, w_lo a_mid (each <= 2^-24 |w a|), w_lo a_lo (2^-32) and the two residuals
          r_w a, w r_a (each <= 2^-24) sum to under 4 * 2^-24:  delta = 2^-22.  bfloat16 keeps float32's exponent
          range, so there is no absolute term:  eta = 0.
  f16x2   x = hi + lo / 2048 + r with |x - hi| <= 2^-11 |x| and |r| <= 2^-11 |x - hi| <= 2^-22 |x| while hi and lo are
          normal float16.  The dropped w_lo a_lo (<= 2^-22) plus the residuals r_w a, w r_a (each <= 2^-22) give
          delta = 2^-20.  Below |x| = 2^-14 hi is a float16 subnormal, and lo (stored as (x - hi) 2^11) reaches float16's
          subnormals once |x - hi| < 2^-25: the split then resolves x only to an absolute 2^-24 / 2^11 / 2 = 2^-36 per
          operand.  eta = 2^-35 covers both operands' share.  Above 65504 the split saturates: that is outside the bound
          and outside every window a test claims (see assert_sane and F16_MAX).

Softmax.  With the float32 logits z' = z + e, |e_j| <= E_j, and the float32 exp (relative error <= 3u measured as
about 2u), the shift by the max (rounding u |z_j - m|), the float32 sum (gamma_{nn}) and the divide (u):

    |P'_j - P_j| <= P_j expm1(D_j + max_i D_i + gamma_{nn} + u) + 2^-148,     D_j = E_j + u |z_j - m| + 3u,

where the absolute 2^-148 is the two half-quanta of a subnormal exp result and of the subnormal quotient.
Value:  |v' - v| <= E_y + 2^-21 (the canonical tanh is (1 - t) / (1 + t) with t = exp(-2|y|), a few u absolute).
"""
import numpy as np

U32 = 2.0 ** -24
MODES = {                       # mode -> (delta, eta) of the convolutions
    "f32": (0.0, 0.0),
    "bf16x3": (2.0 ** -22, 0.0),
    "f16x2": (2.0 ** -20, 2.0 ** -35),
}
F16_MAX = 65504.0


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def _conv(x, w, b=None):
    """x (B, C, n, n), w (O, C, k, k) with k in {1, 3}, zero padding 'same' -> (B, O, n, n); float64."""
    B, C, n, _ = x.shape
    k = w.shape[2]
    if k == 1:
        y = np.einsum("oc,bcp->bop", w[:, :, 0, 0], x.reshape(B, C, n * n)).reshape(B, -1, n, n)
    else:
        xp = np.zeros((B, C, n + 2, n + 2))
        xp[:, :, 1:-1, 1:-1] = x
        y = np.zeros((B, w.shape[0], n, n))
        for ky in range(3):
            for kx in range(3):
                y += np.einsum("oc,bcij->boij", w[:, :, ky, kx], xp[:, :, ky:ky + n, kx:kx + n])
    if b is not None:
        y += b.reshape(1, -1, 1, 1)
    return y


class _Fwd:
    """Runs layers in float64 and carries the error bound E of the float32 (or emulated) computation alongside."""

    def __init__(self, mode):
        self.delta, self.eta = MODES[mode]
        self.acts = []            # every layer input/output seen, for the range checks
        self.weights = []

    def conv(self, x, E, w, b, skip=None, skipE=None, relu=True):
        w = np.asarray(w, np.float64)
        b = np.zeros(w.shape[0]) if b is None else np.asarray(b, np.float64)
        self.acts.append(x); self.weights.append(w)
        K = w.shape[1] * w.shape[2] * w.shape[3]
        y = _conv(x, w, b)
        aw, ax = np.abs(w), np.abs(x)
        mag = _conv(ax, aw) + np.abs(b).reshape(1, -1, 1, 1)
        E = _conv(E, aw) + gamma(K + 2) * mag + self.delta * _conv(ax, aw)
        if self.eta:
            E = E + self.eta * (_conv(np.ones_like(x), aw) + _conv(ax, (w != 0).astype(np.float64)))
        if skip is not None:
            E = E + skipE + gamma(K + 2) * np.abs(skip)
            y = y + skip
        if relu:
            y = np.maximum(y, 0.0)
        self.acts.append(y)
        return y, E

    def fc(self, x, E, w, b, relu=False):
        w = np.asarray(w, np.float64); b = np.asarray(b, np.float64)
        self.acts.append(x); self.weights.append(w)
        K = w.shape[1]
        y = x @ w.T + b
        E = E @ np.abs(w).T + gamma(K + 1) * (np.abs(x) @ np.abs(w).T + np.abs(b))
        if relu:
            y = np.maximum(y, 0.0)
        self.acts.append(y)
        return y, E


def _heads(f, h, E, pw, pb, vw, vb, pfw, pfb, v1w, v1b, v2w, v2b):
    B = h.shape[0]
    p, pE = f.conv(h, E, pw, pb)
    v, vE = f.conv(h, E, vw, vb)
    logits, lE = f.fc(p.reshape(B, -1), pE.reshape(B, -1), pfw, pfb)
    hid, hE = f.fc(v.reshape(B, -1), vE.reshape(B, -1), v1w, v1b, relu=True)
    y, yE = f.fc(hid, hE, np.asarray(v2w).reshape(1, -1), np.asarray(v2b).reshape(1))
    return logits, lE, y[:, 0], yE[:, 0]


def _softmax_out(f, logits, lE, y, yE):
    z = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(z)
    P = e / e.sum(axis=1, keepdims=True)
    nn = logits.shape[1]
    D = lE + U32 * np.abs(z) + 3 * U32
    PE = np.minimum(P * np.expm1(np.minimum(D + D.max(axis=1, keepdims=True) + gamma(nn) + U32, 700.0)), 1.0) + 2.0 ** -148
    slack = 1.0 + 2.0 ** -10
    return dict(logits=logits, y=y, P=P, v=np.tanh(y), E_logits=lE * slack, E_y=yE * slack, E_P=PE * slack,
                E_v=yE * slack + 2.0 ** -21, acts=f.acts, weights=f.weights)


def gomoku_forward(sd, planes, mode="f32"):
    """GomokuNet (net.py) on planes (B, 4, n, n) -> dict(logits, y (value before tanh), P, v, E_* bounds, acts)."""
    x = np.asarray(planes, np.float64)
    if x.ndim == 3:
        x = x[None]
    f = _Fwd(mode)
    E = np.zeros_like(x)
    for i in (1, 2, 3):
        x, E = f.conv(x, E, sd[f"conv{i}.weight"], sd[f"conv{i}.bias"])
    out = _heads(f, x, E, sd["policy_conv.weight"], sd["policy_conv.bias"], sd["value_conv.weight"], sd["value_conv.bias"],
                 sd["policy_fc.weight"], sd["policy_fc.bias"], sd["value_fc1.weight"], sd["value_fc1.bias"],
                 sd["value_fc2.weight"], sd["value_fc2.bias"])
    return _softmax_out(f, *out)


def resnet_forward(folded, planes, mode="f32"):
    """ResidualBlock net on the 24 folded tensors of fold_resnet_state_dict (BatchNorm already in the convs)."""
    t = [np.asarray(a, np.float64) for a in folded]
    x = np.asarray(planes, np.float64)
    if x.ndim == 3:
        x = x[None]
    f = _Fwd(mode)
    E = np.zeros_like(x)
    x, E = f.conv(x, E, t[0], t[1])
    for r in range(3):
        w1, b1, w2, b2 = t[2 + 4 * r: 6 + 4 * r]
        h, hE = f.conv(x, E, w1, b1)
        x, E = f.conv(h, hE, w2, b2, skip=x, skipE=E)
    pw, pb, vw, vb = t[14], t[15], t[16], t[17]
    out = _heads(f, x, E, pw.reshape(pw.shape[0], -1, 1, 1), pb, vw.reshape(vw.shape[0], -1, 1, 1), vb, *t[18:24])
    return _softmax_out(f, *out)


# ------------------------------------------------------------------ exact weight transforms
GOMOKU_BIASES = ("conv1.bias", "conv2.bias", "conv3.bias", "policy_conv.bias", "value_conv.bias")


def scale_invariance(sd, a):
    """T_a on a GomokuNet state dict: conv1 weight and every conv bias times 2^a, policy_fc / value_fc1 weights times
    2^-a.  Every trunk activation scales by 2^a; logits, value and P do not change (exactly, while all stays normal)."""
    out = {k: np.array(v, np.float32, copy=True) for k, v in sd.items()}
    s = np.float32(2.0 ** a)
    out["conv1.weight"] = out["conv1.weight"] * s
    for k in GOMOKU_BIASES:
        out[k] = out[k] * s
    for k in ("policy_fc.weight", "value_fc1.weight"):
        out[k] = out[k] * np.float32(2.0 ** -a)
    return out


def resnet_scale_invariance(sd, a):
    """T_a on a ResidualBlock state dict (unfolded): the stem conv's weight, every conv bias, every BatchNorm's
    running_mean and bias times 2^a; policy_fc / value_fc1 weights times 2^-a.  Folding commutes with it exactly."""
    out = {k: np.array(v, np.float32, copy=True) for k, v in sd.items()}
    s = np.float32(2.0 ** a)
    for k in out:
        layer, what = k.rsplit(".", 1)
        if k == "conv.weight" or (what == "bias" and (layer.endswith("conv") or "bn" in layer)) or what == "running_mean":
            out[k] = out[k] * s
    for k in ("policy_fc.weight", "value_fc1.weight"):
        out[k] = out[k] * np.float32(2.0 ** -a)
    return out


def confidence(sd, p, v):
    """C_{p,v}: policy_fc (weight and bias) times 2^p, value_fc2 (weight and bias) times 2^v.  Logits scale by 2^p (zero
    and subnormal priors), the value's argument by 2^v (tanh saturates to exactly +-1)."""
    out = {k: np.array(w, np.float32, copy=True) for k, w in sd.items()}
    for k in ("policy_fc.weight", "policy_fc.bias"):
        out[k] = out[k] * np.float32(2.0 ** p)
    for k in ("value_fc2.weight", "value_fc2.bias"):
        out[k] = out[k] * np.float32(2.0 ** v)
    return out


# ------------------------------------------------------------------ range checks (run before anything goes to a GPU)
def _nz_min(a):
    a = np.abs(a[np.isfinite(a) & (a != 0)])
    return float(a.min()) if a.size else np.inf


def ranges(ref):
    """(max |activation|, max |weight|, smallest nonzero |w| * |x| over the layers) of a forward's result."""
    amax = max(float(np.abs(a).max()) for a in ref["acts"])
    wmax = max(float(np.abs(w).max()) for w in ref["weights"])
    prod = min(_nz_min(w) * _nz_min(x) for w, x in zip(ref["weights"], ref["acts"][0::2]))
    return amax, wmax, prod


def assert_sane(ref, amax_below=2.0 ** 100, prod_above=2.0 ** -78):
    """Before any launch: everything finite, activations below amax_below, and every product of a nonzero weight and
    a nonzero layer input at least prod_above.  With prod_above = 2^-78 every partial sum of a dot product is a multiple
    of at least 2^-125, so it is 0 or a normal float32: power-of-two rescalings (T_a) are then exact."""
    for key in ("logits", "y", "P", "v"):
        assert np.all(np.isfinite(ref[key])), key
    for a in ref["acts"] + ref["weights"]:
        assert np.all(np.isfinite(a))
    amax, wmax, prod = ranges(ref)
    assert amax < amax_below, f"activation {amax:g} not below {amax_below:g}"
    assert prod >= prod_above, f"smallest product {prod:g} below {prod_above:g}"
    return amax, wmax, prod


def p_bar(P_ref, p):
    """Bar for priors against torch's under C_{p,v}: the build's torch bar for logits (2e-5) scaled by 2^p moves a prior
    by at most expm1(2 * 2^p * 2e-5) relative; plus the usual 1e-6 absolute."""
    return 1e-6 + np.asarray(P_ref, np.float64) * np.expm1(2 * 2.0 ** p * 2e-5)


def bound_ratio(got, ref_value, bound):
    """max |got - ref| / bound (must be <= 1)."""
    d = np.abs(np.asarray(got, np.float64) - ref_value)
    return float(np.max(d / bound))
