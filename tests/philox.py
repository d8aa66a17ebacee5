"""The AZ_RNG_PHILOX stream restated from its contract in include/az_engine.h: Philox4x32-10 on plain integers, the float64
arithmetic on Python floats (one IEEE operation per operator, like the library's translation units under -ffp-contract=off),
and log / exp through az_rng_log / az_rng_exp, the two functions the contract names (their fma chains have no Python
equivalent before math.fma).  Nothing here reads the library's sampler."""
import math

import numpy as np

from alphazero_piskvorky_amd import _capi

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MOVE, NORMAL, ACCEPT, BOOST, GUMBEL = range(5)
ATTEMPTS = 64


def philox4x32(counter, key):
    c0, c1, c2, c3 = (int(x) for x in counter)
    k0, k1 = (int(x) for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniforms(seed, attempt, rank, ply, purpose):
    seed &= 2 ** 64 - 1
    w = philox4x32((attempt, rank, ply, purpose), (seed & MASK, seed >> 32))
    return (float((w[0] >> 5) * 67108864 + (w[1] >> 6)) / 9007199254740992.0,
            float((w[2] >> 5) * 67108864 + (w[3] >> 6)) / 9007199254740992.0)


def log(x):
    return _capi.rng_log(x)


def gamma(alpha, seed, ply, rank):
    boost = alpha < 1.0
    a = alpha + 1.0 if boost else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    out = d
    for t in range(ATTEMPTS):
        ua, ub = uniforms(seed, t, rank, ply, NORMAL)
        x1, x2 = 2.0 * ua - 1.0, 2.0 * ub - 1.0
        r2 = x1 * x1 + x2 * x2
        if r2 >= 1.0 or r2 == 0.0:
            continue
        x = x1 * math.sqrt(-2.0 * log(r2) / r2)
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        U = uniforms(seed, t, rank, ply, ACCEPT)[0]
        xx = x * x
        if U < 1.0 - 0.0331 * xx * xx or log(U) < 0.5 * xx + d * (1.0 - v + log(v)):
            out = d * v
            break
    if boost:
        U = uniforms(seed, 0, rank, ply, BOOST)[0]
        out = out * _capi.rng_exp(log(U) / alpha)
    return out


def dirichlet_sum(g):
    p = [0.0] * 64
    for j, x in enumerate(g):
        p[j % 64] = p[j % 64] + x               # rank j, j + 64, ...: rising rank within a partial
    h = 32
    while h >= 1:
        for l in range(h):
            p[l] = p[l] + p[l + h]
        h //= 2
    return p[0]


def ply_draws(seed, nn, alpha, ply, kind):
    k = nn - ply
    if kind == "gumbel":
        out = []
        for j in range(k):
            inner = log(1.0 - uniforms(seed, 0, j, ply, GUMBEL)[0])
            out.append(-log(-inner))
        return out
    g = [gamma(alpha, seed, ply, j) for j in range(k)]
    s = dirichlet_sum(g)
    return [1.0 / float(k)] * k if s == 0.0 else [x / s for x in g]


def tape(seed, n, alpha=0.3, max_plies=0, kind="dirichlet"):
    """(noise, u) of one game in az_rng_selfplay_tape's layout"""
    nn = n * n
    plies = max_plies if 0 < max_plies < nn else nn
    noise, u = [], []
    for m in range(plies):
        noise.extend(ply_draws(seed, nn, alpha, m, kind))
        u.append(uniforms(seed, 0, 0, m, MOVE)[0])
    return np.array(noise, np.float64), np.array(u, np.float64)
