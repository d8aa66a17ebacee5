// az_rng_dev.h -- the counter-based RNG stream of AZ_RNG_PHILOX (include/az_engine.h states the contract): Philox4x32-10, the
// software float64 log, and the samplers of one tape entry.  Everything is __host__ __device__ and one sequence of integer
// operations and separately rounded float64 + - * / sqrt and explicit fma, so az_rng_philox_tape (host) and k_tape (device)
// give the same bits as long as the translation unit keeps -ffp-contract=off.  No libm, no device library log / exp / pow.
#pragma once
#include "az_device.h"

namespace azphilox {

enum { PURPOSE_MOVE = 0, PURPOSE_NORMAL = 1, PURPOSE_ACCEPT = 2, PURPOSE_BOOST = 3, PURPOSE_GUMBEL = 4 };
enum { KIND_DIRICHLET = 0, KIND_GUMBEL = 1 };
constexpr int MAX_ATTEMPTS = 64;         // AZ_RNG_PHILOX_ATTEMPTS: attempts of one gamma draw; then the draw is d, the sampler's value at x = 0

__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// two 53-bit uniforms in [0, 1) from the four words of one call: (w0 >> 5) * 2^26 + (w1 >> 6) over 2^53, and the same of
// w2, w3 (every step exact in float64)
__host__ __device__ __forceinline__ void uniforms2(uint64_t seed, uint32_t attempt, uint32_t rank, uint32_t ply, uint32_t purpose,
                                                   double &a, double &b)
{
    const uint32_t ctr[4] = {attempt, rank, ply, purpose}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    a = ((double)(w[0] >> 5) * 67108864.0 + (double)(w[1] >> 6)) / 9007199254740992.0;
    b = ((double)(w[2] >> 5) * 67108864.0 + (double)(w[3] >> 6)) / 9007199254740992.0;
}

// Natural logarithm in software.  x = m * 2^k with m in [sqrt(1/2), sqrt(2)); f = m - 1, s = f / (2 + f), z = s * s;
// log(m) = f - (f * f / 2 - s * (f * f / 2 + R(z))) with R the degree-7 polynomial of the classic fdlibm log (Sun, 1993) in
// one fma Horner chain; the result adds k * ln2 in the two parts az_exp uses.  +-0 gives -inf, a negative argument NaN, +inf
// and NaN themselves; subnormals are scaled by 2^54 first.
__host__ __device__ __forceinline__ double az_log(double x)
{
    u64 bits;
    __builtin_memcpy(&bits, &x, sizeof bits);
    if ((bits << 1) == 0) return -__builtin_inf();
    if (bits >> 63) return __builtin_nan("");
    if ((bits >> 52) == 0x7FF) return x;
    long long k = 0;
    if ((bits >> 52) == 0) {
        x = x * 18014398509481984.0;       // 2^54, exact
        __builtin_memcpy(&bits, &x, sizeof bits);
        k = -54;
    }
    k += (long long)(bits >> 52) - 1023;
    u64 mant = bits & 0x000FFFFFFFFFFFFFull;
    u64 mbits = mant | 0x3FF0000000000000ull;                      // m in [1, 2)
    if (mant > 0x6A09E667F3BCCull) { mbits = mant | 0x3FE0000000000000ull; k += 1; }      // above sqrt(2): halve
    double m;
    __builtin_memcpy(&m, &mbits, sizeof m);
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double R = 1.479819860511658591e-01;
    R = __builtin_fma(R, z, 1.531383769920937332e-01);
    R = __builtin_fma(R, z, 1.818357216161805012e-01);
    R = __builtin_fma(R, z, 2.222219843214978396e-01);
    R = __builtin_fma(R, z, 2.857142874366239149e-01);
    R = __builtin_fma(R, z, 3.999999999940941908e-01);
    R = __builtin_fma(R, z, 6.666666666666735130e-01);
    R = R * z;
    const double hfsq = 0.5 * f * f;
    const double dk = (double)k;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

// the move uniform of ply m
__host__ __device__ __forceinline__ double move_uniform(uint64_t seed, int ply)
{
    double a, b;
    uniforms2(seed, 0, 0, (uint32_t)ply, PURPOSE_MOVE, a, b);
    return a;
}

// Gumbel(0, 1) of (ply, rank): -log(-log(1 - U))
__host__ __device__ __forceinline__ double gumbel(uint64_t seed, int ply, int rank)
{
    double a, b;
    uniforms2(seed, 0, (uint32_t)rank, (uint32_t)ply, PURPOSE_GUMBEL, a, b);
    return -az_log(-az_log(1.0 - a));
}

// Gamma(alpha, 1) of (ply, rank) by Marsaglia and Tsang (2000) with shape a = alpha (alpha >= 1) or alpha + 1 (below 1):
// d = a - 1/3, c = 1 / sqrt(9 d).  Attempt t = 0, 1, ...: the normal pair's two uniforms give x1 = 2 U1 - 1, x2 = 2 U2 - 1,
// r2 = x1 x1 + x2 x2; r2 >= 1 or r2 == 0 fails the attempt; x = x1 * sqrt(-2 log(r2) / r2) (the polar method's second normal is
// not used); v = 1 + c x, v <= 0 fails the attempt; v = v v v; U is the attempt's acceptance uniform; accepted when
// U < 1 - 0.0331 (x x) (x x) or log(U) < 0.5 x x + d (1 - v + log(v)).  The draw is d v; after MAX_ATTEMPTS failed attempts it
// is d.  Below 1 the draw is multiplied by exp(log(U) / alpha), U the boost uniform.
struct Gamma {
    double alpha, d, c;
    bool boost;
};
__host__ __device__ __forceinline__ Gamma gamma_of(double alpha)
{
    Gamma g;
    g.alpha = alpha;
    g.boost = alpha < 1.0;
    const double a = g.boost ? alpha + 1.0 : alpha;
    g.d = a - 1.0 / 3.0;
    g.c = 1.0 / __builtin_sqrt(9.0 * g.d);
    return g;
}
__host__ __device__ inline double gamma_draw(const Gamma &g, uint64_t seed, int ply, int rank)
{
    double out = g.d;
    for (int t = 0; t < MAX_ATTEMPTS; t++) {
        double u1, u2;
        uniforms2(seed, (uint32_t)t, (uint32_t)rank, (uint32_t)ply, PURPOSE_NORMAL, u1, u2);
        const double x1 = 2.0 * u1 - 1.0, x2 = 2.0 * u2 - 1.0;
        const double r2 = x1 * x1 + x2 * x2;
        if (r2 >= 1.0 || r2 == 0.0) continue;
        const double x = x1 * __builtin_sqrt(-2.0 * az_log(r2) / r2);
        double v = 1.0 + g.c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        double U, unused;
        uniforms2(seed, (uint32_t)t, (uint32_t)rank, (uint32_t)ply, PURPOSE_ACCEPT, U, unused);
        const double xx = x * x;
        if (U < 1.0 - 0.0331 * xx * xx || az_log(U) < 0.5 * xx + g.d * (1.0 - v + az_log(v))) {
            out = g.d * v;
            break;
        }
    }
    if (g.boost) {
        double U, unused;
        uniforms2(seed, 0, (uint32_t)rank, (uint32_t)ply, PURPOSE_BOOST, U, unused);
        out = out * az_exp(az_log(U) / g.alpha);
    }
    return out;
}

// doubles before ply m in one game's noise tape: sum_{i < m} (nn - i)
__host__ __device__ __forceinline__ int64_t tape_offset(int nn, int m) { return (int64_t)m * nn - (int64_t)m * (m - 1) / 2; }

// the Dirichlet sum of a ply's k gammas in its one order: 64 partial sums, partial l = 0.0 + g[l] + g[l + 64] + ... with rising
// rank, folded by halves (p[l] = p[l] + p[l + h] for l < h; h = 32, 16, 8, 4, 2, 1) -- what the 64-lane butterfly of the kernel
// leaves in every lane
inline double dirichlet_sum_host(const double *g, int k)
{
    double p[64];
    for (int l = 0; l < 64; l++) {
        p[l] = 0.0;
        for (int j = l; j < k; j += 64) p[l] = p[l] + g[j];
    }
    for (int h = 32; h >= 1; h >>= 1)
        for (int l = 0; l < h; l++) p[l] = p[l] + p[l + h];
    return p[0];
}

// one game's tape on the host, in az_rng_selfplay_tape's layout
inline void tape_host(uint64_t seed, int nn, double alpha, int plies, int kind, double *noise, double *u)
{
    const Gamma gm = gamma_of(alpha);
    for (int m = 0; m < plies; m++) {
        const int k = nn - m;
        if (noise) {
            double *row = noise + tape_offset(nn, m);
            if (kind == KIND_GUMBEL) {
                for (int j = 0; j < k; j++) row[j] = gumbel(seed, m, j);
            } else {
                for (int j = 0; j < k; j++) row[j] = gamma_draw(gm, seed, m, j);
                const double sum = dirichlet_sum_host(row, k);
                for (int j = 0; j < k; j++) row[j] = sum == 0.0 ? 1.0 / (double)k : row[j] / sum;
            }
        }
        u[m] = move_uniform(seed, m);
    }
}

} // namespace azphilox
