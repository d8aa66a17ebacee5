// az_philox.hip -- AZ_RNG_PHILOX: the tape kernel, its launcher for the engine, and the host entry points that run the same
// sampler (az_rng_dev.h) compiled for the host.  A translation unit of its own: the kernels of az_kernels.hip do not see it.
#include "az_rng_dev.h"
#include "../../include/az_engine.h"

// One wavefront per (game, ply) of games [0, G) x plies [m0, m1); lanes run over the legal ranks, 64 apart.  Fills
// noise[g * noise_stride + off(m) + j] (noise may be null: the move uniforms alone, az_arena) and u[g * nn + m].  A game whose
// done[g] is non-zero is skipped (done may be null).  Every rejection loop is per lane and bounded (azphilox::MAX_ATTEMPTS).
__global__ __launch_bounds__(256) void k_tape(uint64_t seed0, int G, int nn, int m0, int m1, double alpha, int kind,
                                              const int *__restrict__ done, double *__restrict__ noise, int64_t noise_stride,
                                              double *__restrict__ u)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int span = m1 - m0;
    if (w >= (int64_t)G * span) return;
    const int g = (int)(w / span), m = m0 + (int)(w % span);
    if (done && done[g]) return;
    const uint64_t seed = seed0 + (uint64_t)g;
    if (lane == 0) u[(int64_t)g * nn + m] = azphilox::move_uniform(seed, m);
    if (!noise) return;
    const int k = nn - m;
    double *row = noise + (int64_t)g * noise_stride + azphilox::tape_offset(nn, m);
    if (kind == azphilox::KIND_GUMBEL) {
        for (int j = lane; j < k; j += 64) row[j] = azphilox::gumbel(seed, m, j);
        return;
    }
    const azphilox::Gamma gm = azphilox::gamma_of(alpha);
    double v[4], part = 0.0;          // nn <= 225: at most four ranks a lane
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int j = lane + 64 * i;
        v[i] = 0.0;
        if (j < k) {
            v[i] = azphilox::gamma_draw(gm, seed, m, j);
            part = part + v[i];
        }
    }
    const double sum = wave_sum_butterfly_d(part);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int j = lane + 64 * i;
        if (j < k) row[j] = sum == 0.0 ? 1.0 / (double)k : v[i] / sum;
    }
}

// for the engine: plies [m0, m1) of games seed0 + [0, G) on `stream`; the caller owns the buffers (noise_stride >= off(m1))
hipError_t az_tape_launch(hipStream_t stream, uint64_t seed0, int G, int nn, int m0, int m1, double alpha, int kind, const int *done,
                          double *noise, int64_t noise_stride, double *u)
{
    const int64_t waves = (int64_t)G * (m1 - m0);
    if (waves <= 0) return hipSuccess;
    if (nn > 256 || m0 < 0 || m1 > nn || waves > ((int64_t)1 << 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tape, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, seed0, G, nn, m0, m1, alpha, kind, done, noise,
                       noise_stride, u);
    return hipGetLastError();
}

extern "C" void az_rng_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    azphilox::philox4x32_10(ctr, key, out);
}
extern "C" double az_rng_log(double x) { return azphilox::az_log(x); }
extern "C" double az_rng_exp(double x) { return az_exp(x); }

extern "C" int az_rng_philox_tape(uint64_t seed, int board_size, double alpha, int max_plies, int kind, double *noise, double *u)
{
    if (board_size < 1 || board_size > 15 || !u || (kind != AZ_TAPE_DIRICHLET && kind != AZ_TAPE_GUMBEL)) return AZ_ERR_INVALID;
    if (noise && kind == AZ_TAPE_DIRICHLET && !(alpha > 0.0 && alpha < __builtin_inf())) return AZ_ERR_INVALID;
    const int nn = board_size * board_size;
    azphilox::tape_host(seed, nn, noise ? alpha : 1.0, max_plies > 0 && max_plies < nn ? max_plies : nn, kind, noise, u);
    return AZ_OK;
}
