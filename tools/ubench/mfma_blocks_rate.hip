// Microbenchmark: issue rate of v_mfma_f32_4x4x1_16b_f32 (16 independent 4x4 outer products, K = 1) in cycles per MFMA per SIMD:
// (a) independent accumulators, one wave per SIMD; (b) ONE dependent accumulator chain per wave, at one and at two waves per SIMD
// (the shape of the fused trunk's head convs on 4-row blocks).
// hipcc --offload-arch=gfx950 -O3 -o mfma_blocks_rate mfma_blocks_rate.hip && ./mfma_blocks_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <algorithm>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

// NACC accumulators, each its own chain; NACC = 1 is the single dependent chain.  The operands change every instruction (four
// registers of each, as one ds_read_b128 / one 16-byte weight load would deliver them).
template <int NACC>
__global__ __launch_bounds__(512) void kblk(float *out, unsigned long long *cyc, unsigned long long *rtc, int iters)
{
    f32x4 acc[NACC];
    for (int i = 0; i < NACC; i++) acc[i] = f32x4{0, 0, 0, 0};
    float a[4], b[4];
    for (int e = 0; e < 4; e++) {
        a[e] = ((threadIdx.x * 13 + e * 29) % 97) * 1.37e-3f - 0.06f;
        b[e] = ((threadIdx.x * 31 + e * 17) % 89) * 2.1e-3f - 0.09f;
    }
    unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int i = 0; i < NACC; i++) acc[i] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[e], b[(e + i) & 3], acc[i], 0, 0, 0);
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0;
    for (int i = 0; i < NACC; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) { cyc[blockIdx.x] = t1 - t0; rtc[blockIdx.x] = r1 - r0; }
}

template <class K>
void run(const char *name, K kern, int nacc, int threads)
{
    // >= 2 s of back-to-back launches before the reading, then the mean cycles and the median clock over workgroups
    const int iters = 20000, blocks = 256;
    float *out; unsigned long long *cyc, *rtc;
    hipMalloc(&out, blocks * threads * 4); hipMalloc(&cyc, blocks * 8); hipMalloc(&rtc, blocks * 8);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float ms = 0, total = 0;
    while (total < 2000.0f) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, 0, out, cyc, rtc, iters);
        hipEventRecord(e1);
        if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); exit(1); }
        hipEventElapsedTime(&ms, e0, e1);
        total += ms;
    }
    std::vector<unsigned long long> h(blocks), hr(blocks);
    hipMemcpy(h.data(), cyc, blocks * 8, hipMemcpyDeviceToHost);
    hipMemcpy(hr.data(), rtc, blocks * 8, hipMemcpyDeviceToHost);
    std::vector<double> ghz(blocks);
    double mean = 0;
    for (int i = 0; i < blocks; i++) { ghz[i] = (double)h[i] / (double)hr[i] * 0.1; mean += h[i]; }
    mean /= blocks;
    std::sort(ghz.begin(), ghz.end());
    const double mfma_per_simd = (double)iters * 4 * nacc * (threads / 64) / 4.0;
    printf("%-44s waves/SIMD %d  cycles/MFMA/SIMD %6.2f   in-kernel clock %.3f GHz (median; %.3f .. %.3f)\n", name, threads / 256,
           mean / mfma_per_simd, ghz[blocks / 2], ghz[0], ghz[blocks - 1]);
    hipFree(out); hipFree(cyc); hipFree(rtc);
}

int main()
{
    run("(a) 4x4x1, 8 independent accumulators", kblk<8>, 8, 256);
    run("(a) 4x4x1, 4 independent accumulators", kblk<4>, 4, 256);
    run("(b) 4x4x1, ONE dependent chain per wave", kblk<1>, 1, 256);
    run("(b) 4x4x1, ONE dependent chain per wave", kblk<1>, 1, 512);
    return 0;
}
