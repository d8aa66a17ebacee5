// az_ext.h -- the batched external evaluator (az_set_external_evaluator, and the one az_search_callback installs for its
// own call): the pending leaves of every game as one compact batch of encoded positions for an evaluator outside the
// engine, and its priors and values back into the rows the tree step reads.  Both kernels work over the net kernels' view of a lane
// (LaunchCtx.dv: B = evaluation items = slots x leaves per batch, s_status / s_net per item).  The lanes of an engine are served one launch after another on one stream, each
// appending to the same request, so a request lists its items in ascending (lane, slot, leaf-of-batch) order.
#pragma once
#include "az_tree.h"

constexpr int EXT_GATHER_THREADS = 1024;

// ------------------------------------------------------------------------------------------------
// k_ext_gather: ONE workgroup.  Selects the items that wait for net `net`, compacts them in item order (ballot / popcount
// prefix inside a wave, the waves' counts through LDS, 1024 items per round), writes map[j] = item_base + item for request
// entry j and the running count, then encodes the planes of its entries as games.py:86-129 does: plane 0 the side to move,
// 1 the opponent, 2 the last move one-hot, 3 zeros -- every float of every entry, as 16-byte stores (an entry is 4 n*n
// floats, so every entry starts 16-byte aligned when `planes` does), and nothing behind the last entry.
// first != 0 starts a request (entry 0); otherwise the launch appends behind the *count entries of the earlier lanes.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(EXT_GATHER_THREADS) void k_ext_gather(DevState dv, int net, int item_base, int first, int capacity,
                                                                  float *__restrict__ planes, int *map, int *count)
{
    typedef TreeGeo<N> G;
    constexpr int NWAVES = EXT_GATHER_THREADS / 64;
    __shared__ int wave_cnt[NWAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int base0 = first ? 0 : *count;
    __syncthreads();                                   // everyone has read the count before it is written below
    int base = base0;
    for (int c0 = 0; c0 < dv.B; c0 += EXT_GATHER_THREADS) {
        const int it = c0 + (int)threadIdx.x;
        const bool sel = it < dv.B && dv.s_status[it] == SLOT_ACTIVE && leaf_needs_net(dv.leaf_kind[it]) && dv.s_net[it] == net;
        const u64 m = __ballot(sel);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; w++) {
            const int c = wave_cnt[w];
            before += w < wv ? c : 0;
            total += c;
        }
        const int j = base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (sel && j < capacity) map[j] = item_base + it;
        base += total;
        __syncthreads();                               // wave_cnt is rewritten by the next round; the map entries are visible
    }
    if (base > capacity) base = capacity;              // never reached: the host checks capacity >= items at episode begin
    if (threadIdx.x == 0) *count = base;
    for (int j = base0 + wv; j < base; j += NWAVES) {  // one wavefront per entry
        const int it = map[j] - item_base;
        const u64 *lf = dv.leaf + (size_t)it * 8;       // mover-relative: words 0-3 the side to move, 4-7 the opponent
        const int last = dv.leaf_last[it];
        float4 *o = reinterpret_cast<float4 *>(planes + (size_t)j * 4 * G::nn);
        for (int q = lane; q < G::nn; q += 64) {        // float4 q holds floats 4q .. 4q + 3 of the entry
            float f[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int idx = 4 * q + c, p = idx / G::nn, cell = idx - p * G::nn;
                const bool stone = p < 2 && ((lf[4 * p + (cell >> 6)] >> (cell & 63)) & 1ull);
                f[c] = (stone || (p == 2 && cell == last)) ? 1.0f : 0.0f;
            }
            o[q] = make_float4(f[0], f[1], f[2], f[3]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_ext_scatter: one wavefront per request entry; entries of other lanes are skipped.  policy[j][0 .. n*n) becomes the
// logits row of the entry's item (row stride RW, the tail up to RW zeroed) and value[j]
// the first entry of its hidden row: where the tree step's ext_eval branch reads priors and value.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void k_ext_scatter(DevState dv, int item_base, int count, const int *__restrict__ map,
                                                     const float *__restrict__ policy, const float *__restrict__ value)
{
    typedef TreeGeo<N> G;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= count) return;
    const int it = map[j] - item_base;
    if (it < 0 || it >= dv.B) return;
    float *lg = dv.logits + (size_t)it * G::RW;
    const float *pj = policy + (size_t)j * G::nn;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        const int c = lane + 64 * i;
        lg[c] = c < G::nn ? pj[c] : 0.0f;
    }
    if (lane == 0) dv.vhid[(size_t)it * 64] = value[j];
}
