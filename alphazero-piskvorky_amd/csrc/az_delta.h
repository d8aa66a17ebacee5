// az_delta.h -- delta evaluation of the plain float32 trunk at n = 15.
//
// Within one ply a game's root position does not change across its S + 1 evaluations, and a leaf is the root plus `depth`
// stones.  Seen from the leaf's side to move, the net's input differs from one of two per-ply BASE inputs -- the root's stones
// in the root mover's perspective (parity 0) or in the opponent's (parity 1), last-move plane empty -- in `depth` cells.  Three
// 3x3 convs give a changed cell a 3x3 / 5x5 / 7x7 footprint in the outputs of conv1 / conv2 / conv3 (and the 1x1 heads); every
// other output element is the same k-ordered fma chain over the same inputs as in the base evaluation, so it has the same bits.
//
//   k_trunk_base   once per ply, grid (slots, 2): the full trunk arithmetic (trunk_group's, ring tiling) on a base input; keeps
//                  the packed conv1 / conv2 images exactly as they lie in LDS (padding ring included) and the head feature
//                  row in HBM: DeltaGeo::STRIDE floats per (slot, parity)
//   k_trunk_delta  in k_trunk's place, one workgroup per board: changed cells = leaf XOR base, dilated by 1 / 2 / 3 cells into
//                  three lists of 16-cell tiles; the windows of the base images those tiles read are copied into LDS, the
//                  layers run on the listed tiles only (conv_layer's subset mode, no border-tap skipping), and the feature
//                  row is the base row with the conv3-region cells replaced.  A board with too many changed cells or conv3
//                  tiles is evaluated in full by the same workgroup with the same code: its lists are the whole board
//                  (delta_lists_full: 15 tiles per layer), its images start as zeros and nothing is read from the base.
//                  One trunk launch per batch (5h): the separate launch of trunk_group for those boards cost every batch a
//                  whole-CU slot per board only to read a flag.
// Which tile and lane computes an element does not enter (az_net.h, BorderSkip): results are bit-identical to k_trunk's.
#pragma once
#include "az_net.h"

constexpr int DELTA_MAX_CHANGED = 8;          // more changed cells than this: the board is evaluated in full
constexpr int DELTA_TILES_DEFAULT = 12;       // ... and so is one with more conv3 tiles than this (az_delta_max_tiles)
// per-slot counters: delta evaluations, full evaluations, conv3 tiles of the delta ones, base evaluations, then the delta
// evaluations by conv3 tile count 0 .. 15
constexpr int DELTA_CNT = 4 + 16;

template <int N>
struct DeltaGeo : NetGeo<N> {                 // NetGeo's images and waves; no BORDER_SKIP member: every tap is computed
    typedef NetGeo<N> B;
    static constexpr int IMG = 96 * B::CS;                    // floats of the two packed images: conv1 out (32 ch), conv2 out (64 ch)
    static constexpr int STRIDE = IMG + B::FROW;              // floats per (slot, parity) in HBM: the images, then the feature row
    static constexpr int MAXM = ((B::nn + 15) / 16) * 16;     // lanes of the longest tile list (a region is at most the board)
    static constexpr int C3 = 4;                              // conv3 tiles per chunk: their cell-major image overlays conv1's output
};

// Chebyshev distance of padded-image position (pr, pc) to the nearest changed board cell, 255 with none.
__host__ __device__ inline int delta_dist(int n, int pr, int pc, const unsigned char *changed, int nch)
{
    int best = 255;
    for (int i = 0; i < nch; i++) {
        const int cr = changed[i] / n, cc = changed[i] - cr * n;
        const int dr = pr - 1 - cr < 0 ? cr - (pr - 1) : pr - 1 - cr, dc = pc - 1 - cc < 0 ? cc - (pc - 1) : pc - 1 - cc;
        const int dd = dr > dc ? dr : dc;
        best = dd < best ? dd : best;
    }
    return best;
}
// The five position lists of a delta evaluation, each in ascending padded position:
//   list 0 / 1 / 2  board cells within 1 / 2 / 3 of a changed cell: the cells conv1 / conv2 / conv3 + heads compute
//   list 3 / 4      padded positions (ring included) within 3 / 4: the windows of the base conv1 / conv2 images the layers read
__host__ __device__ inline bool delta_member(int n, int list, int pr, int pc, int dist)
{
    const bool inb = pr >= 1 && pr <= n && pc >= 1 && pc <= n;
    return list < 3 ? (inb && dist <= list + 1) : dist <= list;
}
// Tile lists as conv_layer addresses them: lane m of a list computes the cell at padded position wpos[m]; the lanes behind the
// last cell, up to a whole tile, repeat the last cell's position (inside the copied windows at every tap) and are marked junk.
template <int N>
struct DeltaLists {
    typedef DeltaGeo<N> G;
    unsigned short wpos[3][G::MAXM], cell[3][G::MAXM];
    unsigned short halo[2][G::PP];
    int cnt[5];                                // cells / positions per list
    __host__ __device__ int tiles(int l) const { return (cnt[l] + 15) >> 4; }
    __host__ __device__ void put(int list, int at, int pr, int pc)
    {
        const unsigned short pos = (unsigned short)(pr * G::PW + pc);
        if (list < 3) { wpos[list][at] = pos; cell[list][at] = (unsigned short)((pr - 1) * N + (pc - 1)); }
        else halo[list - 3][at] = pos;
    }
    __host__ __device__ void junk(int list, int i)      // i-th lane behind the last cell of the list
    {
        const int c = cnt[list], at = c + i;
        if (c > 0 && at < tiles(list) * 16) { wpos[list][at] = wpos[list][c - 1]; cell[list][at] = 0xFFFF; }
    }
};
// The lists of a set of changed cells, one position after the other: what k_trunk_delta builds with one thread per position
// (same members, same order), here so that the integer logic can be checked on the CPU.
template <int N>
__host__ __device__ inline void delta_lists_serial(const unsigned char *changed, int nch, DeltaLists<N> &L)
{
    typedef DeltaGeo<N> G;
    for (int l = 0; l < 5; l++) L.cnt[l] = 0;
    for (int p = 0; p < G::PP; p++) {
        const int pr = p / G::PW, pc = p - pr * G::PW;
        const int dist = delta_dist(N, pr, pc, changed, nch);
        for (int l = 0; l < 5; l++)
            if (delta_member(N, l, pr, pc, dist)) L.put(l, L.cnt[l]++, pr, pc);
    }
    for (int l = 0; l < 3; l++)
        for (int i = 0; i < 16; i++) L.junk(l, i);
}
// The lists of a board evaluated in full (more changed cells than DELTA_MAX_CHANGED, or more conv3 tiles than the threshold):
// every layer computes all N x N cells in ascending position -- a cell's place in lists 0 - 2 is its cell index --, and no
// window is read: the images start as zeros, ring included, and every cell the layers read has been computed.
template <int N>
__host__ __device__ inline void delta_full_put(DeltaLists<N> &L, int pr, int pc)        // one padded position's part
{
    if (pr < 1 || pr > N || pc < 1 || pc > N) return;
    for (int l = 0; l < 3; l++) L.put(l, (pr - 1) * N + (pc - 1), pr, pc);
}
template <int N>
__host__ __device__ inline void delta_full_cnt(DeltaLists<N> &L, int l) { L.cnt[l] = l < 3 ? N * N : 0; }
template <int N>
__host__ __device__ inline void delta_lists_full(DeltaLists<N> &L)
{
    typedef DeltaGeo<N> G;
    for (int p = 0; p < G::PP; p++) delta_full_put<N>(L, p / G::PW, p % G::PW);
    for (int l = 0; l < 5; l++) delta_full_cnt<N>(L, l);
    for (int l = 0; l < 3; l++)
        for (int i = 0; i < 16; i++) L.junk(l, i);
}

#ifdef __HIPCC__
// diagnostic builds only (-DAZ_STAMPS): k_trunk_delta's phase stamps (s_memtime), 16 u64 per workgroup in k_trunk's rows of the
// debug buffer.  0 entry, 1 lists done, 2 windows in LDS, 3 conv1, 4 conv2, 5 + 2 i / 6 + 2 i conv3 chunk i / its heads pass
// (zero where the leaf has no such chunk), 13 the conv3 tile count, 14 / 15 s_memrealtime at entry / at the last heads pass
#ifdef AZ_STAMPS
#define AZ_DSTAMP(k) do { if (threadIdx.x == 0 && dbg) dbg[(size_t)blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define AZ_DSTAMP_VAL(k, v) do { if (threadIdx.x == 0 && dbg) dbg[(size_t)blockIdx.x * 16 + (k)] = (unsigned long long)(v); } while (0)
#else
#define AZ_DSTAMP(k) do { } while (0)
#define AZ_DSTAMP_VAL(k, v) do { } while (0)
#endif

// policy_conv / value_conv of one chunk of conv3 tiles (trunk_heads' arithmetic: one k-ordered chain on v_mfma_f32_4x4x1): wave w
// takes chunk cells 32 w .. 32 w + 31 of the cell-major image out3; frow = the board's feature row
template <class G>
__device__ __forceinline__ void delta_heads(const NetWeights &w, float *__restrict__ frow, const float *out3, const float *hdq_lds,
                                            const unsigned short *cellof, int ncell, int wave, int lane)
{
    if (wave * 32 >= ncell) return;
    const int half = (lane >> 2) & 1;
    const int m = wave * 32 + (lane >> 3) * 4 + (lane & 3);
    float hb[4];
#pragma unroll
    for (int i = 0; i < 4; i++) hb[i] = (half * 4 + i) < 6 ? w.hdb[half * 4 + i] : 0.0f;
    const float4 *ap = reinterpret_cast<const float4 *>(hdq_lds) + (lane & 7);
    const float4 *bp = reinterpret_cast<const float4 *>(out3 + (m < ncell ? m : 0) * OUT3_CM_STRIDE);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k4 = 0; k4 < 32; k4++) {
        const float4 a = ap[k4 * 8], b = bp[k4];
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.w, b.w, acc, 0, 0, 0);
    }
    if (m < ncell) {
        const int cell = cellof[m];
        if (cell != 0xFFFF) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int j = half * 4 + i;
                if (j < 6) {
                    float v = acc[i] + hb[i];
                    frow[j * G::nn + cell] = v > 0.0f ? v : 0.0f;
                }
            }
        }
    }
}

// f(0), f(1), ... f(E - 1) with the round as a compile-time value: the fragment arrays below are indexed by constants only
template <int K, int E, class F>
__device__ __forceinline__ void delta_rounds(F &&f)
{
    if constexpr (K < E) { f(std::integral_constant<int, K>{}); delta_rounds<K + 1, E>(f); }
}

// Base evaluation: blockIdx.x = slot, blockIdx.y = parity.  trunk_group's phases on the root's stones; the two packed images
// leave for HBM between conv2 and conv3, the feature row after the heads.
// cnt: the per-slot counters [B][DELTA_CNT]
template <int N>
__global__ __launch_bounds__(NetGeo<N>::NW * 64) void k_trunk_base(DevState d, NetWeights w, int net_id, float *__restrict__ base,
                                                                    unsigned long long *cnt)
{
    typedef FusedGeo<N> G;
    typedef DeltaGeo<N> DG;
    static_assert(G::G == 1, "one board per workgroup");
    __shared__ __attribute__((aligned(16))) float lds[G::LDSF];
    __shared__ __attribute__((aligned(16))) float hdq_lds[1024];
    __shared__ unsigned short wpos[G::MR];
    __shared__ unsigned short cellof[G::MR];
    const int b = blockIdx.x, par = blockIdx.y;
    if (d.s_status[b] != SLOT_ACTIVE || d.s_net[b] != net_id) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float2 hq = reinterpret_cast<const float2 *>(w.hdq)[tid];
    bool e_me = false, e_op = false;
    int e_pos = G::PW + 1;
    if (tid < G::nn) {
        const int r = tid / N, c = tid - r * N;
        e_pos = (r + 1) * G::PW + (c + 1);
        const u64 *bd = d.board + (size_t)b * 8;
        const bool x = (bd[tid >> 6] >> (tid & 63)) & 1ull, o = (bd[4 + (tid >> 6)] >> (tid & 63)) & 1ull;
        const bool me_is_x = (d.s_player[b] == 1) != (par == 1);       // parity 0: the root's mover is "me"
        e_me = me_is_x ? x : o;
        e_op = me_is_x ? o : x;
    }
    reinterpret_cast<float2 *>(hdq_lds)[tid] = hq;
    if (tid < G::MR) {
        if constexpr (BorderSkip<G>::value) { wpos[tid] = G::map.pos[tid]; cellof[tid] = G::map.cell[tid]; }
        else {
            const int t = tid >> 4, c = tid & 15;
            wpos[tid] = (unsigned short)((t + 1) * G::PW + (c + 1));
            cellof[tid] = (unsigned short)(c < N ? t * N + c : 0xFFFF);
        }
    }
    {
        float4 *z = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < (96 * G::CS) / 4; i += G::NW * 64) z[i] = float4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    float *inA = lds, *inB = lds + 32 * G::CS;
    if (e_me) inB[e_pos] = 1.0f;
    if (e_op) inB[G::CS + e_pos] = 1.0f;
    __syncthreads();
    conv_layer<G, 4, 32, CONV_OUT_PACKED>(inB, inA, w.c1, w.c1b, wpos, cellof, wave, lane);
    __syncthreads();
    for (int i = tid; i < 3 * G::CS; i += G::NW * 64) inB[i] = 0.0f;
    __syncthreads();
    conv_layer<G, 32, 64, CONV_OUT_PACKED>(inA, inB, w.c2, w.c2b, wpos, cellof, wave, lane);
    __syncthreads();
    float *row = base + ((size_t)b * 2 + par) * DG::STRIDE;
    {
        const float4 *s = reinterpret_cast<const float4 *>(lds);
        float4 *g = reinterpret_cast<float4 *>(row);
        for (int i = tid; i < DG::IMG / 4; i += G::NW * 64) g[i] = s[i];
    }
    conv_layer<G, 64, 128, CONV_OUT3_CM>(inB, lds, w.c3, w.c3b, wpos, cellof, wave, lane);
    __syncthreads();
    // trunk_heads stores to feat[b * FROW + ...]: hand it the row's address less that offset
    trunk_heads<G>(d, w, net_id, row + DG::IMG - (size_t)b * G::FROW, lds, hdq_lds, cellof, b, wave, lane);
    if (tid == 0 && par == 0) cnt[(size_t)b * DELTA_CNT + 3] += 2ull;
}

// done[b]: 0 = evaluated in full, 1 + conv3 tiles = evaluated as a delta (or nothing to evaluate)
template <int N>
__global__ __launch_bounds__(NetGeo<N>::NW * 64) void k_trunk_delta(DevState d, NetWeights w, int net_id, float *__restrict__ feat,
                                                                     const float *__restrict__ base, unsigned char *done,
                                                                     unsigned long long *cnt, int max_tiles, unsigned long long *dbg)
{
    typedef DeltaGeo<N> G;
    constexpr int NT = G::NW * 64;
    static_assert(G::G == 1 && NT >= G::PP && NT == 512, "one board per workgroup, one thread per padded position");
    static_assert(G::C3 * 16 * OUT3_CM_STRIDE <= 32 * G::CS, "a chunk's conv3 image fits the dead conv1 image");
    static_assert(G::STRIDE % 4 == 0, "16-byte rows");
    __shared__ __attribute__((aligned(16))) float lds[G::IMG];          // conv1 image, conv2 image; a conv3 chunk overlays the first
    __shared__ __attribute__((aligned(16))) float planes[4 * G::CS];    // me, opponent, last move, zeros
    __shared__ __attribute__((aligned(16))) float hdq_lds[1024];
    __shared__ DeltaLists<N> L;
    __shared__ unsigned char changed[DELTA_MAX_CHANGED];
    __shared__ int s_nch;
    __shared__ int s_wc[5][5];                                          // [wave][list] members among the wave's 64 positions
    const int b = blockIdx.x;
    if (b >= d.B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    AZ_DSTAMP(0);
    AZ_DSTAMP_VAL(14, __builtin_amdgcn_s_memrealtime());
#ifdef AZ_STAMPS
    for (int k = 1; k < 14; k++) AZ_DSTAMP_VAL(k, 0);
#endif
    {
        const int kind = d.leaf_kind[b];
        if (!((kind == LEAF_ROOT || kind == LEAF_EXPAND) && d.s_status[b] == SLOT_ACTIVE && d.s_net[b] == net_id)) {
            if (tid == 0) done[b] = 1;
            return;
        }
    }
    const float2 hq = reinterpret_cast<const float2 *>(w.hdq)[tid];
    const u64 *lf = d.leaf + (size_t)b * 8, *bd = d.board + (size_t)b * 8;
    const int last = d.leaf_last[b];
    // parity of the leaf: an even number of stones beyond the root's means the root's mover is to move
    int stones = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) stones += __popcll(lf[i]) - __popcll(bd[i]);
    const int par = stones & 1;
    bool e_me = false, e_op = false, e_last = false;
    int e_pos = G::PW + 1;
    if (tid == 0) s_nch = 0;
    for (int i = tid; i < 4 * G::CS; i += NT) planes[i] = 0.0f;
    reinterpret_cast<float2 *>(hdq_lds)[tid] = hq;
    __syncthreads();
    if (tid < G::nn) {
        const int r = tid / N, c = tid - r * N;
        e_pos = (r + 1) * G::PW + (c + 1);
        e_me = (lf[tid >> 6] >> (tid & 63)) & 1ull;
        e_op = (lf[4 + (tid >> 6)] >> (tid & 63)) & 1ull;
        e_last = last == tid;
        const bool x = (bd[tid >> 6] >> (tid & 63)) & 1ull, o = (bd[4 + (tid >> 6)] >> (tid & 63)) & 1ull;
        const bool me_is_x = (d.s_player[b] == 1) != (par == 1);
        if (e_me != (me_is_x ? x : o) || e_op != (me_is_x ? o : x) || e_last) {
            const int k = atomicAdd(&s_nch, 1);
            if (k < DELTA_MAX_CHANGED) changed[k] = (unsigned char)tid;
        }
        if (e_me) planes[e_pos] = 1.0f;
        if (e_op) planes[G::CS + e_pos] = 1.0f;
        if (e_last) planes[2 * G::CS + e_pos] = 1.0f;
    }
    __syncthreads();
    const int nch = s_nch;
    // full: the board is evaluated in full by this workgroup (delta_lists_full), uniform over the workgroup
    bool full = nch > DELTA_MAX_CHANGED;
    const int pr = tid / G::PW, pc = tid - pr * G::PW;
    int dist = 255;
    if (!full) {
        // the five lists, one thread per padded position: a member's place is the number of members in front of it
        u64 bal[5] = {0, 0, 0, 0, 0};
        if (wave < 5) {
            const bool in_img = tid < G::PP;
            if (in_img) dist = delta_dist(N, pr, pc, changed, nch);
#pragma unroll
            for (int l = 0; l < 5; l++) {
                bal[l] = __ballot(in_img && delta_member(N, l, pr, pc, dist));
                if (lane == 0) s_wc[wave][l] = __popcll(bal[l]);
            }
        }
        __syncthreads();
        if (wave < 5 && tid < G::PP) {
#pragma unroll
            for (int l = 0; l < 5; l++) {
                if (!((bal[l] >> lane) & 1ull)) continue;
                int at = __popcll(bal[l] & ((1ull << lane) - 1ull));
                for (int v = 0; v < wave; v++) at += s_wc[v][l];
                L.put(l, at, pr, pc);
            }
        }
        if (tid < 5) L.cnt[tid] = s_wc[0][tid] + s_wc[1][tid] + s_wc[2][tid] + s_wc[3][tid] + s_wc[4][tid];
        __syncthreads();
        full = L.tiles(2) > max_tiles;
        if (full) __syncthreads();          // every thread has read the count before the lists are written again
    }
    float *inA = lds, *inB = lds + 32 * G::CS;
    if (full) {
        // too many changed cells or conv3 tiles: all 225 cells at every layer, 15 tiles through the same chunk loops below
        if (tid < G::PP) delta_full_put<N>(L, pr, pc);
        if (tid < 5) delta_full_cnt<N>(L, tid);
        // no window is read: conv1 and conv2 write every board cell of their images, the ring has to be zero
        float4 *z = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < G::IMG / 4; i += NT) z[i] = float4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
    }
    const int t1 = L.tiles(0), t2 = L.tiles(1), t3 = L.tiles(2);
    AZ_DSTAMP(1);
    AZ_DSTAMP_VAL(13, t3);
    if (tid < 48) L.junk(tid >> 4, tid & 15);
    if (tid == 0) {
        if (full) { done[b] = 0; cnt[(size_t)b * DELTA_CNT + 1] += 1ull; }
        else {
            done[b] = (unsigned char)(1 + t3);
            cnt[(size_t)b * DELTA_CNT + 0] += 1ull;
            cnt[(size_t)b * DELTA_CNT + 2] += (unsigned long long)t3;
            cnt[(size_t)b * DELTA_CNT + 4 + t3] += 1ull;
        }
    }
    // The windows of the base images and the base feature row: every global load is issued before the first store.  Plane =
    // wave, list positions over the lanes, so no index is divided: the 8 float4 planes of conv1's image at list 3, planes w and
    // 8 + w of conv2's 16 at list 4, in WR rounds of 64 positions (a list holds at most PP positions: WR + 2 WR fragments per
    // thread bound what stays in registers, nothing is left over).  conv1's windows are stored in front of conv1.  conv2's
    // stay in registers through conv1, which reads neither image, and are stored in front of conv2: BEFORE conv2's epilogue
    // writes its cells of the same image, so no position has to be skipped.  The feature row: the thread of an in-board
    // position further than 3 from every changed cell copies the cell's 6 values (the heads write the others), each once.
    constexpr int WR = (G::PP + 63) / 64;
    static_assert(WR * 64 >= G::PP && G::NW == 8, "the rounds reach the longest list; one conv1 plane and two conv2 planes per wave");
    f32x4 w1[WR], w2[2][WR];
    float fr[6];
    f32x4 *l4 = reinterpret_cast<f32x4 *>(lds);
    float *frow = feat + (size_t)b * G::FROW;
    const bool keep = !full && tid < G::PP && delta_member(N, 2, pr, pc, 0) && dist > 3;      // (distance 0: is the position a board cell)
    const int fcell = (pr - 1) * N + (pc - 1);
    const int n3 = full ? 0 : L.cnt[3], n4 = full ? 0 : L.cnt[4];
    {
        const float *brow = base + ((size_t)b * 2 + par) * G::STRIDE;
        const f32x4 *g4 = reinterpret_cast<const f32x4 *>(brow);
        const float *bf = brow + G::IMG;
        delta_rounds<0, WR>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (j * 64 + lane < n3) w1[j] = g4[wave * G::CS + L.halo[0][j * 64 + lane]];
        });
        delta_rounds<0, WR>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (j * 64 + lane < n4) {
                const int pos = L.halo[1][j * 64 + lane];
                w2[0][j] = g4[(8 + wave) * G::CS + pos];
                w2[1][j] = g4[(16 + wave) * G::CS + pos];
            }
        });
        if (keep) {
#pragma unroll
            for (int i = 0; i < 6; i++) fr[i] = bf[i * G::nn + fcell];
        }
        delta_rounds<0, WR>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (j * 64 + lane < n3) l4[wave * G::CS + L.halo[0][j * 64 + lane]] = w1[j];
        });
    }
    __syncthreads();
    AZ_DSTAMP(2);
    for (int t0 = 0; t0 < t1; t0 += 4)
        conv_layer<G, 4, 32, CONV_OUT_PACKED, 4>(planes, inA, w.c1, w.c1b, L.wpos[0], L.cell[0], wave, lane, t0, t1 - t0 < 4 ? t1 - t0 : 4);
    delta_rounds<0, WR>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j * 64 + lane < n4) {
            const int pos = L.halo[1][j * 64 + lane];
            l4[(8 + wave) * G::CS + pos] = w2[0][j];
            l4[(16 + wave) * G::CS + pos] = w2[1][j];
        }
    });
    if (keep) {
#pragma unroll
        for (int i = 0; i < 6; i++) frow[i * G::nn + fcell] = fr[i];
    }
    __syncthreads();
    AZ_DSTAMP(3);
    for (int t0 = 0; t0 < t2;) {
        const int c = t2 - t0;
        if (c > 2) { conv_layer<G, 32, 64, CONV_OUT_PACKED, 4>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, c < 4 ? c : 4); t0 += 4; }
        else { conv_layer<G, 32, 64, CONV_OUT_PACKED, 2>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, c); t0 += 2; }
    }
    __syncthreads();
    AZ_DSTAMP(4);
    for (int t0 = 0; t0 < t3; t0 += G::C3) {
        const int c = t3 - t0 < G::C3 ? t3 - t0 : G::C3;
        // conv_layer counts the cell-major rows from tile 0 of the list: the chunk's first row is lds
        float *o3 = lds - t0 * 16 * OUT3_CM_STRIDE;
        if (c == 4) conv_layer<G, 64, 128, CONV_OUT3_CM, 4>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 4);
        else if (c == 3) conv_layer<G, 64, 128, CONV_OUT3_CM, 3>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 3);
        else if (c == 2) conv_layer<G, 64, 128, CONV_OUT3_CM, 2>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 2);
        else conv_layer<G, 64, 128, CONV_OUT3_CM, 1>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 1);
        __syncthreads();
        AZ_DSTAMP(5 + 2 * (t0 / G::C3));
        delta_heads<G>(w, frow, lds, hdq_lds, L.cell[2] + t0 * 16, c * 16, wave, lane);
        __syncthreads();
        AZ_DSTAMP(6 + 2 * (t0 / G::C3));
        AZ_DSTAMP_VAL(15, __builtin_amdgcn_s_memrealtime());
    }
}
#endif  // __HIPCC__
