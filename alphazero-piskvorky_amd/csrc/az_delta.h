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
//                  tiles is left to
//   k_trunk_rest   k_trunk's code (trunk_group) for the boards k_trunk_delta did not do.
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

#ifdef __HIPCC__
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

// done[b]: 0 = left to k_trunk_rest, 1 + conv3 tiles = evaluated here (or nothing to evaluate)
template <int N>
__global__ __launch_bounds__(NetGeo<N>::NW * 64) void k_trunk_delta(DevState d, NetWeights w, int net_id, float *__restrict__ feat,
                                                                     const float *__restrict__ base, unsigned char *done,
                                                                     unsigned long long *cnt, int max_tiles)
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
    __shared__ unsigned char s_dist[G::PP];
    __shared__ int s_nch;
    __shared__ int s_wc[5][5];                                          // [wave][list] members among the wave's 64 positions
    const int b = blockIdx.x;
    if (b >= d.B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
    if (nch > DELTA_MAX_CHANGED) {
        if (tid == 0) { done[b] = 0; cnt[(size_t)b * DELTA_CNT + 1] += 1ull; }
        return;
    }
    // the five lists, one thread per padded position: a member's place is the number of members in front of it
    int dist = 255, pr = 0, pc = 0;
    u64 bal[5] = {0, 0, 0, 0, 0};
    if (wave < 5) {
        const bool in_img = tid < G::PP;
        if (in_img) {
            pr = tid / G::PW; pc = tid - pr * G::PW;
            dist = delta_dist(N, pr, pc, changed, nch);
            s_dist[tid] = (unsigned char)dist;
        }
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
    const int t1 = L.tiles(0), t2 = L.tiles(1), t3 = L.tiles(2);
    if (t3 > max_tiles) {
        if (tid == 0) { done[b] = 0; cnt[(size_t)b * DELTA_CNT + 1] += 1ull; }
        return;
    }
    if (tid < 48) L.junk(tid >> 4, tid & 15);
    if (tid == 0) {
        done[b] = (unsigned char)(1 + t3);
        cnt[(size_t)b * DELTA_CNT + 0] += 1ull;
        cnt[(size_t)b * DELTA_CNT + 2] += (unsigned long long)t3;
        cnt[(size_t)b * DELTA_CNT + 4 + t3] += 1ull;
    }
    float *inA = lds, *inB = lds + 32 * G::CS;
    const float *brow = base + ((size_t)b * 2 + par) * G::STRIDE;
    {
        // the windows of the base images: 8 float4 planes of conv1's output at list 3, 16 of conv2's at list 4
        const float4 *g4 = reinterpret_cast<const float4 *>(brow);
        float4 *l4 = reinterpret_cast<float4 *>(lds);
        const int n3 = L.cnt[3], n4 = L.cnt[4];
        for (int i = tid; i < 8 * n3; i += NT) {
            const int pl = i / n3, at = pl * G::CS + L.halo[0][i - pl * n3];
            l4[at] = g4[at];
        }
        for (int i = tid; i < 16 * n4; i += NT) {
            const int pl = i / n4, at = (8 + pl) * G::CS + L.halo[1][i - pl * n4];
            l4[at] = g4[at];
        }
        // the feature row: the base's, without the cells the heads below write
        const float *bf = brow + G::IMG;
        float *frow = feat + (size_t)b * G::FROW;
        for (int i = tid; i < 6 * G::nn; i += NT) {
            const int p = i % G::nn, r = p / N, c = p - r * N;
            if (s_dist[(r + 1) * G::PW + (c + 1)] > 3) frow[i] = bf[i];
        }
    }
    __syncthreads();
    for (int t0 = 0; t0 < t1; t0 += 4)
        conv_layer<G, 4, 32, CONV_OUT_PACKED, 4>(planes, inA, w.c1, w.c1b, L.wpos[0], L.cell[0], wave, lane, t0, t1 - t0 < 4 ? t1 - t0 : 4);
    __syncthreads();
    for (int t0 = 0; t0 < t2;) {
        const int c = t2 - t0;
        if (c > 2) { conv_layer<G, 32, 64, CONV_OUT_PACKED, 4>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, c < 4 ? c : 4); t0 += 4; }
        else { conv_layer<G, 32, 64, CONV_OUT_PACKED, 2>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, c); t0 += 2; }
    }
    __syncthreads();
    float *frow = feat + (size_t)b * G::FROW;
    for (int t0 = 0; t0 < t3; t0 += G::C3) {
        const int c = t3 - t0 < G::C3 ? t3 - t0 : G::C3;
        // conv_layer counts the cell-major rows from tile 0 of the list: the chunk's first row is lds
        float *o3 = lds - t0 * 16 * OUT3_CM_STRIDE;
        if (c == 4) conv_layer<G, 64, 128, CONV_OUT3_CM, 4>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 4);
        else if (c == 3) conv_layer<G, 64, 128, CONV_OUT3_CM, 3>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 3);
        else if (c == 2) conv_layer<G, 64, 128, CONV_OUT3_CM, 2>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 2);
        else conv_layer<G, 64, 128, CONV_OUT3_CM, 1>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 1);
        __syncthreads();
        delta_heads<G>(w, frow, lds, hdq_lds, L.cell[2] + t0 * 16, c * 16, wave, lane);
        __syncthreads();
    }
}

// k_trunk's work for the boards k_trunk_delta left: the same trunk_group, behind the per-board flag
template <int N>
__global__ __launch_bounds__(NetGeo<N>::NW * 64) void k_trunk_rest(DevState d, NetWeights w, int net_id, float *__restrict__ feat,
                                                                    const unsigned char *done)
{
    typedef FusedGeo<N> G;
    static_assert(G::G == 1, "one board per workgroup");
    __shared__ __attribute__((aligned(16))) float lds[G::LDSF];
    __shared__ __attribute__((aligned(16))) float hdq_lds[1024];
    __shared__ unsigned short wpos[G::MR];
    __shared__ unsigned short cellof[G::MR];
    __shared__ int any_active;
    const int grp = blockIdx.x;
    if (grp >= d.B || done[grp]) return;
    trunk_group<N>(d, w, net_id, feat, nullptr, grp, lds, hdq_lds, wpos, cellof, &any_active, threadIdx.x);
}
#endif  // __HIPCC__
