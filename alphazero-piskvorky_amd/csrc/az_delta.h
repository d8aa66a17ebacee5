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
//                  three lists of 16-cell tiles; conv1 is recomputed from the leaf's own planes on the widest list (5i: 4 input
//                  planes, nearly free, and nothing to wait for), the window of the base conv2 image that conv3's tiles read is
//                  copied into LDS, conv2 and conv3 run on their listed tiles only (conv_layer's subset mode, no border-tap
//                  skipping), and the feature row is the base row with the conv3-region cells replaced.  A board with too many changed cells or conv3
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
//   list 0 / 1 / 2  board cells within 1 / 2 / 3 of a changed cell: the 3x3 / 5x5 / 7x7 footprints.  conv2 computes list 1, conv3
//                   and the heads list 2 -- and so does conv1 (5i), in place of copying its window; list 0 is only reported
//   list 3          padded positions (ring included) within 3: the region conv1 computes (its board cells ARE list 2, in order)
//                   plus the ring positions the kernel zeroes; the kernel does not build it
//   list 4          padded positions within 4: the window of the base conv2 image that conv3 reads
__host__ __device__ inline bool delta_member(int n, int list, int pr, int pc, int dist)
{
    const bool inb = pr >= 1 && pr <= n && pc >= 1 && pc <= n;
    return list < 3 ? (inb && dist <= list + 1) : dist <= list;
}
// Tile lists as conv_layer addresses them: lane m of a list computes the cell at padded position wpos[m]; the lanes behind the
// last cell, up to a whole tile, repeat the last cell's position (inside the computed / copied region at every tap) and are marked junk.
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
    __host__ __device__ void junk_at(int list, int c, int i, int pos)   // ... of a list of c cells whose last one lies at pos
    {
        const int at = c + i;
        if (i >= 0 && i < 16 && at < ((c + 15) >> 4) * 16) { wpos[list][at] = (unsigned short)pos; cell[list][at] = 0xFFFF; }
    }
};
// The lists of a set of changed cells, one position after the other: what k_trunk_delta builds with one thread per position
// (same members, same order; the kernel leaves out list 3 and cnt[]), here so that the integer logic can be checked on the CPU.
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

// The changed cells of a leaf against its base evaluation, a pure function of the 16 board words (5i): leaf = the pending leaf's
// planes (words 0-3 side to move, 4-7 opponent), board = the root's (words 0-3 X, 4-7 O), player = the root's mover (1 / 2),
// last = the leaf's last move or -1.  The leaf's parity is the number of stones beyond the root's, mod 2: even means the root's
// mover is to move, and the base of that parity shows the root's stones from that side with an empty last-move plane.  A cell
// is changed where either plane differs from the base's or where the last move lies.  Returns the k-th changed cell in
// ascending order (0xFF where there are not that many), their number in *count.  The 16 words are the same in every lane and
// cost scalar arithmetic once; only the walk to the k-th set bit depends on k, so in the kernel lane k finds cell k and the
// wave reads the first DELTA_MAX_CHANGED of them back (extracting them one after the other in every wave cost 600 scalar
// instructions per wave on the one scalar unit of the CU).
template <int N>
__host__ __device__ inline __attribute__((always_inline)) int delta_changed(const u64 *leaf, const u64 *board, int player, int last, int k, int *count, int *parity)
{
    static_assert(N * N > 192 && N * N <= 256, "four words of cells, the last one in part");
    int stones = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) stones += __builtin_popcountll(leaf[i]) - __builtin_popcountll(board[i]);
    const int par = stones & 1;
    const bool me_is_x = (player == 1) != (par == 1);
    u64 v = 0;
    int total = 0, wi = 0, kk = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u64 bme = me_is_x ? board[i] : board[4 + i], bop = me_is_x ? board[4 + i] : board[i];
        u64 dw = (leaf[i] ^ bme) | (leaf[4 + i] ^ bop);
        if (last >= 0 && last < N * N && (last >> 6) == i) dw |= 1ull << (last & 63);
        if (i == 3 && N * N < 256) dw &= (1ull << ((N * N) & 63)) - 1ull;             // only board cells count
        const int c = __builtin_popcountll(dw);
        if (k >= total && k < total + c) { v = dw; wi = i; kk = k - total; }         // the word that holds the k-th changed cell
        total += c;
    }
#pragma unroll
    for (int j = 0; j < DELTA_MAX_CHANGED - 1; j++)
        if (j < kk) v &= v - 1ull;
    *count = total;
    *parity = par;
    return (k >= 0 && k < total && k < DELTA_MAX_CHANGED && v) ? wi * 64 + __builtin_ctzll(v) : 0xFF;
}

#ifdef __HIPCC__
// a per-slot counter of the delta kernel: one workgroup per slot and launch, so the add needs no result and no round trip
__device__ __forceinline__ void delta_count(unsigned long long *p, unsigned long long v)
{
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a board word, the same in every lane, moved to scalar registers: what delta_changed makes of it is scalar arithmetic
__device__ __forceinline__ u64 delta_uniform(u64 v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}

// diagnostic builds only (-DAZ_STAMPS): k_trunk_delta's phase stamps (s_memtime), 16 u64 per workgroup in k_trunk's rows of the
// debug buffer.  0 entry, 1 lists done, 2 window loads issued, 3 conv1 and the window stores, 4 conv2, 5 + 2 i / 6 + 2 i conv3
// chunk i / its heads pass (zero where the leaf has no such chunk), 13 the conv3 tile count (bits 0-7) and the conv2 tile count
// (bits 8-15), 14 / 15 s_memrealtime at entry / at the last heads pass
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
// Prologue (5i): every entry load is issued before the early-exit test; the changed cells come from delta_changed on the 16
// board words every wave holds (no LDS atomic, no barrier of their own); each padded position's thread writes its planes once,
// builds its part of lists 0, 1, 2 and 4 and, on the ring within 3 of a changed cell, zeroes conv1's image; the first lanes
// of the wave that puts a list's last cell write the junk lanes behind it.  Two barriers lie between entry and the window loads.
template <int N>
__global__ __launch_bounds__(NetGeo<N>::NW * 64) void k_trunk_delta(DevState d, NetWeights w, int net_id, float *__restrict__ feat,
                                                                     const float *__restrict__ base, unsigned char *done,
                                                                     unsigned long long *cnt, int max_tiles, unsigned long long *dbg)
{
    typedef DeltaGeo<N> G;
    constexpr int NT = G::NW * 64;
    static_assert(G::G == 1 && NT >= G::CS && NT == 512, "one board per workgroup, one thread per padded position");
    static_assert(G::C3 * 16 * OUT3_CM_STRIDE <= 32 * G::CS, "a chunk's conv3 image fits the dead conv1 image");
    static_assert(G::STRIDE % 4 == 0, "16-byte rows");
    __shared__ __attribute__((aligned(16))) float lds[G::IMG];          // conv1 image, conv2 image; a conv3 chunk overlays the first
    __shared__ __attribute__((aligned(16))) float planes[4 * G::CS];    // me, opponent, last move, zeros
    __shared__ __attribute__((aligned(16))) float hdq_lds[1024];
    __shared__ DeltaLists<N> L;                                         // (cnt[] is the host's: the kernel keeps the counts in registers)
    __shared__ __attribute__((aligned(16))) int s_wc[5][4];                                       // [wave][list 0, 1, 2, 4] members among the wave's 64 positions
    const int b = blockIdx.x;
    if (b >= d.B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    AZ_DSTAMP(0);
    AZ_DSTAMP_VAL(14, __builtin_amdgcn_s_memrealtime());
#ifdef AZ_STAMPS
    for (int k = 1; k < 14; k++) AZ_DSTAMP_VAL(k, 0);
#endif
    // every entry load at once (all indices are in bounds for b < d.B), conv1's weights with them
    const int kind = d.leaf_kind[b], status = d.s_status[b], snet = d.s_net[b], last = d.leaf_last[b], player = d.s_player[b];
    u64 lf[8], bd[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { lf[i] = delta_uniform(d.leaf[(size_t)b * 8 + i]); bd[i] = delta_uniform(d.board[(size_t)b * 8 + i]); }
    const float2 hq = reinterpret_cast<const float2 *>(w.hdq)[tid];
    const ConvPre<4> pre1 = conv_prefetch<G, 4, 32>(w.c1, wave, lane);
    if (!((kind == LEAF_ROOT || kind == LEAF_EXPAND) && status == SLOT_ACTIVE && snet == net_id)) {
        if (tid == 0) done[b] = 1;
        return;
    }
    int ch[DELTA_MAX_CHANGED], par, nch;
    {
        // lane k finds the k-th changed cell; every wave reads the first eight back into scalar registers
        const int mine = delta_changed<N>(lf, bd, player, last, lane & (DELTA_MAX_CHANGED - 1), &nch, &par);
#pragma unroll
        for (int i = 0; i < DELTA_MAX_CHANGED; i++) ch[i] = __builtin_amdgcn_readlane(mine, i);
    }
    // full: the board is evaluated in full by this workgroup (delta_lists_full), uniform over the workgroup
    bool full = nch > DELTA_MAX_CHANGED;
    const int pr = tid / G::PW, pc = tid - pr * G::PW;
    const bool in_img = tid < G::PP, inb = in_img && pr >= 1 && pr <= N && pc >= 1 && pc <= N;
    const int fcell = (pr - 1) * N + (pc - 1);
    f32x4 *l4 = reinterpret_cast<f32x4 *>(lds);
    if (tid < G::CS) {
        // the input planes, each position once: the position's own cell, zeros on the ring and behind the image
        const int cp = inb ? fcell : 0, wi = cp >> 6;
        const u64 me = wi == 0 ? lf[0] : wi == 1 ? lf[1] : wi == 2 ? lf[2] : lf[3];
        const u64 op = wi == 0 ? lf[4] : wi == 1 ? lf[5] : wi == 2 ? lf[6] : lf[7];
        planes[tid] = inb && ((me >> (cp & 63)) & 1ull) ? 1.0f : 0.0f;
        planes[G::CS + tid] = inb && ((op >> (cp & 63)) & 1ull) ? 1.0f : 0.0f;
        planes[2 * G::CS + tid] = inb && last == cp ? 1.0f : 0.0f;
        planes[3 * G::CS + tid] = 0.0f;
    }
    int dist = 255;
    u64 bal[4] = {0, 0, 0, 0};
    if (!full && wave < 5) {
        // lists 0, 1, 2 and 4, one thread per padded position: a member's place is the number of members in front of it
        if (in_img) {
#pragma unroll
            for (int i = 0; i < DELTA_MAX_CHANGED; i++) {
                if (i < nch) {
                    const int cr = ch[i] / N, cc = ch[i] - cr * N;
                    const int dr = pr - 1 - cr < 0 ? cr - (pr - 1) : pr - 1 - cr, dc = pc - 1 - cc < 0 ? cc - (pc - 1) : pc - 1 - cc;
                    const int dd = dr > dc ? dr : dc;
                    dist = dd < dist ? dd : dist;
                }
            }
        }
#pragma unroll
        for (int l = 0; l < 4; l++) {
            bal[l] = __ballot(in_img && delta_member(N, l < 3 ? l : 4, pr, pc, dist));
            if (lane == 0) s_wc[wave][l] = __popcll(bal[l]);
        }
        // conv1 runs on list 2 and conv2 reads one position further: the ring positions within 3 are zeros of conv1's image
        if (in_img && !inb && dist <= 3) {
#pragma unroll
            for (int k = 0; k < 8; k++) l4[k * G::CS + tid] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
    int c[4] = {G::nn, G::nn, G::nn, 0}, front[4] = {0, 0, 0, 0};        // a list's members, and those of the waves in front of this one
    if (!full) {
        c[0] = c[1] = c[2] = 0;
#pragma unroll
        for (int v = 0; v < 5; v++) {
            const int4 r = reinterpret_cast<const int4 *>(&s_wc[0][0])[v];
            const int rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int l = 0; l < 4; l++) { c[l] += rv[l]; front[l] += v < wave ? rv[l] : 0; }
        }
        full = ((c[2] + 15) >> 4) > max_tiles;
        if (full) { c[0] = c[1] = c[2] = G::nn; c[3] = 0; }
    }
    if (!full) {
        if (wave < 5 && in_img) {
#pragma unroll
            for (int l = 0; l < 4; l++) {
                if ((bal[l] >> lane) & 1ull) L.put(l < 3 ? l : 4, front[l] + __popcll(bal[l] & ((1ull << lane) - 1ull)), pr, pc);
                // the junk lanes, by the first lanes of the wave that holds the list's last cell: a padded position is its
                // thread's index, so the last cell's position is the wave's base plus the highest member lane
                if (l < 3 && bal[l] && front[l] + __popcll(bal[l]) == c[l])
                    L.junk_at(l, c[l], lane, wave * 64 + 63 - __builtin_clzll(bal[l]));
            }
        }
    } else {
        // too many changed cells or conv3 tiles: all 225 cells at every layer, 15 tiles through the same chunk loops below
        if (in_img) delta_full_put<N>(L, pr, pc);
#pragma unroll
        for (int l = 0; l < 3; l++) L.junk_at(l, G::nn, tid, N * G::PW + N);
        // no window is read: conv1 and conv2 write every board cell of their images, the ring has to be zero
        for (int i = tid; i < G::IMG / 4; i += NT) l4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    const int t2 = (c[1] + 15) >> 4, t3 = (c[2] + 15) >> 4, n4 = c[3];
    AZ_DSTAMP(1);
    AZ_DSTAMP_VAL(13, t3 | (t2 << 8));
    if (tid == 0) {
        // counters off the path: adds that return nothing, so that wave 0 does not wait for them in front of its window loads
        unsigned long long *cb = cnt + (size_t)b * DELTA_CNT;
        if (full) { done[b] = 0; delta_count(cb + 1, 1ull); }
        else {
            done[b] = (unsigned char)(1 + t3);
            delta_count(cb + 0, 1ull);
            delta_count(cb + 2, (unsigned long long)t3);
            delta_count(cb + 4 + t3, 1ull);
        }
    }
    // The windows of the base conv2 image and the base feature row: every global load is issued before the first store.  Plane =
    // wave, list positions over the lanes, so no index is divided: planes w and 8 + w of conv2's 16 float4 planes at list 4, in
    // WR rounds of 64 positions (a list holds at most PP positions: 2 WR fragments per thread bound what stays in registers,
    // nothing is left over).  They stay in registers through conv1, which reads neither image, and are stored in front of conv2:
    // BEFORE conv2's epilogue writes its cells of the same image, so no position has to be skipped.  Nothing is loaded for
    // conv1 (5i): it recomputes the cells of list 2 from the planes.  The feature row: the thread of an in-board position
    // further than 3 from every changed cell copies the cell's 6 values (the heads write the others), each once.
    constexpr int WR = (G::PP + 63) / 64;
    static_assert(WR * 64 >= G::PP && G::NW == 8, "the rounds reach the longest list; two conv2 planes per wave");
    f32x4 w2[2][WR];
    float fr[6];
    float *frow = feat + (size_t)b * G::FROW;
    const bool keep = !full && inb && dist > 3;
    {
        const float *brow = base + ((size_t)b * 2 + par) * G::STRIDE;
        const f32x4 *g4 = reinterpret_cast<const f32x4 *>(brow);
        const float *bf = brow + G::IMG;
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
    }
    // conv2's first weight fragments fly under conv1, conv3's under conv2; they are the same for every chunk of a layer and stay
    // in registers, so no chunk starts with a weight fetch
    const ConvPre<32> pre2 = conv_prefetch<G, 32, 64>(w.c2, wave, lane);
    AZ_DSTAMP(2);
    float *inA = lds, *inB = lds + 32 * G::CS;
    for (int t0 = 0; t0 < t3; t0 += 4)
        conv_layer<G, 4, 32, CONV_OUT_PACKED, 4>(planes, inA, w.c1, w.c1b, L.wpos[2], L.cell[2], wave, lane, t0, t3 - t0 < 4 ? t3 - t0 : 4,
                                                 0, nullptr, nullptr, &pre1);
    reinterpret_cast<float2 *>(hdq_lds)[tid] = hq;
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
    // exact tile counts: a chunk of c tiles runs the c-tile instantiation, no surplus chain (5i)
    for (int t0 = 0; t0 < t2; t0 += 4) {
        const int c2 = t2 - t0 < 4 ? t2 - t0 : 4;
        if (c2 == 4) conv_layer<G, 32, 64, CONV_OUT_PACKED, 4>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, 4, 0, nullptr, nullptr, &pre2);
        else if (c2 == 3) conv_layer<G, 32, 64, CONV_OUT_PACKED, 3>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, 3, 0, nullptr, nullptr, &pre2);
        else if (c2 == 2) conv_layer<G, 32, 64, CONV_OUT_PACKED, 2>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, 2, 0, nullptr, nullptr, &pre2);
        else conv_layer<G, 32, 64, CONV_OUT_PACKED, 1>(inA, inB, w.c2, w.c2b, L.wpos[1], L.cell[1], wave, lane, t0, 1, 0, nullptr, nullptr, &pre2);
    }
    __syncthreads();
    AZ_DSTAMP(4);
    for (int t0 = 0; t0 < t3; t0 += G::C3) {
        const int c3 = t3 - t0 < G::C3 ? t3 - t0 : G::C3;
        // conv_layer counts the cell-major rows from tile 0 of the list: the chunk's first row is lds
        float *o3 = lds - t0 * 16 * OUT3_CM_STRIDE;
        if (c3 == 4) conv_layer<G, 64, 128, CONV_OUT3_CM, 4>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 4);
        else if (c3 == 3) conv_layer<G, 64, 128, CONV_OUT3_CM, 3>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 3);
        else if (c3 == 2) conv_layer<G, 64, 128, CONV_OUT3_CM, 2>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 2);
        else conv_layer<G, 64, 128, CONV_OUT3_CM, 1>(inB, o3, w.c3, w.c3b, L.wpos[2], L.cell[2], wave, lane, t0, 1);
        __syncthreads();
        AZ_DSTAMP(5 + 2 * (t0 / G::C3));
        delta_heads<G>(w, frow, lds, hdq_lds, L.cell[2] + t0 * 16, c3 * 16, wave, lane);
        __syncthreads();
        AZ_DSTAMP(6 + 2 * (t0 / G::C3));
        AZ_DSTAMP_VAL(15, __builtin_amdgcn_s_memrealtime());
    }
}
#endif  // __HIPCC__
