// az_net.h -- the policy/value net forward as HIP kernels for gfx950.
//
//  k_trunk     : GomokuNet (net.py:55-72): leaf encode (games.py:86-129) -> conv1 -> conv2 -> conv3 -> policy/value
//                1x1 convs.  One workgroup per group of G boards, every activation resident in LDS: zero-padded
//                images, so the 3x3 im2col is "base + constant offset"; conv2/conv3 inputs in a packed layout read
//                with ds_read_b128; contraction on v_mfma_f32_16x16x4_f32 with the weights as the A operand.
//  k_trunk_res : the ResidualBlock variant (BASELINE config 5): stem + 3 residual blocks + 1x1 heads, same machinery.
//  k_fc        : policy_fc and value_fc1 as a batched GEMM over boards, same MFMA, one k-ordered chain per output.
// softmax / value_fc2 / tanh are fused into the tree kernel that consumes them (az_tree.h).
//
// Numerics: every output element is ONE k-ordered fp32 fma chain from +0 (what the f32 MFMA computes,
// bit for bit), bias added afterwards.  conv k = (ky*3+kx)*Cin + ci; FC k ascending.
#pragma once
#include "az_tree.h"
#include <type_traits>

#ifdef AZ_STAMPS
// diagnostic build only: per-workgroup phase time stamps (s_memtime) into a buffer no other code reads
// slots 0..5: s_memtime (shader clock ticks) at the phase boundaries; slots 14 / 15: s_memrealtime (the constant 100 MHz counter)
// at the first and the last stamp, so that the clock the chip HELD inside the kernel is (t5 - t0) / (rt5 - rt0) x 100 MHz
// (MI355X_MICROARCH.md, DVFS give-back item 6)
#define AZ_STAMP(k) do { if (threadIdx.x == 0 && dbg) { dbg[(size_t)grp * 16 + (k)] = __builtin_amdgcn_s_memtime(); \
    if ((k) == 0) dbg[(size_t)grp * 16 + 14] = __builtin_amdgcn_s_memrealtime(); \
    if ((k) == 5) dbg[(size_t)grp * 16 + 15] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define AZ_STAMP(k) do { } while (0)
#endif

struct NetWeights {
    // MFMA-fragment packed (see pack_* in az_engine.hip): [ntile][kstep/4][lane][4]
    const float *c1, *c2, *c3, *hd, *pf, *vf;
    const float *hdq;                                 // the head convs again, in 4-row block order for the fused trunk (pack_heads_blocks): [k/4][8 rows][4]
    const float *c1b, *c2b, *c3b, *hdb, *pfb, *vfb;   // biases (hdb: 4 policy_conv + 2 value_conv)
    const void *c1x[2], *c2x[2], *c3x[2], *hdx[2];    // the convs and head convs split into 16-bit fragments (az_net_emul.h), [0] bf16x3, [1] f16x2
};

// Canonical order of an FC output over K inputs (oracle: fc_dot): the inputs are taken in groups of 16 (four k-steps of
// v_mfma_f32_16x16x4_f32) and cut into FOUR contiguous blocks of fc_chain_groups(K) groups; each block is one k-ordered fma
// chain from +0, and the output is ((p0 + p1) + (p2 + p3)) + bias.  Four chains instead of one so that an output tile's
// contraction spreads over four wavefronts (k_fc) or four independent accumulators (k_search) -- a 15x15 policy output is
// 4 x 60 dependent MFMAs instead of 228.
__host__ __device__ constexpr int fc_chain_groups(int K) { return (((K + 15) / 16) + 3) / 4; }

__host__ __device__ constexpr int up16(int x) { return x + ((16 - (x % 32) + 32) % 32); }   // smallest y >= x, y == 16 (mod 32)

// Row stride (floats) of the fused trunk's cell-major conv3 image out3[tile cell][channel]: 128 channels + 4, so that consecutive
// cells start 4 LDS banks apart and a row stays 16-byte aligned (528 B)
constexpr int OUT3_CM_STRIDE = 128 + 4;

// Boards per trunk workgroup for an n x n board: as many as fit the LDS budget, at most 4 (so that 1024 games still
// give >= 256 workgroups).  chan = LDS floats per padded cell (96 plain net: 32+64 channels; 128 ResidualBlock net).
__host__ __device__ constexpr int trunk_lds_floats(int n, int g, int chan)
{
    const int cs = up16(g * (n + 2) * (n + 2));
    const int mr = ((g * n * n + 15) / 16) * 16;
    // plain net: the conv3 images overlay the inputs -- [co][cell] with stride up16(mr) (the emulated trunks) and the fused
    // trunk's cell-major one, [cell][OUT3_CM_STRIDE]
    const int a = chan * cs, b = chan == 96 ? 128 * up16(mr) : 0, c = chan == 96 ? OUT3_CM_STRIDE * mr : 0;
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}
constexpr int TRUNK_LDS_BUDGET = 36500;     // LDS floats the packed images of one trunk workgroup may take (146 KB)
__host__ __device__ constexpr int pick_boards(int n, int chan, int budget)
{
    // powers of two only: 1024 x k games then split into whole rounds of 256 workgroups (3 boards per workgroup left
    // the last round of a 4096-game 9x9 launch one-third full)
    int g = 1;
    for (int t = 2; t <= 4; t *= 2)
        if (trunk_lds_floats(n, t, chan) <= budget) g = t;
    return g;
}

template <int N>
struct NetGeo {
    static constexpr int n = N, nn = N * N, PW = N + 2, PP = PW * PW;
    static constexpr int G = pick_boards(N, 96, TRUNK_LDS_BUDGET);       // boards per workgroup: 1 at n >= 12, 2 at 8-11, 4 below
    static constexpr int M = G * nn;                               // real GEMM columns (board cells)
    // 16-cell MFMA tiles.  n = 15: one tile = one board row + its right padding cell (contiguous in the padded
    // image, so the 16 lanes of a fragment hit 16 consecutive LDS banks); other sizes: 16 consecutive cells.
    // Row tiles are what k_tile (grid: boards x board rows), the emulated trunks and the FC constants use at n = 15; the fused
    // float32 trunk keeps MT, MR and the images but lays its 15 tiles round the board instead (RingGeo below).
    static constexpr bool ROWT = (N == 15);
    static constexpr int MT = ROWT ? G * N : (M + 15) / 16, MR = MT * 16;
    static constexpr int CS = up16(G * PP);                        // channel stride of padded planes (floats), == 16 mod 32
    static constexpr int CS3 = up16(MR);                           // channel stride of the conv3 output image
    static constexpr int LDSF = trunk_lds_floats(N, G, 96);       // max(96 CS, 128 CS3, OUT3_CM_STRIDE MR)
    static constexpr int RW = ((nn + 63) / 64) * 64;
    static constexpr int NW = 8;                                   // waves per trunk workgroup
    static_assert(G == (N >= 12 ? 1 : N >= 8 ? 2 : 4), "the cell-major conv3 image must not change the boards per workgroup");
    static_assert(LDSF >= 96 * CS && LDSF >= 128 * CS3 && LDSF >= OUT3_CM_STRIDE * MR, "LDS images of the trunk");
    static_assert(LDSF * 4 + 2 * MR * 2 + 4096 + 64 <= 160 * 1024, "a trunk workgroup stays under the CU's 160 KB of LDS");
    // FC kernel
    static constexpr int PC = 4, VC = 2;                           // policy_conv / value_conv output channels (net.py:46,52)
    static constexpr int NTP = (nn + 15) / 16;                     // policy N-tiles
    static constexpr int FROW = (((PC + VC) * nn + 3) / 4) * 4;    // feature row in HBM: [0,PC*nn) policy, [PC*nn,(PC+VC)*nn) value, zero tail
    // FC layers (fc_chains below): K inputs = groups of 16 (four MFMA k-steps), cut into 4 chains of QG groups each
    static constexpr int QGP = fc_chain_groups(PC * nn), QGV = fc_chain_groups(VC * nn);
    static constexpr int QGMAX = QGP > QGV ? QGP : QGV;
        // LDS feature rows of the persistent search kernel: policy inputs, then value inputs, each padded to whole chains (zeros)
    static constexpr int VOFFL = 64 * QGP;
    static constexpr int FSTR0 = 64 * (QGP + QGV);
    static constexpr int FSTR = FSTR0 + ((4 - (FSTR0 % 32) + 32) % 32);   // LDS row stride, == 4 (mod 32), multiple of 4
};

// The ring tiling of the fused float32 trunk at n = 15 (RingGeo below): tile lane -> padded-image position and board cell.
//   tile 0 / n - 1     : row 0 / row n - 1, all 15 columns                         1 junk lane each
//   tile 1 / n - 2     : column 0 / column n - 1, rows 1..13                       3 junk lanes each
//   tiles 2 .. n - 3   : the 13 x 13 interior, 169 cells in 11 x 16 lanes          7 junk lanes
// so that a whole tile, not one lane of sixteen, faces each zero border: the row tiles have nothing to add at ky = 0 / ky = 2
// as before, and the column tiles nothing at kx = 0 / kx = 2 (conv_layer, BorderSkip).
// Banks: a fragment read is one ds_read_b128 per lane at float4 index (cg*4 + q) * CS + pos, served 16 lanes at a time (each
// group takes lanes r16 {0-3, 12-15} of one q and {4-11} of the next, i.e. sixteen DIFFERENT r16); the bank is 4 (index mod 16) and
// CS is a multiple of 16, so a read is conflict-free exactly when the 16 lanes of a tile have distinct pos mod 16 =
// (r + c + 2) mod 16.  A row has 15 consecutive residues and a column's positions are PW = 17 apart.  The interior cannot have it
// everywhere: the diagonals r + c = 13, 14, 15 hold 12, 13 and 12 interior cells against 11 tiles, so at least 4 cells share a
// residue with a tile-mate.  The fill reaches 4: the cells in row-major order, each into the first interior tile that has fewer than
// 15 cells and none of its residue (L-shaped runs of the board, so the heads' feature stores stay mostly contiguous); the four
// cells that find no such tile take the 16th lane of tiles 2..5, one each.
// Each of the 4 pairs costs its tile a second pass in EVERY 16-lane group of a read (a group holds one lane of each r16): 8 cycles
// instead of 4 for the reads of tiles 2..5 (SQ_LDS_BANK_CONFLICT, and that it stays behind the MFMA issue).
// A junk lane repeats the position of its tile's last cell: an identical LDS address is a broadcast (measured: the conflict
// counter reads the same to the digit with every junk lane on a residue of its own instead), it stays inside the image at
// every tap offset, and it keeps a border tile's dead taps dead.  Its cellof is 0xFFFF.
template <int N>
struct RingMap {
    unsigned short pos[N * 16], cell[N * 16];
    int cnt[N];
    __host__ __device__ constexpr void put(int t, int r, int c)
    {
        pos[t * 16 + cnt[t]] = (unsigned short)((r + 1) * (N + 2) + (c + 1));
        cell[t * 16 + cnt[t]] = (unsigned short)(r * N + c);
        cnt[t]++;
    }
    __host__ __device__ constexpr bool has_residue(int t, int res) const
    {
        for (int i = 0; i < cnt[t]; i++) if ((pos[t * 16 + i] & 15) == res) return true;
        return false;
    }
};
template <int N>
__host__ __device__ constexpr RingMap<N> ring_map()
{
    RingMap<N> m{};
    for (int c = 0; c < N; c++) { m.put(0, 0, c); m.put(N - 1, N - 1, c); }
    for (int r = 1; r < N - 1; r++) { m.put(1, r, 0); m.put(N - 2, r, N - 1); }
    int spill_r[N] = {}, spill_c[N] = {}, ns = 0;
    for (int r = 1; r < N - 1; r++)
        for (int c = 1; c < N - 1; c++) {
            int t = 2;
            while (t < N - 2 && (m.cnt[t] >= 15 || m.has_residue(t, (r + c + 2) & 15))) t++;
            if (t < N - 2) m.put(t, r, c);
            else if (ns < N) { spill_r[ns] = r; spill_c[ns] = c; ns++; }
        }
    for (int j = 0; j < ns && j < N - 4; j++) m.put(2 + j, spill_r[j], spill_c[j]);
    for (int t = 0; t < N; t++)
        for (int i = m.cnt[t]; i < 16; i++) { m.pos[t * 16 + i] = m.pos[t * 16 + m.cnt[t] - 1]; m.cell[t * 16 + i] = 0xFFFF; }
    return m;
}
// what RingGeo asserts of the map
template <int N>
__host__ __device__ constexpr bool ring_cells_once(const RingMap<N> &m)
{
    int seen[N * N] = {};
    for (int i = 0; i < N * 16; i++) if (m.cell[i] != 0xFFFF) { if (m.cell[i] >= N * N) return false; seen[m.cell[i]]++; }
    for (int p = 0; p < N * N; p++) if (seen[p] != 1) return false;
    return true;
}
template <int N>
__host__ __device__ constexpr bool ring_borders(const RingMap<N> &m)      // the border tiles hold cells of their border only, at their positions
{
    for (int i = 0; i < N * 16; i++) {
        const int t = i >> 4, p = m.cell[i];
        if (p == 0xFFFF) continue;
        const int r = p / N, c = p - r * N;
        if (m.pos[i] != (r + 1) * (N + 2) + (c + 1)) return false;
        if ((t == 0 && r != 0) || (t == N - 1 && r != N - 1) || (t == 1 && c != 0) || (t == N - 2 && c != N - 1)) return false;
    }
    return true;
}
template <int N>
__host__ __device__ constexpr int ring_conflicts(const RingMap<N> &m, bool worst_tile)     // lane pairs at different positions with equal pos mod 16
{
    int total = 0, worst = 0;
    for (int t = 0; t < N; t++) {
        int k = 0;
        for (int i = 0; i < 16; i++)
            for (int j = i + 1; j < 16; j++) {
                const int a = m.pos[t * 16 + i], b = m.pos[t * 16 + j];
                if (a != b && (a & 15) == (b & 15)) k++;
            }
        total += k;
        if (k > worst) worst = k;
    }
    return worst_tile ? worst : total;
}
template <int N>
__host__ __device__ constexpr bool ring_in_image(const RingMap<N> &m)
{
    for (int i = 0; i < N * 16; i++)
        if (m.pos[i] < (N + 2) + 1 || m.pos[i] > (N + 2) * (N + 2) - (N + 2) - 2) return false;
    for (int t = 0; t < N; t++)          // a junk lane repeats a cell of its own tile
        for (int i = 0; i < 16; i++) {
            if (m.cell[t * 16 + i] != 0xFFFF) continue;
            bool twin = false;
            for (int j = 0; j < 16; j++) if (m.cell[t * 16 + j] != 0xFFFF && m.pos[t * 16 + j] == m.pos[t * 16 + i]) twin = true;
            if (!twin) return false;
        }
    return true;
}

// Geometry of the fused float32 plain trunk at n = 15 (trunk_group<15> / k_trunk<15> only): NetGeo<15>'s images, tile count, waves
// and LDS, with the tiles laid round the board (RingMap above) and the predicate that tells conv_layer which (tile, tap) pairs
// multiply nothing but a zero border: 12 of the 135 per layer.
template <int N>
struct RingGeo : NetGeo<N> {
    typedef NetGeo<N> B;
    static_assert(N == 15 && B::G == 1 && B::MT == N, "one board per workgroup, as many tiles as board rows");
    static constexpr bool BORDER_SKIP = true;                      // conv_layer leaves out the taps that tap_dead names
    static constexpr RingMap<N> map = ring_map<N>();
    // tile t has nothing to add at this tap: every cell of it reads the zero row above / below or the zero column left / right
    __host__ __device__ static constexpr bool tap_dead(int t, int tap)
    {
        const int ky = tap / 3, kx = tap % 3;
        return (t == 0 && ky == 0) || (t == N - 1 && ky == 2) || (t == 1 && kx == 0) || (t == N - 2 && kx == 2);
    }
    __host__ __device__ static constexpr int live_pairs()
    {
        int v = 0;
        for (int t = 0; t < B::MT; t++) for (int tap = 0; tap < 9; tap++) v += tap_dead(t, tap) ? 0 : 1;
        return v;
    }
    static_assert(ring_cells_once(map), "every board cell is in exactly one tile lane");
    static_assert(ring_borders(map), "tiles 0, 14, 1, 13 hold only cells of row 0, row 14, column 0, column 14");
    static_assert(ring_conflicts(map, true) <= 1 && ring_conflicts(map, false) == 4, "at most one lane pair per tile shares a bank group, four in all");
    static_assert(ring_in_image(map), "every lane's 3x3 window lies inside the padded image; a junk lane repeats a tile-mate");
    static_assert(live_pairs() == 9 * B::MT - 12, "123 live (tile, tap) pairs per layer");
};
// the geometry trunk_group / k_trunk run on
template <int N>
using FusedGeo = std::conditional_t<N == 15, RingGeo<N>, NetGeo<N>>;


// Geometry of the ResidualBlock variant (BASELINE config 5; topology from the reference's historical checkpoints,
// SURVEY.md §8c): 64-channel stem + 3 residual blocks, 2/1-channel heads.  Two 64-channel packed images live in LDS.
template <int N>
struct ResGeo {
    static constexpr int n = N, nn = N * N, PW = N + 2, PP = PW * PW;
    static constexpr int G = pick_boards(N, 128, 39500);           // boards per workgroup (LDS: 2 x 64 channels)
    static constexpr int M = G * nn;
    static constexpr bool ROWT = (N == 15);
    static constexpr int MT = ROWT ? G * N : (M + 15) / 16, MR = MT * 16;
    static constexpr int CS = up16(G * PP);
    static constexpr int CS3 = CS;                                 // unused (no conv3-style overlay)
    static constexpr int LDSF = 128 * CS;
    static constexpr int RW = ((nn + 63) / 64) * 64;
    static constexpr int NW = N == 15 ? 12 : 8;                    // 4 channel tiles x {3,2} cell-tile groups: 15 = 3 x 5 tiles, no surplus
    static constexpr int PC = 2, VC = 1;
    static constexpr int NTP = (nn + 15) / 16;
    static constexpr int FROW = (((PC + VC) * nn + 3) / 4) * 4;
    static constexpr int QGP = fc_chain_groups(PC * nn), QGV = fc_chain_groups(VC * nn);
    static constexpr int QGMAX = QGP > QGV ? QGP : QGV;
    // LDS feature rows of the persistent search kernel (as NetGeo)
    static constexpr int VOFFL = 64 * QGP;
    static constexpr int FSTR0 = 64 * (QGP + QGV);
    static constexpr int FSTR = FSTR0 + ((4 - (FSTR0 % 32) + 32) % 32);
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// LDS activation image of a conv input with C >= 16 channels ("packed"): channel ci = 16*cg + 4*e + q lives at
//   float index  (((cg*4 + q) * CS + pos) * 4 + e)
// so that ONE ds_read_b128 at (cg, q, pos) delivers the B-operand values of four consecutive k-steps
// (e = 0..3) of lane group q, and the 16 lanes of a group read 256 contiguous bytes (conflict-free; CS % 16 == 0).
template <class GEO>
__device__ __forceinline__ int pk_index(int ci, int pos)
{
    return ((((ci >> 4) * 4 + (ci & 3)) * GEO::CS + pos) << 2) + ((ci >> 2) & 3);
}
enum { CONV_OUT_PACKED = 0, CONV_OUT3 = 1, CONV_OUT_RESIDUAL = 2,    // RESIDUAL: relu(acc + bias + out[same index]) in place
       CONV_OUT3_RESIDUAL = 3,     // relu(acc + bias + res[packed index]) into the [co][cell] tile (the last block of a tile-split ResidualBlock trunk)
       CONV_OUT3_CM = 4 };         // conv3 of the fused trunk: the output cell-major, float index m * OUT3_CM_STRIDE + co for tile cell m -- no
                                   // padding ring (a 1x1 conv reads it); a lane's four channels are ONE ds_write_b128, and four consecutive
                                   // channels of a cell ONE ds_read_b128 of the heads

// One conv layer on the workgroup's LDS image, computed as D[co][cell] = sum_k W[co][k] * X[k][cell]:
// the weight fragment is the MFMA A operand (row = output channel), the activation fragment the B operand
// (column = board cell), so an accumulator register holds 16 consecutive cells of one channel per 16 lanes.
// A wave owns one channel tile x MTW cell tiles.
// CIN == 4 (conv1) reads plain planes [ci][pos]; CIN >= 32 reads the packed image above.
// OUT3=false: relu(acc+bias) -> packed image of the next layer.  OUT3=true (conv3): barrier, then the
// [co][cell] image that overlays the (now dead) inputs.
// MTL / mt_base / mt_cnt: the tile-split kernels (k_tile) give one workgroup only the cell tiles mt_base .. mt_base + mt_cnt - 1
// (mt_cnt <= MTL); GO / out_pos_off: their packed output goes to an image of another geometry (the full board image in
// global memory) at positions shifted by out_pos_off; O3S: row stride of the [co][cell] output of CONV_OUT3, whose columns
// are counted from the workgroup's first tile.  The fused kernels use the defaults (all tiles, same geometry).
// The first weight fragments of a layer (the ones conv_layer asks for at its top), requested by the caller ahead of the layer.
// The persistent search kernel of the small boards does that one layer early: there a layer lasts 0.3-8 us, and the L2 round
// trip in front of its first MFMA was a visible part of it.  Same registers, same values: results cannot change.
template <int CIN>
struct ConvPre {
    static constexpr int NF = CIN == 4 ? 3 : CIN / 16;       // float4 fragments per channel tile: conv1's whole weights, one tap's otherwise
    float4 bw[NF];
};
template <class G, int CIN, int COUT>
__device__ __forceinline__ ConvPre<CIN> conv_prefetch(const float *__restrict__ wp, int wave, int lane)
{
    typedef ConvPre<CIN> P;
    constexpr int NG = COUT / 16;
    constexpr int KS4 = (9 * (CIN / 4) + 3) / 4;
    const int ng = wave % NG;
    P r;
    const float4 *w4 = reinterpret_cast<const float4 *>(wp) + (size_t)ng * KS4 * 64 + lane;
#pragma unroll
    for (int j = 0; j < P::NF; j++) r.bw[j] = w4[(size_t)j * 64];
    return r;
}

// Border tiles of a single-board geometry whose tiles lie along the borders (RingGeo, n = 15).  For the tile of row 0 the three
// taps with ky = 0 read nothing but the top padding row of the LDS image, for the tile of row n - 1 the three with ky = 2 nothing
// but the bottom one; likewise the tile of column 0 at the three taps with kx = 0 reads only the left padding column and the
// tile of column n - 1 at kx = 2 only the right one (its junk lanes repeat a cell of the same column).  The padding ring is zero
// by construction: conv_layer leaves those MFMAs (and fragment reads) out.  Which (tile, tap) pairs they are is the
// geometry's word (G::tap_dead).  Only a geometry that says so (BORDER_SKIP) is touched: NetGeo, the tile-split geometries
// (TileGeoT::A / B) and the persistent search kernel's have no such member and compile to the code they had.
// Exactness: for a finite weight fma(w, +0, acc) == acc bit for bit unless acc is -0 (then +0).  A -0 accumulator can only
// come from a real product that underflowed, and the layer's output erases its sign in both variants: acc + bias, then
// v > 0 ? v : +0 (the residual paths likewise), so every layer output keeps its bits.  With a non-finite weight the full chain
// made NaN on the border cells where the oracle (conv3x3_core: out-of-board taps skipped) does not: the skip is the definition.
// Which tile and lane computes an output element does not enter: it is the same k-ordered chain over the same 3x3 window.
template <class G, class = void>
struct BorderSkip { static constexpr bool value = false; };
template <class G>
struct BorderSkip<G, std::void_t<decltype(G::BORDER_SKIP)>> { static constexpr bool value = G::BORDER_SKIP; };

// tile i of cell-tile group mgc (tile mgc + i * MG of the geometry) has nothing to add at this tap
template <bool SKIP, class G, int MG>
__host__ __device__ constexpr bool border_dead(int mgc, int i, int tap)
{
    if constexpr (SKIP) return G::tap_dead(mgc + i * MG, tap);
    else return false;
}
template <bool SKIP, class G, int MG>
__host__ __device__ constexpr int border_live(int mgc, int mtw, int tap)
{
    int c = 0;
    for (int i = 0; i < mtw; i++) c += border_dead<SKIP, G, MG>(mgc, i, tap) ? 0 : 1;
    return c;
}

// Runs body(cell tiles of the wave's cell-tile group, the group) with BOTH as compile-time values: one body per group.
template <int K, int MG, int MT_FULL, int MT_REM, class B>
__device__ __forceinline__ void conv_by_group(int mg, B &body)
{
    constexpr int MTW = MT_FULL + (K < MT_REM ? 1 : 0);
    if constexpr (K + 1 == MG) body(std::integral_constant<int, MTW>{}, std::integral_constant<int, K>{});
    else if (mg == K) body(std::integral_constant<int, MTW>{}, std::integral_constant<int, K>{});
    else conv_by_group<K + 1, MG, MT_FULL, MT_REM>(mg, body);
}

template <class G, int CIN, int COUT, int MODE, int MTL = G::MT, class GO = G, int O3S = G::CS3>
__device__ __forceinline__ void conv_layer(const float *in, float *out, const float *__restrict__ wp,
                                           const float *__restrict__ bias, const unsigned short *wpos,
                                           const unsigned short *cellof, int wave, int lane,
                                           int mt_base = 0, int mt_cnt = MTL, int out_pos_off = 0, const float *res = nullptr,
                                           unsigned long long *lst = nullptr, const ConvPre<CIN> *pre = nullptr)
{
    // diagnostic builds only (-DAZ_STAMPS): per-wave time stamps of a layer's phases into lst[wave * 4 + k]
#ifdef AZ_STAMPS
#define AZ_LSTAMP(k) do { if (lst && lane == 0) lst[wave * 4 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define AZ_LSTAMP(k) do { } while (0)
#endif
    constexpr bool OUT3 = MODE == CONV_OUT3 || MODE == CONV_OUT3_RESIDUAL || MODE == CONV_OUT3_CM;
    constexpr bool SUBSET = MTL < G::MT;                       // a tile-split kernel: waves without a tile skip the layer
    constexpr int NG = COUT / 16;                              // channel tiles
    constexpr int MG = (G::NW / NG) > 0 ? (G::NW / NG) : 1;    // cell-tile groups
    // cell tiles per wave: the first MTL % MG cell-tile groups take one more than the others.  The layer's body is
    // instantiated for both counts and a wave runs the one that is its own (until round 3 every wave ran the larger count and
    // threw the surplus tile away: 16 instead of 15 tile chains per SIMD in conv2 at n = 15).
    constexpr int MT_FULL = MTL / MG, MT_REM = MTL % MG;
    constexpr int KST = CIN / 4;           // k-steps per tap
    constexpr int KS = 9 * KST;
    constexpr int KS4 = (KS + 3) / 4;
    const int ng = wave % NG, mg = wave / NG;       // wave is wave-uniform (readfirstlane) -> scalar control flow
    const int q = lane >> 4, r16 = lane & 15;
    // border tiles (BorderSkip above): the packed-input layers of a fused kernel whose geometry names dead taps; the cell-tile
    // group is then a compile-time value of the body (MGC), so that G::tap_dead(tile, tap) folds away in the unrolled tap loop
    constexpr bool SKIP = BorderSkip<G>::value && !SUBSET && CIN >= 32;

    auto body = [&](auto mtw_c, auto mg_c) __attribute__((always_inline)) {
    constexpr int MTW = decltype(mtw_c)::value;
    constexpr int MGC = decltype(mg_c)::value;      // the wave's cell-tile group where SKIP, else unused
    if constexpr (MTW == 0) {
        if constexpr (OUT3) __syncthreads();       // a wave without a tile still meets the layer's barrier
    } else {
    AZ_LSTAMP(0);
    f32x4 acc[MTW];
#pragma unroll
    for (int i = 0; i < MTW; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float4 *wp4 = reinterpret_cast<const float4 *>(wp) + (size_t)ng * KS4 * 64 + lane;
    // the epilogue's biases are requested before the main loop, so that their L2 round trip is not paid between two layers
    float bias_pre[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) bias_pre[rg] = bias[ng * 16 + q * 4 + rg];
    if (!SUBSET || mg < mt_cnt) {
    if constexpr (CIN == 4) {
        // conv1: 9 k-steps (one per tap), channels = {mover, opponent, last move, zero plane}, planes [ci][pos]
        int rb[MTW];
#pragma unroll
        for (int i = 0; i < MTW; i++) {
            int mt = mg + i * MG;
            int m = (mt_base + (mt < mt_cnt ? mt : 0)) * 16 + r16;       // a surplus tile aliases the first one (computed, never written back)
            rb[i] = (int)wpos[m] - (G::PW + 1) + q * G::CS;
        }
        float4 b0, b1, b2;
        if (pre) { b0 = pre->bw[0]; b1 = pre->bw[1]; b2 = pre->bw[2]; }
        else { b0 = wp4[0]; b1 = wp4[64]; b2 = wp4[128]; }
        const float bk[12] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int toff = (tap / 3) * G::PW + (tap % 3);
#pragma unroll
            for (int i = 0; i < MTW; i++) {
                const float a = in[rb[i] + toff];
                acc[i] = mfma4(bk[tap], a, acc[i]);
            }
        }
    } else {
        constexpr int NQ = KST / 4;        // weight groups (= 16-channel groups) per tap: 2 for conv2, 4 for conv3
        // Software pipeline pinned with sched_group_barrier: while the 4*MTW MFMAs of group g issue, the MTW
        // ds_read_b128 of group g+1 are interleaved between them; the weight fragments of tap t+1 are fetched (L2)
        // at the top of tap t.
        const float4 *in4 = reinterpret_cast<const float4 *>(in);
        int ra[MTW];                       // running float4 index: (cg*4 + q)*CS + top-left position of the window
#pragma unroll
        for (int i = 0; i < MTW; i++) {
            int mt = mg + i * MG;
            int m = (mt_base + (mt < mt_cnt ? mt : 0)) * 16 + r16;
            ra[i] = (int)wpos[m] - (G::PW + 1) + q * G::CS;
        }
        float4 a0[MTW], a1[MTW];
        float4 bw[NQ], bnx[NQ];
        const int prio_turn = (wave >> 2) % (G::NW / 4);        // scalar: which of the waves sharing a SIMD this one is
#pragma unroll
        for (int j = 0; j < NQ; j++) bw[j] = pre ? pre->bw[j] : wp4[(size_t)j * 64];
#pragma unroll
        for (int i = 0; i < MTW; i++)
            if (!border_dead<SKIP, G, MG>(MGC, i, 0)) a0[i] = in4[ra[i]];
        // The nine taps unrolled, so that every fragment address is the tile's base register + a constant (the ds_read's
        // 16-bit immediate: at most ((NQ - 1) 4 CS + 2 PW + 2) x 16 B = 58.9 KB at n = 15) and the weight registers of
        // consecutive taps are renamed instead of copied.  The rolled loop kept a running index per tile and recomputed
        // the bases every tap: 0.82 vector instructions per MFMA in conv3 -- and the float32 MFMA leaves the SIMD's vector
        // issue so little room that those showed one for one: 35.2 cycles per MFMA instead of 32 (measured with the LDS
        // reads AND the weight fetches taken out: still 35).
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int tn = tap + 1 < 9 ? tap + 1 : tap;
#pragma unroll
            for (int j = 0; j < NQ; j++) bnx[j] = wp4[(size_t)(tn * NQ + j) * 64];
#pragma unroll
            for (int sq = 0; sq < NQ; sq++) {
                // The waves that share a SIMD (w, w + 4, ...) run the same program; left alone, one of them wins the issue
                // arbitration every time, finishes the layer early and leaves its partner to run the rest alone -- and ONE
                // wave issues an MFMA only every ~44 cycles (measured: conv3 at n = 15, waves 4-7 done after 102.6 k cycles,
                // waves 0-3 after 151.6 k; the matrix pipe needs 138.2 k).  Taking turns with the priority, tap by tap, keeps
                // them level, so that the pipe has two streams to draw from until the end.
                if (sq == 0) {
                    if ((tap % (G::NW / 4)) == prio_turn) __builtin_amdgcn_s_setprio(1);
                    else __builtin_amdgcn_s_setprio(0);
                }
                float4 *cur = (sq & 1) ? a1 : a0;
                float4 *nxt = (sq & 1) ? a0 : a1;
                // float4 offset of the NEXT group's fragments from the tile's base: next 16-channel group of this tap, or the
                // first group of the next tap (the last group of all reads its own again: never used)
                const int gtap = sq + 1 < NQ ? tap : tn, gsq = sq + 1 < NQ ? sq + 1 : (tap + 1 < 9 ? 0 : sq);
                const int noff = gsq * 4 * G::CS + (gtap / 3) * G::PW + (gtap % 3);
                // a border tile neither reads nor multiplies the fragments of its zero row or column
#pragma unroll
                for (int i = 0; i < MTW; i++)
                    if (!border_dead<SKIP, G, MG>(MGC, i, gtap)) nxt[i] = in4[ra[i] + noff];
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < MTW; i++) {
                        if (border_dead<SKIP, G, MG>(MGC, i, tap)) continue;
                        const float4 wv = bw[sq];
                        const float we = e == 0 ? wv.x : e == 1 ? wv.y : e == 2 ? wv.z : wv.w;
                        const float ae = e == 0 ? cur[i].x : e == 1 ? cur[i].y : e == 2 ? cur[i].z : cur[i].w;
                        acc[i] = mfma4(we, ae, acc[i]);
                    }
                // one read after the four MFMAs of a tile; where this group and the next differ in live tiles (with the ring
                // tiling at every change of tap), the surplus reads follow the last MFMAs, surplus MFMAs go without a read
                const int nm = border_live<SKIP, G, MG>(MGC, MTW, tap);
                const int nr = border_live<SKIP, G, MG>(MGC, MTW, gtap);
#pragma unroll
                for (int i = 0; i < MTW; i++) {
                    if (i < nm) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);         // 4 MFMAs
                    if (i < nr) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);         // 1 LDS read (b128)
                }
            }
#pragma unroll
            for (int j = 0; j < NQ; j++) bw[j] = bnx[j];
        }
        __builtin_amdgcn_s_setprio(0);
    }
    }
    AZ_LSTAMP(1);
    if constexpr (OUT3) __syncthreads();   // every wave has finished reading the conv3 input image
    AZ_LSTAMP(2);
    float bco[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) bco[rg] = bias_pre[rg];
#pragma unroll
    for (int i = 0; i < MTW; i++) {
        const int mt = mg + i * MG;
        if (mt < mt_cnt) {
            const int m = (mt_base + mt) * 16 + r16;
            const bool valid = cellof[m] != 0xFFFFu;
            const int pos = (int)wpos[m] + out_pos_off;
            if constexpr (MODE == CONV_OUT3_CM) {
                // the lane's registers are channels 16 ng + 4 q + 0..3 of cell m: 16 contiguous bytes of the cell's row
                float4 v4;
                v4.x = acc[i][0] + bco[0]; v4.y = acc[i][1] + bco[1]; v4.z = acc[i][2] + bco[2]; v4.w = acc[i][3] + bco[3];
                v4.x = v4.x > 0.0f ? v4.x : 0.0f; v4.y = v4.y > 0.0f ? v4.y : 0.0f;
                v4.z = v4.z > 0.0f ? v4.z : 0.0f; v4.w = v4.w > 0.0f ? v4.w : 0.0f;
                *reinterpret_cast<float4 *>(out + m * OUT3_CM_STRIDE + ng * 16 + q * 4) = v4;
            } else
#pragma unroll
            for (int rg = 0; rg < 4; rg++) {
                const int co = ng * 16 + q * 4 + rg;      // = 16*cg + 4*e + q' with cg = ng, e = q, q' = rg
                float v = acc[i][rg] + bco[rg];
                v = v > 0.0f ? v : 0.0f;
                if constexpr (MODE == CONV_OUT3_RESIDUAL) {
                    float r = acc[i][rg] + bco[rg] + (valid ? res[pk_index<GO>(co, pos)] : 0.0f);
                    out[co * O3S + mt * 16 + r16 + (SUBSET ? 0 : mt_base * 16)] = r > 0.0f ? r : 0.0f;
                } else if constexpr (OUT3) out[co * O3S + mt * 16 + r16 + (SUBSET ? 0 : mt_base * 16)] = v;
                else if constexpr (MODE == CONV_OUT_RESIDUAL) {
                    if (valid) {                          // net block: relu(bn2(conv2(h)) + x), x updated in place
                        const int oi = pk_index<GO>(co, pos);
                        float r = acc[i][rg] + bco[rg] + out[oi];
                        out[oi] = r > 0.0f ? r : 0.0f;
                    }
                } else if (valid) out[pk_index<GO>(co, pos)] = v;
            }
        }
    }
    AZ_LSTAMP(3);
    }
    };
    typedef std::integral_constant<int, -1> any_group;
    if constexpr (SKIP) conv_by_group<0, MG, MT_FULL, MT_REM>(mg, body);
    else if constexpr (MT_REM == 0) body(std::integral_constant<int, MT_FULL>{}, any_group{});
    else if (mg < MT_REM) body(std::integral_constant<int, MT_FULL + 1>{}, any_group{});
    else body(std::integral_constant<int, MT_FULL>{}, any_group{});
}

// policy_conv (128->4) and value_conv (128->2), 1x1 (net.py:64,69) of the fused trunk, on v_mfma_f32_4x4x1_16b_f32: 16 independent
// 4x4 outer products (blocks) with K = 1.  Block b of a wave is lanes 4b .. 4b + 3: its channel half is b & 1 (head rows 0-3
// policy_conv, 4-5 value_conv, 6-7 zero weights) and its cell quad b >> 1, so one instruction adds ONE input channel to 8 head
// rows x 32 tile cells, and wave w owns tile cells 32 w .. 32 w + 31.  Lane 4b + i supplies A = the weight of head row
// 4 (b & 1) + i, lane 4b + j supplies B = out3[cell 4 (b >> 1) + j][k], and register i of lane 4b + j receives head row
// 4 (b & 1) + i of that cell.  k runs 0..127 in program order on one accumulator from +0: the chain the 16x16x4 tiles computed
// (16 s4 + 4 e + q ascending), bit for bit.  hdq_lds: the block-ordered weights (NetWeights::hdq) staged in LDS by the prologue;
// out3: the cell-major conv3 image (CONV_OUT3_CM).  One ds_read_b128 of each feeds four MFMAs.
template <class G>
__device__ __forceinline__ void trunk_heads(const DevState &d, const NetWeights &w, int net_id, float *__restrict__ feat,
                                            const float *out3, const float *hdq_lds, const unsigned short *cellof, int b0, int wave, int lane)
{
    static_assert(G::MR <= G::NW * 32, "one group of 32 tile cells per wave");
    static_assert(G::NW * 64 * 2 == 32 * 8 * 4, "trunk_group stages the block-ordered head weights with one float2 per thread");
    const int half = (lane >> 2) & 1;
    const int m = wave * 32 + (lane >> 3) * 4 + (lane & 3);        // the lane's tile cell; past the image: cell 0 again, computed and dropped
    float hb[4];
#pragma unroll
    for (int i = 0; i < 4; i++) hb[i] = (half * 4 + i) < 6 ? w.hdb[half * 4 + i] : 0.0f;
    const float4 *ap = reinterpret_cast<const float4 *>(hdq_lds) + (lane & 7);
    const float4 *bp = reinterpret_cast<const float4 *>(out3 + (m < G::MR ? m : 0) * OUT3_CM_STRIDE);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k4 = 0; k4 < 32; k4++) {
        const float4 a = ap[k4 * 8], b = bp[k4];
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.w, b.w, acc, 0, 0, 0);
    }
    if (m < G::MR) {
        const int cell = cellof[m];
        if (cell != 0xFFFF) {
            const int g = cell / G::nn, p = cell - g * G::nn;
            const int b = b0 + g;
            if (b < d.B && d.s_net[b] == net_id) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int j = half * 4 + i;       // head channel: 0-3 policy_conv, 4-5 value_conv (net.py:64,69 flatten order)
                    if (j < 6) {
                        float v = acc[i] + hb[i];
                        feat[(size_t)b * G::FROW + j * G::nn + p] = v > 0.0f ? v : 0.0f;
                    }
                }
            }
        }
    }
}

// The work of one board group: one k_trunk workgroup (several groups per workgroup measured the same).
template <int N>
__device__ __forceinline__ void trunk_group(const DevState &d, const NetWeights &w, int net_id, float *__restrict__ feat,
                                                      unsigned long long *dbg, int grp, float *lds, float *hdq_lds, unsigned short *wpos,
                                                      unsigned short *cellof, int *any_active_p, int tid)
{
    typedef FusedGeo<N> G;
    constexpr bool RING = BorderSkip<G>::value;       // the tile tables come from G::map
    int &any_active = *any_active_p;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = grp * G::G;
    AZ_STAMP(0);
    // the head weights in block order (4 KB, 8 bytes per thread): asked for first of all, so that they arrive with the leaf words
    // requested below, and put into LDS in front of the zero fill; read by trunk_heads only
    const float2 hq = reinterpret_cast<const float2 *>(w.hdq)[tid];
    // ring tiling: the thread's entry of the tile map (960 B of constant data, in L2 after the first workgroups), asked for with
    // the head weights and stored with them
    unsigned short map_pos = 0, map_cell = 0xFFFF;
    if constexpr (RING) {
        if (tid < G::MR) { map_pos = G::map.pos[tid]; map_cell = G::map.cell[tid]; }
    }
    if (tid == 0) any_active = 0;
    __syncthreads();
    if (tid < G::G) {
        int b = b0 + tid;
        if (b < d.B) {
            int kind = d.leaf_kind[b];
            if ((kind == LEAF_ROOT || kind == LEAF_EXPAND) && d.s_status[b] == SLOT_ACTIVE && d.s_net[b] == net_id)
                atomicOr(&any_active, 1);
        }
    }
    float *inA = lds;                  // 32 channels (conv1 out / conv2 in)
    float *inB = lds + 32 * G::CS;     // 64 channels (conv2 out / conv3 in); first 4 channels hold the input planes
    // Every thread requests the leaf words of its cells (games.py:86-129 encode: ch0 = side to move, ch1 = opponent, ch2 = last
    // action, ch3 = zeros) before it is known whether the group has anything to evaluate: the loads are in flight while both
    // padded images are zeroed (the padding ring must read as 0).
    constexpr int EPT = (G::MR + G::NW * 64 - 1) / (G::NW * 64);
    int e_pos[EPT];
    bool e_me[EPT], e_op[EPT], e_last[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int m = tid + e * G::NW * 64;
        int pos = G::PW + 1, cell = 0xFFFF;
        if constexpr (RING) {
            // thread m encodes board CELL m, whichever tile lane reads it later: its leaf words do not wait for the map
            static_assert(EPT == 1 && G::G == 1, "one tile lane per thread, one board");
            if (m < G::nn) {
                const int r = m / N, c = m - r * N;
                pos = (r + 1) * G::PW + (c + 1);
                cell = m;
            }
        } else if (m < G::MR) {
            if constexpr (G::ROWT) {
                const int t = m >> 4, c = m & 15, g = t / N, r = t - g * N;
                pos = g * G::PP + (r + 1) * G::PW + (c + 1);                 // c == N is the right padding cell of the row
                cell = c < N ? g * G::nn + r * N + c : 0xFFFF;
            } else {
                const int g = m / G::nn, p = m - g * G::nn, r = p / N, c = p - r * N;
                pos = m < G::M ? g * G::PP + (r + 1) * G::PW + (c + 1) : G::PW + 1;
                cell = m < G::M ? m : 0xFFFF;
            }
            wpos[m] = (unsigned short)pos;
            cellof[m] = (unsigned short)cell;
        }
        e_pos[e] = pos;
        e_me[e] = e_op[e] = e_last[e] = false;
        if (cell != 0xFFFF) {
            const int g = cell / G::nn, p = cell - g * G::nn;
            const int b = b0 + g;
            if (b < d.B) {
                const u64 *lf = d.leaf + (size_t)b * 8;
                const int ps = sym_cell(d.leaf_sym, b, p, N);
                e_me[e] = (lf[ps >> 6] >> (ps & 63)) & 1ull;
                e_op[e] = (lf[4 + (ps >> 6)] >> (ps & 63)) & 1ull;
                e_last[e] = d.leaf_last[b] == ps;
            }
        }
    }
    reinterpret_cast<float2 *>(hdq_lds)[tid] = hq;       // in front of the zero fill, whose writes cover this one's latency
    if constexpr (RING) {
        if (tid < G::MR) { wpos[tid] = map_pos; cellof[tid] = map_cell; }
    }
    {
        float4 *z = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < (96 * G::CS) / 4; i += G::NW * 64) z[i] = float4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    if (!any_active) return;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        if (e_me[e]) inB[e_pos[e]] = 1.0f;
        if (e_op[e]) inB[G::CS + e_pos[e]] = 1.0f;
        if (e_last[e]) inB[2 * G::CS + e_pos[e]] = 1.0f;
    }
    __syncthreads();
    AZ_STAMP(1);
    conv_layer<G, 4, 32, CONV_OUT_PACKED>(inB, inA, w.c1, w.c1b, wpos, cellof, wave, lane);
    __syncthreads();
    // the input planes lived in the first 3 planes of inB; clear them before conv2's packed output lands there
    // (in packed coordinates some of those floats are padding-ring cells that conv2 never writes)
    for (int i = tid; i < 3 * G::CS; i += G::NW * 64) inB[i] = 0.0f;
    __syncthreads();
    AZ_STAMP(2);
    conv_layer<G, 32, 64, CONV_OUT_PACKED>(inA, inB, w.c2, w.c2b, wpos, cellof, wave, lane);
    __syncthreads();
    AZ_STAMP(3);
#ifdef AZ_STAMPS
    unsigned long long *lst3 = dbg ? dbg + (size_t)d.B * 16 + 4096 * 32 + (size_t)grp * 32 : nullptr;      // behind k_fc's stamps
#else
    unsigned long long *lst3 = nullptr;
#endif
    conv_layer<G, 64, 128, CONV_OUT3_CM>(inB, lds, w.c3, w.c3b, wpos, cellof, wave, lane, 0, G::MT, 0, nullptr, lst3);
    __syncthreads();
    AZ_STAMP(4);
    trunk_heads<G>(d, w, net_id, feat, lds, hdq_lds, cellof, b0, wave, lane);
    AZ_STAMP(5);
}

template <int N>
__global__ __launch_bounds__(NetGeo<N>::NW * 64) void k_trunk(DevState d, NetWeights w, int net_id, float *__restrict__ feat,
                                               unsigned long long *dbg)
{
    typedef FusedGeo<N> G;                    // n = 15: the ring tiling; sizes, waves and LDS are NetGeo<N>'s
    __shared__ __attribute__((aligned(16))) float lds[G::LDSF];
    __shared__ __attribute__((aligned(16))) float hdq_lds[1024];     // head-conv weights in block order, [k/4][8 rows][4]
    __shared__ unsigned short wpos[G::MR];     // centre position of tile cell m in the padded image
    __shared__ unsigned short cellof[G::MR];   // g*nn + cell index, 0xFFFF for a junk lane
    __shared__ int any_active;
    const int ngroups = (d.B + G::G - 1) / G::G;
    // One board group per workgroup.  The body stays inside a one-trip loop on purpose: the compiler schedules trunk_group
    // differently without the loop (at n = 15, 34 more instructions, 23 more VALU between the MFMAs of conv1, conv2 and the
    // heads), and the loop form is the code every measurement in DESIGN.md was taken on.
#pragma unroll 1
    for (int it = 0; it < 1; it++) {
        const int grp = blockIdx.x + it;
        if (grp >= ngroups) break;
        int tid = threadIdx.x;
        trunk_group<N>(d, w, net_id, feat, dbg, grp, lds, hdq_lds, wpos, cellof, &any_active, tid);
    }
}

// ------------------------------------------------------------------------------------------------
// Tile-split trunk (GomokuNet): the low-latency path for launches with few pending boards (episode tails, the arena,
// single-position search).  The fused k_trunk keeps a board on ONE CU (~95 us of paced MFMAs at n = 15); here a board is
// spread over workgroups by CELL tiles (one 16-cell MFMA tile = one board row at n = 15):
//   stage A  grid (groups, MT): encode the rows around tile t, conv1 on the <= 4 tiles conv2 needs (recomputed per
//            workgroup: 9 k-steps), conv2 on tile t (4 waves x 72 MFMAs)        -> img2, the packed 64-channel board image
//   stage B  grid (groups, MT): the rows of img2 around tile t -> conv3 on tile t (8 waves x 144 MFMAs: all 128 channels of
//            the tile's cells are in THIS workgroup) -> 1x1 heads of the tile (32 MFMAs) -> feature rows
// img2 crosses HBM/L2 in scratch, one image per board group (padding ring zeroed once at allocation, never written); 16-24 KB
// of LDS per workgroup (several per CU).  Every output element is the same k-ordered fma chain as in k_trunk -- which
// workgroup computes it does not enter -- so the results are bit-identical.
// ------------------------------------------------------------------------------------------------
template <class F, int NWT>
struct TileGeoT {
    static constexpr int N = F::n, PW = F::PW, PP = F::PP, MT = F::MT, nn = F::nn, M = F::M;
    // padded-image position of tile lane m (the centre of its 3x3 window), -1 for a lane without a cell to compute
    __host__ __device__ static constexpr int centre(int m)
    {
        if (F::ROWT) {
            const int t = m >> 4, c = m & 15, g = t / N, r = t - g * N;
            return g * PP + (r + 1) * PW + (c + 1);          // c == N: the row's right padding cell (computed, never stored)
        }
        if (m >= M) return -1;
        const int g = m / nn, p = m - g * nn, r = p / N, c = p - r * N;
        return g * PP + (r + 1) * PW + (c + 1);
    }
    __host__ __device__ static constexpr int lo_of(int t)
    {
        int v = 1 << 30;
        for (int i = 0; i < 16; i++) { const int c = centre(16 * t + i); if (c >= 0 && c < v) v = c; }
        return v;
    }
    __host__ __device__ static constexpr int hi_of(int t)
    {
        int v = -1;
        for (int i = 0; i < 16; i++) { const int c = centre(16 * t + i); if (c > v) v = c; }
        return v;
    }
    // first-conv tiles stage A computes for tile t: every tile with a cell next to a cell of t (same board group)
    __host__ __device__ static constexpr int c1_lo(int t)
    {
        if (F::ROWT) return (t % N) > 0 ? t - 1 : t;
        const int a = 16 * t - (N + 1);
        return a < 0 ? 0 : a >> 4;
    }
    __host__ __device__ static constexpr int c1_hi(int t)
    {
        if (F::ROWT) return (t % N) < N - 1 ? t + 1 : t;
        const int b = (16 * t + 15 + N + 1) >> 4;
        return b > MT - 1 ? MT - 1 : b;
    }
    // origins (first padded-image position held in LDS) and extents of the two kinds of image
    __host__ __device__ static constexpr int org_b(int t) { return lo_of(t) - (PW + 1); }
    __host__ __device__ static constexpr int org_a(int t) { return lo_of(c1_lo(t)) - (PW + 1); }
    __host__ __device__ static constexpr int span_b()
    {
        int v = 0;
        for (int t = 0; t < MT; t++) { const int e = hi_of(t) + (PW + 1) - org_b(t) + 1; if (e > v) v = e; }
        return v;
    }
    __host__ __device__ static constexpr int span_a()
    {
        int v = 0;
        for (int t = 0; t < MT; t++) { const int e = hi_of(c1_hi(t)) + (PW + 1) - org_a(t) + 1; if (e > v) v = e; }
        return v;
    }
    __host__ __device__ static constexpr int c1_tiles()
    {
        int v = 0;
        for (int t = 0; t < MT; t++) { const int e = c1_hi(t) - c1_lo(t) + 1; if (e > v) v = e; }
        return v;
    }
    static constexpr int CSA = ((span_a() + 15) / 16) * 16, CSB = ((span_b() + 15) / 16) * 16;   // plane strides: multiples of 16 (conflict-free b128 reads)
    static constexpr int MTL1 = c1_tiles();
    static_assert(MTL1 <= 4, "stage A covers the first conv with at most 4 cell tiles per channel tile");
    // what conv_layer sees of the geometry in each stage: the full board's tiling, the local image's stride
    struct A { static constexpr int NW = NWT, MT = F::MT, PW = F::PW, CS = CSA, CS3 = 16; };
    struct B { static constexpr int NW = NWT, MT = F::MT, PW = F::PW, CS = CSB, CS3 = 16; };

    // relative-position tables of one workgroup (origin org, image stride csl) + the group's activity flag; false = nothing to do
    __device__ static __forceinline__ bool prologue(const DevState &d, int net_id, int b0, int org, int csl, unsigned short *wpos,
                                                    unsigned short *cellof, int *any_active, int tid, int nth)
    {
        if (tid == 0) *any_active = 0;
        __syncthreads();
        if (tid < F::G) {
            const int b = b0 + tid;
            if (b < d.B) {
                const int kind = d.leaf_kind[b];
                if ((kind == LEAF_ROOT || kind == LEAF_EXPAND) && d.s_status[b] == SLOT_ACTIVE && d.s_net[b] == net_id)
                    atomicOr(any_active, 1);
            }
        }
        for (int m = tid; m < F::MR; m += nth) {
            const int c = centre(m);
            int cell = 0xFFFF;
            if (c >= 0) {
                if constexpr (F::ROWT) { if ((m & 15) < N) cell = (m >> 4) * N + (m & 15); }
                else cell = m;
            }
            const int rel = c - org;
            // lanes outside this workgroup's image (other tiles, junk lanes) get a harmless in-range position: they are
            // either never used or computed and thrown away
            wpos[m] = (unsigned short)((c >= 0 && rel >= PW + 1 && rel + PW + 1 < csl) ? rel : PW + 1);
            cellof[m] = (unsigned short)cell;
        }
        __syncthreads();
        return *any_active != 0;
    }
    // games.py:86-129 encode of the cells inside an image of stride csl starting at org: planes [mover | opponent | last move | 0]
    __device__ static __forceinline__ void encode(const DevState &d, int b0, int org, int csl, float *planes, const unsigned short *cellof,
                                                  int tid, int nth)
    {
        for (int m = tid; m < F::MR; m += nth) {
            const int cell = cellof[m];
            const int rel = centre(m) - org;
            if (cell != 0xFFFF && rel >= 0 && rel < csl) {
                const int g = cell / nn, p = cell - g * nn;
                const int b = b0 + g;
                if (b < d.B) {
                    const u64 *lf = d.leaf + (size_t)b * 8;
                    const int ps = sym_cell(d.leaf_sym, b, p, N);
                    if ((lf[ps >> 6] >> (ps & 63)) & 1ull) planes[rel] = 1.0f;
                    if ((lf[4 + (ps >> 6)] >> (ps & 63)) & 1ull) planes[csl + rel] = 1.0f;
                    if (d.leaf_last[b] == ps) planes[2 * csl + rel] = 1.0f;
                }
            }
        }
    }
    // the positions org .. org + CSB of the 16 planes (cg, q) of a packed 64-channel board image (stride F::CS) into LDS
    __device__ static __forceinline__ void load_rows(const float *img, int org, float *lds, int tid, int nth)
    {
        const float4 *src = reinterpret_cast<const float4 *>(img);
        float4 *dst = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < 16 * CSB; i += nth) {
            const int plane = i / CSB, rel = i - plane * CSB, pos = org + rel;
            dst[i] = (pos >= 0 && pos < F::CS) ? src[plane * F::CS + pos] : float4{0.f, 0.f, 0.f, 0.f};
        }
    }
};
template <int N>
struct TileGeo : TileGeoT<NetGeo<N>, NetGeo<N>::NW> {
    typedef TileGeoT<NetGeo<N>, NetGeo<N>::NW> T;
    static constexpr int LDSA = 36 * T::CSA, LDSB = 64 * T::CSB + 128 * 16;
    static constexpr int SCRATCH = 64 * NetGeo<N>::CS;        // floats of scratch per board group: img2
};

template <int N, int STAGE>
__global__ __launch_bounds__(NetGeo<N>::NW * 64) void k_tile(DevState d, NetWeights w, int net_id, float *__restrict__ scratch,
                                                     float *__restrict__ feat)
{
    typedef NetGeo<N> F;
    typedef TileGeo<N> TG;
    constexpr int NTH = F::NW * 64;
    __shared__ __attribute__((aligned(16))) float lds[STAGE == 1 ? TG::LDSA : TG::LDSB];
    __shared__ unsigned short wpos[F::MR];      // centre of tile lane m RELATIVE to this workgroup's image origin
    __shared__ unsigned short cellof[F::MR];
    __shared__ int any_active;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = blockIdx.x, t = blockIdx.y, b0 = grp * F::G;
    const int org = STAGE == 1 ? TG::org_a(t) : TG::org_b(t);
    if constexpr (STAGE == 1) {
        float4 *z = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < TG::LDSA / 4; i += NTH) z[i] = float4{0.f, 0.f, 0.f, 0.f};
    }
    if (!TG::prologue(d, net_id, b0, org, STAGE == 1 ? TG::CSA : TG::CSB, wpos, cellof, &any_active, tid, NTH)) return;
    float *img2 = scratch + (size_t)grp * TG::SCRATCH;      // the packed 64-channel board image (padding ring zeroed once)
    if constexpr (STAGE == 1) {
        float *planes = lds, *img1 = lds + 4 * TG::CSA;
        TG::encode(d, b0, org, TG::CSA, planes, cellof, tid, NTH);
        __syncthreads();
        const int tlo = TG::c1_lo(t), cnt = TG::c1_hi(t) - tlo + 1;
        conv_layer<typename TG::A, 4, 32, CONV_OUT_PACKED, TG::MTL1>(planes, img1, w.c1, w.c1b, wpos, cellof, wave, lane, tlo, cnt);
        __syncthreads();
        conv_layer<typename TG::A, 32, 64, CONV_OUT_PACKED, 1, F>(img1, img2, w.c2, w.c2b, wpos, cellof, wave, lane, t, 1, org);
    } else {
        TG::load_rows(img2, org, lds, tid, NTH);              // the rows of the conv2 image this tile's windows touch
        __syncthreads();
        float *out3 = lds + 64 * TG::CSB;                     // [co][16 cells of the tile]
        conv_layer<typename TG::B, 64, 128, CONV_OUT3, 1, typename TG::B, 16>(lds, out3, w.c3, w.c3b, wpos, cellof, wave, lane, t, 1);
        __syncthreads();
        if (wave == 0) {                                      // policy_conv (128->4) and value_conv (128->2) of the tile's cells
            const int q = lane >> 4, r16 = lane & 15;
            const float4 *wp4 = reinterpret_cast<const float4 *>(w.hd) + lane;
            float hb[4];
#pragma unroll
            for (int rg = 0; rg < 4; rg++) hb[rg] = (q * 4 + rg) < 6 ? w.hdb[q * 4 + rg] : 0.0f;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *ip = out3 + q * 16 + r16;
#pragma unroll
            for (int s4 = 0; s4 < 8; s4++) {
                const float4 bq = wp4[s4 * 64];
                acc = mfma4(bq.x, ip[(s4 * 16 + 0) * 16], acc);
                acc = mfma4(bq.y, ip[(s4 * 16 + 4) * 16], acc);
                acc = mfma4(bq.z, ip[(s4 * 16 + 8) * 16], acc);
                acc = mfma4(bq.w, ip[(s4 * 16 + 12) * 16], acc);
            }
            const int cell = cellof[t * 16 + r16];
            if (cell != 0xFFFF) {
                const int g = cell / F::nn, p = cell - g * F::nn;
                const int b = b0 + g;
                if (b < d.B && d.s_net[b] == net_id) {
#pragma unroll
                    for (int rg = 0; rg < 4; rg++) {
                        const int j = q * 4 + rg;
                        if (j < 6) {
                            float v = acc[rg] + hb[rg];
                            feat[(size_t)b * F::FROW + j * F::nn + p] = v > 0.0f ? v : 0.0f;
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// ResidualBlock variant: stem conv(4->64)+BN+ReLU, 3 x {conv+BN+ReLU, conv+BN, +skip, ReLU}, 1x1 heads (2 policy
// channels, 1 value channel) + BN + ReLU.  Eval-mode BatchNorm is folded into the conv weights/biases by the host
// layer.  Two 64-channel packed images in LDS: A holds the block input/output (updated in place by the skip add),
// B the intermediate.
// ------------------------------------------------------------------------------------------------
struct ResWeights {
    const float *stem, *stemb;
    const float *blk[6], *blkb[6];     // res1.conv1, res1.conv2, res2.conv1, ... (MFMA-fragment packed), folded biases
    const float *hd, *hdb;             // policy_conv (2) + value_conv (1) rows of one 16-row tile, folded biases [3]
    const void *stemx[2], *blkx[2][6], *hdx[2];   // stem, the six 64 -> 64 convs and the head rows split into 16-bit fragments (az_net_emul.h), [0] bf16x3, [1] f16x2
};

template <int N>
__global__ __launch_bounds__(ResGeo<N>::NW * 64) void k_trunk_res(DevState d, ResWeights w, int net_id, float *__restrict__ feat)
{
    typedef ResGeo<N> G;
    constexpr int NTH = G::NW * 64;
    __shared__ __attribute__((aligned(16))) float lds[G::LDSF];
    __shared__ unsigned short wpos[G::MR];
    __shared__ unsigned short cellof[G::MR];
    __shared__ int any_active;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = blockIdx.x * G::G;
    if (tid == 0) any_active = 0;
    __syncthreads();
    if (tid < G::G) {
        int b = b0 + tid;
        if (b < d.B) {
            int kind = d.leaf_kind[b];
            if ((kind == LEAF_ROOT || kind == LEAF_EXPAND) && d.s_status[b] == SLOT_ACTIVE && d.s_net[b] == net_id)
                atomicOr(&any_active, 1);
        }
    }
    __syncthreads();
    if (!any_active) return;
    float *A = lds, *B = lds + 64 * G::CS;
    {
        float4 *z = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < G::LDSF / 4; i += NTH) z[i] = float4{0.f, 0.f, 0.f, 0.f};
    }
    for (int m = tid; m < G::MR; m += NTH) {
        int pos, cell;
        if constexpr (G::ROWT) {
            const int t = m >> 4, c = m & 15, g = t / N, r = t - g * N;
            pos = g * G::PP + (r + 1) * G::PW + (c + 1);
            cell = c < N ? g * G::nn + r * N + c : 0xFFFF;
        } else {
            const int g = m / G::nn, p = m - g * G::nn, r = p / N, c = p - r * N;
            pos = m < G::M ? g * G::PP + (r + 1) * G::PW + (c + 1) : G::PW + 1;
            cell = m < G::M ? m : 0xFFFF;
        }
        wpos[m] = (unsigned short)pos;
        cellof[m] = (unsigned short)cell;
    }
    __syncthreads();
    for (int m = tid; m < G::MR; m += NTH) {          // games.py:86-129 encode into plain planes at the start of B
        const int cell = cellof[m];
        if (cell != 0xFFFF) {
            const int g = cell / G::nn, p = cell - g * G::nn;
            const int b = b0 + g;
            if (b < d.B) {
                const u64 *lf = d.leaf + (size_t)b * 8;
                const int pos = wpos[m];
                const int ps = sym_cell(d.leaf_sym, b, p, N);
                if ((lf[ps >> 6] >> (ps & 63)) & 1ull) B[pos] = 1.0f;
                if ((lf[4 + (ps >> 6)] >> (ps & 63)) & 1ull) B[G::CS + pos] = 1.0f;
                if (d.leaf_last[b] == ps) B[2 * G::CS + pos] = 1.0f;
            }
        }
    }
    __syncthreads();
    conv_layer<G, 4, 64, CONV_OUT_PACKED>(B, A, w.stem, w.stemb, wpos, cellof, wave, lane);
    __syncthreads();
    for (int i = tid; i < 3 * G::CS; i += NTH) B[i] = 0.0f;     // the planes would alias padding cells of the packed image
    __syncthreads();
#pragma unroll 1
    for (int blk = 0; blk < 3; blk++) {
        conv_layer<G, 64, 64, CONV_OUT_PACKED>(A, B, w.blk[2 * blk], w.blkb[2 * blk], wpos, cellof, wave, lane);
        __syncthreads();
        conv_layer<G, 64, 64, CONV_OUT_RESIDUAL>(B, A, w.blk[2 * blk + 1], w.blkb[2 * blk + 1], wpos, cellof, wave, lane);
        __syncthreads();
    }
    // heads: D[head channel][cell] over the packed trunk image A, 16 k-steps (64 channels)
    {
        const int q = lane >> 4, r16 = lane & 15;
        const float4 *wp4 = reinterpret_cast<const float4 *>(w.hd) + lane;
        const float4 *in4 = reinterpret_cast<const float4 *>(A);
        float hb[4];
#pragma unroll
        for (int rg = 0; rg < 4; rg++) hb[rg] = (q * 4 + rg) < (G::PC + G::VC) ? w.hdb[q * 4 + rg] : 0.0f;
        for (int mt = wave; mt < G::MT; mt += G::NW) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            const int base = q * G::CS + (int)wpos[mt * 16 + r16];
#pragma unroll
            for (int cg = 0; cg < 4; cg++) {
                const float4 a = in4[base + cg * 4 * G::CS];
                const float4 wq = wp4[cg * 64];
                acc = mfma4(wq.x, a.x, acc);
                acc = mfma4(wq.y, a.y, acc);
                acc = mfma4(wq.z, a.z, acc);
                acc = mfma4(wq.w, a.w, acc);
            }
            const int cell = cellof[mt * 16 + r16];
            if (cell != 0xFFFF) {
                const int g = cell / G::nn, p = cell - g * G::nn;
                const int b = b0 + g;
                if (b < d.B && d.s_net[b] == net_id) {
#pragma unroll
                    for (int rg = 0; rg < 4; rg++) {
                        const int j = q * 4 + rg;     // 0-1 policy_conv, 2 value_conv
                        if (j < G::PC + G::VC) {
                            float v = acc[rg] + hb[rg];
                            feat[(size_t)b * G::FROW + j * G::nn + p] = v > 0.0f ? v : 0.0f;
                        }
                    }
                }
            }
        }
    }
}

// Tile-split trunk of the ResidualBlock variant: like k_tile, a board spread by CELL tiles, 4 waves per workgroup (the four
// 16-channel tiles of a 64-channel conv on one 16-cell tile: 144 dependent MFMAs each), grid (groups, MT), six launches.
// The 64-channel packed images A (block input/output) and B (intermediate) cross HBM/L2 in the scratch of the board group
// (padding ring zeroed once at allocation, never written):
//   KIND 0  encode + stem on the tiles around t (recomputed per workgroup: 9 k-steps) -> x of tile t to image A; res1.conv1 on tile t -> image B
//   KIND 1  rows of B around t -> conv2 of a block on tile t, relu(. + x) with x read and written in place in A
//   KIND 2  rows of A around t -> conv1 of the next block on tile t -> B
//   KIND 3  the last conv2: relu(. + x) stays in LDS as [channel][16 cells] -> 1x1 heads of the tile -> feature rows
// Same fma chains as k_trunk_res: bit-identical.
template <int N>
struct ResTileGeo : TileGeoT<ResGeo<N>, 4> {
    typedef TileGeoT<ResGeo<N>, 4> T;
    static constexpr int LDS0 = 68 * T::CSA, LDSC = 64 * T::CSB + 64 * 16;
    static constexpr int IMG = 64 * ResGeo<N>::CS;            // floats of one packed 64-channel board image
    static constexpr int SCRATCH = 2 * IMG;                   // floats of scratch per board group: images A and B
};

template <int N, int KIND>
__global__ __launch_bounds__(256) void k_tile_res(DevState d, const float *__restrict__ wp, const float *__restrict__ bias,
                                                  const float *__restrict__ wp2, const float *__restrict__ bias2, int net_id,
                                                  float *__restrict__ scratch, float *__restrict__ feat)
{
    typedef ResGeo<N> F;
    typedef ResTileGeo<N> TG;
    constexpr int NTH = 256;
    __shared__ __attribute__((aligned(16))) float lds[KIND == 0 ? TG::LDS0 : TG::LDSC];
    __shared__ unsigned short wpos[F::MR];
    __shared__ unsigned short cellof[F::MR];
    __shared__ int any_active;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = blockIdx.x, t = blockIdx.y, b0 = grp * F::G;
    const int org = KIND == 0 ? TG::org_a(t) : TG::org_b(t);
    if constexpr (KIND == 0) {
        float4 *z = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < TG::LDS0 / 4; i += NTH) z[i] = float4{0.f, 0.f, 0.f, 0.f};
    }
    if (!TG::prologue(d, net_id, b0, org, KIND == 0 ? TG::CSA : TG::CSB, wpos, cellof, &any_active, tid, NTH)) return;
    float *A = scratch + (size_t)grp * TG::SCRATCH, *B = A + TG::IMG;
    if constexpr (KIND == 0) {
        float *planes = lds, *x = lds + 4 * TG::CSA;          // x: the stem's output around tile t, packed, local geometry
        TG::encode(d, b0, org, TG::CSA, planes, cellof, tid, NTH);
        __syncthreads();
        const int tlo = TG::c1_lo(t), cnt = TG::c1_hi(t) - tlo + 1;
        conv_layer<typename TG::A, 4, 64, CONV_OUT_PACKED, TG::MTL1>(planes, x, wp, bias, wpos, cellof, wave, lane, tlo, cnt);
        __syncthreads();
        // x of tile t also goes to the board image A: the skip operand of res1 (read in place by KIND 1)
        for (int i = tid; i < 64 * 16; i += NTH) {
            const int co = i >> 4, m = t * 16 + (i & 15);
            if (cellof[m] != 0xFFFFu) {
                const int rel = wpos[m];
                A[pk_index<F>(co, rel + org)] = x[pk_index<typename TG::A>(co, rel)];
            }
        }
        conv_layer<typename TG::A, 64, 64, CONV_OUT_PACKED, 1, F>(x, B, wp2, bias2, wpos, cellof, wave, lane, t, 1, org);
    } else {
        TG::load_rows(KIND == 2 ? A : B, org, lds, tid, NTH);
        __syncthreads();
        if constexpr (KIND == 1) conv_layer<typename TG::B, 64, 64, CONV_OUT_RESIDUAL, 1, F>(lds, A, wp, bias, wpos, cellof, wave, lane, t, 1, org);
        else if constexpr (KIND == 2) conv_layer<typename TG::B, 64, 64, CONV_OUT_PACKED, 1, F>(lds, B, wp, bias, wpos, cellof, wave, lane, t, 1, org);
        else {
            float *xt = lds + 64 * TG::CSB;                   // [channel][16 cells of the tile]: the trunk's output
            conv_layer<typename TG::B, 64, 64, CONV_OUT3_RESIDUAL, 1, F, 16>(lds, xt, wp, bias, wpos, cellof, wave, lane, t, 1, org, A);
            __syncthreads();
            if (wave == 0) {                                  // policy_conv (64->2) and value_conv (64->1), BatchNorm folded: wp2 = packed head rows, bias2[3]
                const int q = lane >> 4, r16 = lane & 15;
                const float4 *wp4 = reinterpret_cast<const float4 *>(wp2) + lane;
                float hb[4];
#pragma unroll
                for (int rg = 0; rg < 4; rg++) hb[rg] = (q * 4 + rg) < (F::PC + F::VC) ? bias2[q * 4 + rg] : 0.0f;
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
                const float *ip = xt + q * 16 + r16;
#pragma unroll
                for (int s4 = 0; s4 < 4; s4++) {
                    const float4 bq = wp4[s4 * 64];
                    acc = mfma4(bq.x, ip[(s4 * 16 + 0) * 16], acc);
                    acc = mfma4(bq.y, ip[(s4 * 16 + 4) * 16], acc);
                    acc = mfma4(bq.z, ip[(s4 * 16 + 8) * 16], acc);
                    acc = mfma4(bq.w, ip[(s4 * 16 + 12) * 16], acc);
                }
                const int cell = cellof[t * 16 + r16];
                if (cell != 0xFFFF) {
                    const int g = cell / F::nn, p = cell - g * F::nn;
                    const int b = b0 + g;
                    if (b < d.B && d.s_net[b] == net_id) {
#pragma unroll
                        for (int rg = 0; rg < 4; rg++) {
                            const int j = q * 4 + rg;     // 0-1 policy_conv, 2 value_conv
                            if (j < F::PC + F::VC) {
                                float v = acc[rg] + hb[rg];
                                feat[(size_t)b * F::FROW + j * F::nn + p] = v > 0.0f ? v : 0.0f;
                            }
                        }
                    }
                }
            }
        }
    }
}

// policy_fc (net.py:65) and value_fc1 + ReLU (net.py:69): one workgroup = 16 boards x (TPW x R) 16-output tiles of one
// layer; it works through them in R rounds of TPW tiles, four waves per tile = the four chains of the canonical order
// (fc_chain_groups above).  grid = (ceil(B / 16), ceil(NTP / (TPW R)) policy workgroups + ceil(4 / (TPW R)) value workgroups).
//   * the chain's weight fragments (QG x dwordx4 per lane, L2) are requested first, before anything else, and the next
//     round's while the current round computes;
//   * the features the layer needs (policy or value part of the 16 boards' rows, only boards with a pending evaluation)
//     are staged into LDS once, as [group of 16 inputs][q][board] float4: a thread loads 16 consecutive inputs of one board
//     and stores them transposed 4 x 4, so that lane (q, board) reads the A operands of a group's four MFMAs (inputs
//     16 g + 4 e + q, e = 0..3) with ONE conflict-free ds_read_b128;
//   * QG x 4 dependent MFMAs per wave and round, partial sums combined through LDS in the canonical order.
// <1, 1> (4 waves, one per SIMD, 19 workgroups per board row at n = 15) is the latency shape: few rows, many CUs free.
// <2, 4> (8 waves, 3 workgroups per row) is the throughput shape: with every CU busy under another lane's trunk what the
// kernel costs is the number of CU slots it has to win and the times it stages a row's features (3 instead of 19);
// measured in the 4-lane pipeline at 15x15: one tile per workgroup 158.4 ms per ply, <4, 1> 157.6, trunk-bound floor 155.1.
template <class G, int TPW, int R>
__global__ __launch_bounds__(TPW * 256, (R > 1 && TPW <= 2) ? 2 * TPW : 1) void k_fc(DevState d, NetWeights w, int net_id, const float *__restrict__ feat,
                                                  unsigned long long *dbgfc)
{
    constexpr int NTH = TPW * 256, TW = TPW * R;       // threads, tiles per workgroup
    constexpr int NPW = (G::NTP + TW - 1) / TW;        // policy workgroups per board row
    __shared__ float4 ft4[4 * G::QGMAX * 64];          // [group][q][board]
    __shared__ float4 part[2 * TPW * 3 * 64];          // partial sums of chains 1..3, per tile and lane; double-buffered over the rounds
    __shared__ unsigned fc_active;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chain = wv & 3, tl = wv >> 2;
    const int mb = blockIdx.x * 16;
    const bool is_pol = (int)blockIdx.y < NPW;
    const int tile0 = is_pol ? blockIdx.y * TW + tl : G::NTP + ((int)blockIdx.y - NPW) * TW + tl;   // this wave's tile in round 0
    const int tile_end = is_pol ? G::NTP : G::NTP + 4;
#ifdef AZ_STAMPS
#define FC_STAMP(k) do { if (dbgfc && (threadIdx.x & 63) == 0) dbgfc[((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + ((threadIdx.x >> 6) & 7)) * 4 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define FC_STAMP(k) do { } while (0)
#endif
    FC_STAMP(0);
    const int QG = is_pol ? G::QGP : G::QGV;           // groups per chain
    const int K = is_pol ? G::PC * G::nn : G::VC * G::nn;
    const int koff = is_pol ? 0 : G::PC * G::nn;
    const int q = lane >> 4, r16 = lane & 15;
    // a chain's weight fragments: [tile][4 QG groups, zero-padded][lane] float4 (pack_fc)
    const float4 *wbase = reinterpret_cast<const float4 *>(is_pol ? w.pf : w.vf) + (size_t)chain * QG * 64 + lane;
    const int tsub = is_pol ? 0 : G::NTP;
    float4 wf[G::QGMAX];
    {
        const float4 *wp4 = wbase + (size_t)((tile0 < tile_end ? tile0 : tile_end - 1) - tsub) * 4 * QG * 64;
#pragma unroll
        for (int j = 0; j < G::QGMAX; j++) wf[j] = j < QG ? wp4[(size_t)j * 64] : float4{0.f, 0.f, 0.f, 0.f};
    }
    // the epilogues' biases, one per round, requested now so that no round waits for one
    float bias_r[R];
#pragma unroll
    for (int rd = 0; rd < R; rd++) {
        const int tile = tile0 + rd * TPW, o = (tile - tsub) * 16 + r16;
        bias_r[rd] = (chain == 0 && tile < tile_end && (!is_pol || o < G::nn)) ? (is_pol ? w.pfb[o] : w.vfb[o]) : 0.0f;
    }
    // boards of this row with a pending evaluation (episode tails, terminal leaves, cache hits leave rows idle)
    if (tid == 0) fc_active = 0u;
    __syncthreads();
    if (tid < 16) {
        const int b = mb + tid;
        if (b < d.B) {
            const int kind = d.leaf_kind[b];
            if ((kind == LEAF_ROOT || kind == LEAF_EXPAND) && d.s_status[b] == SLOT_ACTIVE && d.s_net[b] == net_id)
                atomicOr(&fc_active, 1u << tid);
        }
    }
    __syncthreads();
    const unsigned active = fc_active;
    if (!active) return;
    // stage: unit u = (group g, board i); inputs beyond K (chain padding) and idle boards are zeros
    const bool vec4 = (koff & 3) == 0;                 // the ResidualBlock net's value inputs start at 2 n^2: 8-byte aligned for odd n
    for (int u = tid; u < 4 * QG * 16; u += NTH) {
        const int g = u >> 4, i = u & 15;
        float x[16];
#pragma unroll
        for (int e = 0; e < 16; e++) x[e] = 0.0f;
        const int k0 = 16 * g;
        if (((active >> i) & 1u) && k0 < K) {
            const float *src = feat + (size_t)(mb + i) * G::FROW + koff + k0;
            if (vec4) {
#pragma unroll
                for (int a = 0; a < 4; a++)
                    if (k0 + 4 * a < K) {
                        const float4 v = reinterpret_cast<const float4 *>(src)[a];
                        x[4 * a] = v.x; x[4 * a + 1] = v.y; x[4 * a + 2] = v.z; x[4 * a + 3] = v.w;
                    }
            } else {
#pragma unroll
                for (int a = 0; a < 8; a++)
                    if (k0 + 2 * a < K) {
                        const float2 v = reinterpret_cast<const float2 *>(src)[a];
                        x[2 * a] = v.x; x[2 * a + 1] = v.y;
                    }
            }
#pragma unroll
            for (int e = 0; e < 16; e++) x[e] = k0 + e < K ? x[e] : 0.0f;     // the row's next part / tail is not this layer's input
        }
#pragma unroll
        for (int qq = 0; qq < 4; qq++) ft4[(g * 4 + qq) * 16 + i] = float4{x[qq], x[4 + qq], x[8 + qq], x[12 + qq]};
    }
    __syncthreads();
    FC_STAMP(1);
    const float4 *fp = ft4 + (chain * QG * 4 + q) * 16 + r16;
#pragma unroll
    for (int rd = 0; rd < R; rd++) {
        const int tile = tile0 + rd * TPW;
        const bool has_tile = tile < tile_end;
        // the next round's fragments are requested into the registers of this round's as soon as those have been used: a
        // whole round (4 QG MFMAs) of flight time, no second register set (two workgroups fit a CU: one stages while one computes)
        const int tn = tile + TPW < tile_end ? tile + TPW : tile_end - 1;
        const float4 *wnext = wbase + (size_t)(tn - tsub) * 4 * QG * 64;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < G::QGMAX; j++)
            if (j < QG) {
                const float4 af = fp[j * 64];
                const float4 wv = wf[j];
                if (R > 1 && rd + 1 < R) wf[j] = wnext[(size_t)j * 64];
                if (has_tile) {
                    acc = mfma4(af.x, wv.x, acc);
                    acc = mfma4(af.y, wv.y, acc);
                    acc = mfma4(af.z, wv.z, acc);
                    acc = mfma4(af.w, wv.w, acc);
                }
            }
        float4 *pr = part + (rd & 1) * TPW * 3 * 64;
        if (chain) pr[(tl * 3 + chain - 1) * 64 + lane] = float4{acc[0], acc[1], acc[2], acc[3]};
        __syncthreads();
        if (!chain && has_tile) {
            const float4 p1 = pr[(tl * 3) * 64 + lane], p2 = pr[(tl * 3 + 1) * 64 + lane], p3 = pr[(tl * 3 + 2) * 64 + lane];
            const float r[4] = {(acc[0] + p1.x) + (p2.x + p3.x), (acc[1] + p1.y) + (p2.y + p3.y),
                                (acc[2] + p1.z) + (p2.z + p3.z), (acc[3] + p1.w) + (p2.w + p3.w)};
            // only slots with a pending evaluation are written: the row of a slot whose evaluation came from the cache (or
            // that waits on a terminal leaf) must stay as it is
#pragma unroll
            for (int rg = 0; rg < 4; rg++) {
                const int i = q * 4 + rg, b = mb + i;
                if ((active >> i) & 1u) {
                    if (is_pol) {
                        const int j = tile * 16 + r16;
                        if (j < G::nn) d.logits[(size_t)b * G::RW + j] = r[rg] + bias_r[rd];
                    } else {
                        const int o = (tile - G::NTP) * 16 + r16;
                        const float v = r[rg] + bias_r[rd];
                        d.vhid[(size_t)b * 64 + o] = v > 0.0f ? v : 0.0f;
                    }
                }
            }
        }
    }
    FC_STAMP(2);
}
