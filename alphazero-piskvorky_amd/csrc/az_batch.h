// az_batch.h -- az_search, az_search_batch, az_search_callback: given positions into the slots, and every slot's root
// statistics back out.
//
// A wave of the batch is one ply of the lanes it is spread over (all of them, or lane 0 alone for one position): position i
// of the wave sits in slot b of lane l with i = lane.first + b, b < lane.m, and is game i of a one-ply episode (its noise
// row, u, temperature and record are indexed by i).  Both kernels run one 64-lane wavefront per slot over all those lanes in
// one launch; the lanes' buffers
// are separate allocations, so their pointers travel by value in a BatchLanes table.  Neither kernel is compute-bound:
// what matters is one launch per wave and coalesced traffic.
#pragma once
#include "az_tree.h"

constexpr int BATCH_MAX_LANES = 16;    // az_config.engines <= 16

struct BatchLane {
    u64 *board;                        // [B][8]
    int *s_game, *s_ply, *s_player, *s_last, *s_status, *leaf_kind, *carried;
    const Edge *edges;                 // [B][R][RW]
    int B, first, m;                   // slots of the lane; index of its first position in the wave; positions it holds
};
struct BatchLanes {
    int K, L;                          // lanes; evaluation items per slot (DevState.L)
    BatchLane lane[BATCH_MAX_LANES];
};

// wave-uniform: the lane and slot wavefront w works on; false behind the last slot of the last lane
__device__ __forceinline__ bool batch_slot_of(const BatchLanes &bl, int w, int &l, int &b)
{
    int base = 0;
    for (l = 0; l < bl.K; l++) {
        if (w < base + bl.lane[l].B) { b = w - base; return true; }
        base += bl.lane[l].B;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------
// cells_to_planes: one position's cells[n*n] (0 empty, 1 X, 2 O) -> bit-planes, by the whole wavefront.  Lane j reads cell
// j + 64 q; the ballots of (cell == 1) and (cell == 2) ARE word q of the X and O planes, and the ply is the popcount of the
// occupancy.  Returns in lanes 0..3 X word `lane`, in lanes 4..7 O word `lane - 4` (words beyond CPL zero).
// ------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ u64 cells_to_planes(const unsigned char *__restrict__ cp, int lane, int &ply)
{
    typedef TreeGeo<N> G;
    u64 mine = 0ull;
    ply = 0;
#pragma unroll
    for (int q = 0; q < G::CPL; q++) {
        const int j = lane + 64 * q;
        const int c = j < G::nn ? (int)cp[j] : 0;
        const u64 x = __ballot(c == 1), o = __ballot(c == 2);
        ply += __popcll(x | o);
        mine = lane == q ? x : (lane == 4 + q ? o : mine);
    }
    return mine;
}

// ------------------------------------------------------------------------------------------------
// k_set_positions: cells[wave][n*n] -> the slots' bit-planes and game state, as k_refill does for a claimed game.  Slots
// beyond the lane's share go idle.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void k_set_positions(BatchLanes bl, const unsigned char *__restrict__ cells,
                                                       const unsigned char *__restrict__ players, const short *__restrict__ lasts)
{
    typedef TreeGeo<N> G;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    int l, b;
    if (!batch_slot_of(bl, w, l, b)) return;
    const BatchLane &ln = bl.lane[l];
    if (b >= ln.m) {
        if (lane == 0) { ln.s_status[b] = SLOT_IDLE; ln.s_game[b] = -1; }
        return;
    }
    const int i = ln.first + b;
    int ply;
    const u64 mine = cells_to_planes<N>(cells + (size_t)i * G::nn, lane, ply);
    if (lane < 8) ln.board[(size_t)b * 8 + lane] = mine;       // one 64-byte store; words beyond CPL are zero
    if (lane == 0) {
        ln.s_game[b] = i;
        ln.s_ply[b] = ply;
        ln.s_player[b] = players[i];
        ln.s_last[b] = lasts[i];
        ln.s_status[b] = SLOT_ACTIVE;
        ln.leaf_kind[(size_t)b * bl.L] = LEAF_NONE;
        ln.carried[b] = -1;            // a fresh root, whatever az_set_subtree_reuse says
    }
}

// ------------------------------------------------------------------------------------------------
// k_build_positions: cells[count][n*n] -> the table of start positions k_refill loads claimed games from
// (az_set_start_positions).  One wavefront per position, the same planes and ply as k_set_positions.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void k_build_positions(int count, const unsigned char *__restrict__ cells,
                                                         const unsigned char *__restrict__ players, const short *__restrict__ lasts,
                                                         StartPos *__restrict__ table)
{
    typedef TreeGeo<N> G;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= count) return;
    int ply;
    const u64 mine = cells_to_planes<N>(cells + (size_t)i * G::nn, lane, ply);
    if (lane < 8) table[i].w[lane] = mine;
    if (lane == 0) { table[i].ply = ply; table[i].player = players[i]; table[i].last = lasts[i]; table[i].pad = 0; }
}

// ------------------------------------------------------------------------------------------------
// k_gather_roots: after the ply (k_move), the root row of every slot -> compact [wave][n*n] visits / W / prior, illegal
// cells 0 / 0.0 / 0.0f, and the slot's record (pi row, action) -> compact staging, so that every requested output is ONE
// contiguous device-to-host copy per wave.  Occupancy and ply come from the wave's own cell bytes (still in place, the
// ballots of k_set_positions again), not from the slot, so the gather does not depend on what the ply did to the slot's
// state.  The root row is read with 16-byte loads, lane j edge j + 64 q.  Works after the persistent search kernel too: it
// writes the root row back to d.edges before k_move.  Any output pointer may be null.
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void k_gather_roots(BatchLanes bl, int R, int S, const unsigned char *__restrict__ cells,
                                                      const float *__restrict__ rec_pi, const short *__restrict__ rec_action,
                                                      int *__restrict__ visits, double *__restrict__ W, float *__restrict__ prior,
                                                      float *__restrict__ pi, int *__restrict__ action)
{
    typedef TreeGeo<N> G;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    int l, b;
    if (!batch_slot_of(bl, w, l, b)) return;
    const BatchLane &ln = bl.lane[l];
    if (b >= ln.m) return;
    const int i = ln.first + b;                        // the game of the slot
    const unsigned char *cp = cells + (size_t)i * G::nn;
    bool legal[G::CPL];
    int ply = 0;                                       // the record of the search: the stones on the given board
#pragma unroll
    for (int q = 0; q < G::CPL; q++) {
        const int j = lane + 64 * q;
        const int c = j < G::nn ? (int)cp[j] : 0;
        legal[q] = c == 0;
        ply += __popcll(__ballot(c != 0));
    }
    const size_t ri = (size_t)i * G::nn + ply;
    const Edge *root = ln.edges + (size_t)b * R * G::RW;
    const int nmask = S > DEFAULT_MAX_S ? 0xFFFF : EDGE_N_MASK;     // as k_move: deep searches use the whole 16-bit count
#pragma unroll
    for (int q = 0; q < G::CPL; q++) {
        const int j = lane + 64 * q;
        if (j >= G::nn) continue;
        const Edge e = root[j];
        const size_t o = (size_t)i * G::nn + j;
        if (visits) visits[o] = legal[q] ? ((int)e.N & nmask) : 0;
        if (W) W[o] = legal[q] ? e.W : 0.0;
        if (prior) prior[o] = legal[q] ? e.P : 0.0f;
        if (pi) pi[o] = rec_pi[ri * G::nn + j];
    }
    if (action && lane == 0) action[i] = rec_action[ri];
}
