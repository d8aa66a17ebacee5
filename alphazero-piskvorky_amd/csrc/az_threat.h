// az_threat.h -- the root threat search (az_set_threat_search, az_threat_batch): an exact forced-four search ("victory by
// continuous fours") over the rules of the game, run on every root before the simulations.  The rule is stated in full in
// include/az_engine.h; threat_solve_host below restates it literally for the host (az_threat_solve), k_threat runs it with one
// wavefront per position and hands its results to the solver as premarked root statuses (DevState.threat_edges / threat_root).
//
// Both planes are wave-uniform and seen from the root's side to move A: after A's four and D's forced reply A is to move
// again, so the planes never swap.  Lanes take cells lane, lane + 64, ..; a win set is CPL ballots.  Two facts of the game keep
// the kernel short -- a stone of the other colour on an empty cell never changes a maximal run of one's own stones, so
//   win(P + A at x, D) = win(P, D) \ {x}: with the candidates of step 3 it is always empty, the test of step 4 never fires;
//   win(P'', A) = win(P', A) \ {w} = {}: step 1 only ever finds something at the root;
// and a winning cell that appears after A plays x has its run through x: only the cells on the four lines through x within
// k - 1 steps are tested for "is x a four".  The host restatement makes none of these shortcuts.
#pragma once
#include "az_tree.h"

constexpr int THREAT_MAX_DEPTH = 16;   // AZ_THREAT_MAX_DEPTH of include/az_engine.h
constexpr int THREAT_STATS = 5;        // per slot: roots proven WIN, roots proven LOSS, block-only roots, exhausted searches, nodes

// ------------------------------------------------------------------------------------------------
// host: the rule as written, on cell arrays (0 empty, 1 A, 2 D)
// ------------------------------------------------------------------------------------------------
struct ThreatHost {
    int n, k, rule, budget, nodes;
    bool exhausted;
    unsigned char c[225];              // 0 empty, 1 the root's mover A, 2 its opponent D
};
// does a stone of `col` on the empty cell a win at once (wins_through on the plane with the stone added)
inline bool threat_host_wins(const ThreatHost &t, int a, int col)
{
    static const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
    const int n = t.n, r = a / n, c = a - r * n;
    for (int d = 0; d < 4; d++) {
        int cnt = 1;
        for (int s = 1; s < n; s++) {
            const int rr = r + s * dr[d], cc = c + s * dc[d];
            if (rr < 0 || rr >= n || cc < 0 || cc >= n || t.c[rr * n + cc] != col) break;
            cnt++;
        }
        for (int s = 1; s < n; s++) {
            const int rr = r - s * dr[d], cc = c - s * dc[d];
            if (rr < 0 || rr >= n || cc < 0 || cc >= n || t.c[rr * n + cc] != col) break;
            cnt++;
        }
        if (run_wins(cnt, t.k, t.rule)) return true;
    }
    return false;
}
// win(P, col) into out[] in ascending order; returns its size
inline int threat_host_winset(const ThreatHost &t, int col, int *out)
{
    int m = 0;
    for (int j = 0; j < t.n * t.n; j++)
        if (t.c[j] == 0 && threat_host_wins(t, j, col)) out[m++] = j;
    return m;
}
// T(P, d): the depth of the line found (0 = not found), its first move in *move
inline int threat_host_T(ThreatHost &t, int d, int *move)
{
    const int nn = t.n * t.n;
    int wa[225], wd[225], w[225], cand[225];
    if (threat_host_winset(t, 1, wa) > 0) { *move = wa[0]; return 1; }
    if (d <= 1) return 0;
    const int nd = threat_host_winset(t, 2, wd);
    if (nd >= 2) return 0;
    int nc = 0;
    if (nd == 1) cand[nc++] = wd[0];
    else
        for (int j = 0; j < nn; j++)
            if (t.c[j] == 0) cand[nc++] = j;
    for (int i = 0; i < nc; i++) {
        const int x = cand[i];
        t.c[x] = 1;
        const int nw = threat_host_winset(t, 1, w);
        int res = 0;
        if (nw > 0) {
            t.nodes++;
            if (t.nodes > t.budget) { t.exhausted = true; t.c[x] = 0; return 0; }
            if (threat_host_winset(t, 2, wd) == 0) {
                if (nw >= 2) res = 2;
                else {
                    int sub = -1;
                    t.c[w[0]] = 2;
                    const int r = threat_host_T(t, d - 1, &sub);
                    t.c[w[0]] = 0;
                    if (r > 0) res = r + 1;
                }
            }
        }
        t.c[x] = 0;
        if (t.exhausted) return 0;
        if (res > 0) { *move = x; return res; }
    }
    return 0;
}
// One position: board[n*n] (0 empty, 1 X, 2 O) with `player` to move.  Writes the root row's statuses (0 on occupied cells)
// to edges[n*n] when given and returns the root status.
inline int threat_solve_host(const unsigned char *board, int n, int k, int rule, int player, int max_depth, int node_budget,
                             int *move, int *depth, int *nodes, signed char *edges)
{
    ThreatHost t;
    t.n = n; t.k = k; t.rule = rule; t.budget = node_budget; t.nodes = 0; t.exhausted = false;
    const int nn = n * n;
    for (int j = 0; j < nn; j++) t.c[j] = board[j] == 0 ? 0 : (board[j] == player ? 1 : 2);
    int wa[225], wd[225];
    const int na = threat_host_winset(t, 1, wa), nd = threat_host_winset(t, 2, wd);     // the root's Wd, before any node is counted
    int mv = -1;
    int dp = threat_host_T(t, max_depth, &mv);
    if (t.exhausted) { dp = 0; mv = -1; }
    if (edges) {
        for (int j = 0; j < nn; j++) edges[j] = PROOF_UNKNOWN;
        if (dp == 1) { for (int i = 0; i < na; i++) edges[wa[i]] = PROOF_WIN; }
        else if (dp > 1) edges[mv] = PROOF_WIN;
        else if (nd > 0) {
            for (int j = 0; j < nn; j++) edges[j] = t.c[j] == 0 ? PROOF_LOSS : PROOF_UNKNOWN;
            if (nd == 1) edges[wd[0]] = PROOF_UNKNOWN;
        }
    }
    if (move) *move = mv;
    if (depth) *depth = dp;
    if (nodes) *nodes = t.nodes;
    return dp > 0 ? PROOF_WIN : (nd >= 2 ? PROOF_LOSS : PROOF_UNKNOWN);
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pl_clear(Plane &p, int j)
{
    const int wi = j >> 6;
    const u64 b = ~(1ull << (j & 63));
    p.w[0] &= wi == 0 ? b : ~0ull;
    p.w[1] &= wi == 1 ? b : ~0ull;
    p.w[2] &= wi == 2 ? b : ~0ull;
    p.w[3] &= wi == 3 ? b : ~0ull;
}
// the lowest set cell, -1 for the empty plane
__device__ __forceinline__ int pl_lowest(const Plane &p)
{
    if (p.w[0]) return __builtin_ctzll(p.w[0]);
    if (p.w[1]) return 64 + __builtin_ctzll(p.w[1]);
    if (p.w[2]) return 128 + __builtin_ctzll(p.w[2]);
    if (p.w[3]) return 192 + __builtin_ctzll(p.w[3]);
    return -1;
}

// win(P, c): the empty cells where a stone on plane `me` wins at once, one ballot per 64 cells (wins_through counts the
// neighbours of the cell only, so the stone itself need not be added)
template <int N>
__device__ __forceinline__ Plane threat_winset(const Plane &me, const Plane &occ, int k, int rule, int lane)
{
    typedef TreeGeo<N> G;
    Plane w;
    w.w[0] = w.w[1] = w.w[2] = w.w[3] = 0ull;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        const int j = lane + 64 * i;
        const bool hit = j < G::nn && !pl_get(occ, j) && wins_through(me, j, N, k, rule);
        w.w[i] = __ballot(hit);
    }
    return w;
}

// "is x a four": the size of win(P + A at x, A) and, in w, one of its cells (the only one when the size is 1).  me2 / occ2
// hold the stone at x already.  Probe slot idx = 32 * direction + 16 * side + (step - 1), steps 1 .. k - 1 <= 14: two rounds
// of 64 lanes.  The probed cells are distinct, so the ballots count the set.
template <int N>
__device__ __forceinline__ int threat_four(const Plane &me2, const Plane &occ2, int x, int k, int rule, int lane, int &w)
{
    const int r = x / N, c = x - r * N;
    int cnt = 0;
    w = -1;
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int idx = lane + 64 * p;
        const int dsel = idx >> 5, s = (idx & 15) + 1, sgn = (idx & 16) ? -s : s;
        const int dr = dsel == 0 ? 0 : 1, dc = dsel == 0 ? 1 : (dsel == 1 ? 0 : (dsel == 2 ? 1 : -1));
        const int rr = r + sgn * dr, cc = c + sgn * dc;
        const bool inb = s < k && rr >= 0 && rr < N && cc >= 0 && cc < N;
        const int cell = inb ? rr * N + cc : 0;
        const bool hit = inb && !pl_get(occ2, cell) && wins_through(me2, cell, N, k, rule);
        const u64 m = __ballot(hit);
        if (m != 0ull && w < 0) w = __shfl(cell, __builtin_ctzll(m), 64);
        cnt += __popcll(m);
    }
    return cnt;
}

// One wavefront (= one workgroup) per slot.  Every loop is bounded: the sets by n * n, the stack by max_depth, the walk by
// (node_budget + 2) level visits of at most n * n candidates and one return each.
template <int N>
__global__ __launch_bounds__(64) void k_threat(DevState d)
{
    typedef TreeGeo<N> G;
    __shared__ u64 s_cand[THREAT_MAX_DEPTH][4];        // per level: the candidates still to try, the cell tried, the forced reply
    __shared__ int s_x[THREAT_MAX_DEPTH], s_w[THREAT_MAX_DEPTH];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= d.B || d.s_status[b] != SLOT_ACTIVE) return;
    const int k = d.k, rule = d.rule, max_depth = d.threat_max_depth, budget = d.threat_budget;
    const int pl = d.s_player[b];
    const Plane bX = pl_load(d.board + (size_t)b * 8), bO = pl_load(d.board + (size_t)b * 8 + 4);
    Plane me = pl == 1 ? bX : bO, opp = pl == 1 ? bO : bX;
    Plane occ0;
#pragma unroll
    for (int q = 0; q < 4; q++) occ0.w[q] = me.w[q] | opp.w[q];
    const Plane Wa = threat_winset<N>(me, occ0, k, rule, lane);
    const Plane Wd = threat_winset<N>(opp, occ0, k, rule, lane);     // the root's: the LOSS marks do not depend on the budget
    const int nwd = pl_count(Wd);
    int move = -1, depth = 0, nodes = 0;
    if (pl_count(Wa) > 0) {
        move = pl_lowest(Wa);
        depth = 1;
    } else if (max_depth > 1) {
        int lvl = 0;
        bool enter = true;
        Plane cand;
        cand.w[0] = cand.w[1] = cand.w[2] = cand.w[3] = 0ull;
        const int limit = (budget + 2) * (G::nn + 1);
        for (int it = 0; it < limit; it++) {
            if (enter) {
                // steps 2 and 3 of level lvl (max_depth - lvl >= 2 holds for every level entered)
                Plane occ;
#pragma unroll
                for (int q = 0; q < 4; q++) occ.w[q] = me.w[q] | opp.w[q];
                const Plane wd = lvl == 0 ? Wd : threat_winset<N>(opp, occ, k, rule, lane);
                const int c = pl_count(wd);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int rest = G::nn - 64 * q;                       // board cells in word q
                    const u64 board_mask = rest >= 64 ? ~0ull : (rest > 0 ? (1ull << rest) - 1ull : 0ull);
                    cand.w[q] = c >= 2 ? 0ull : (c == 1 ? wd.w[q] : ~occ.w[q] & board_mask);
                }
                enter = false;
            }
            const int x = pl_lowest(cand);
            if (x < 0) {                                                   // step 5: back to the level above, its next candidate
                if (lvl == 0) break;
                lvl--;
                pl_clear(me, s_x[lvl]);
                pl_clear(opp, s_w[lvl]);
#pragma unroll
                for (int q = 0; q < 4; q++) cand.w[q] = s_cand[lvl][q];
                continue;
            }
            pl_clear(cand, x);
            Plane me2 = me, occ2;
            pl_set(me2, x);
#pragma unroll
            for (int q = 0; q < 4; q++) occ2.w[q] = me2.w[q] | opp.w[q];
            int w;
            const int nw = threat_four<N>(me2, occ2, x, k, rule, lane, w);
            if (nw == 0) continue;                                         // not a four: no node
            nodes++;
            if (nodes > budget) break;                                     // exhausted: no win is reported
            if (nw >= 2) { move = lvl == 0 ? x : s_x[0]; depth = lvl + 2; break; }
            // T(P'', d - 1) with d = max_depth - lvl: its step 1 finds nothing, and with d - 1 <= 1 it ends there
            if (max_depth - lvl - 1 <= 1) continue;
            s_x[lvl] = x;
            s_w[lvl] = w;
#pragma unroll
            for (int q = 0; q < 4; q++) s_cand[lvl][q] = cand.w[q];
            me = me2;
            pl_set(opp, w);
            lvl++;
            enter = true;
        }
    }
    const bool found = depth > 0;
    const int root = found ? PROOF_WIN : (nwd >= 2 ? PROOF_LOSS : PROOF_UNKNOWN);
    unsigned char *erow = d.threat_edges + (size_t)b * G::RW;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        const int j = lane + 64 * i;
        const bool legal = j < G::nn && !pl_get(occ0, j);
        int st = PROOF_UNKNOWN;
        if (depth == 1) st = legal && pl_get(Wa, j) ? PROOF_WIN : PROOF_UNKNOWN;
        else if (found) st = j == move ? PROOF_WIN : PROOF_UNKNOWN;
        else if (nwd > 0) st = legal && !(nwd == 1 && pl_get(Wd, j)) ? PROOF_LOSS : PROOF_UNKNOWN;
        erow[j] = (unsigned char)st;
    }
    if (lane == 0) {
        d.threat_root[b] = (signed char)root;
        d.threat_depth[b] = (signed char)depth;
        d.threat_move[b] = (short)move;
        d.threat_nodes[b] = nodes;
        unsigned long long *st = d.threat_stat + (size_t)b * THREAT_STATS;
        st[0] += root == PROOF_WIN ? 1ull : 0ull;
        st[1] += root == PROOF_LOSS ? 1ull : 0ull;
        st[2] += !found && nwd == 1 ? 1ull : 0ull;
        st[3] += nodes > budget ? 1ull : 0ull;
        st[4] += (unsigned long long)nodes;
    }
}
