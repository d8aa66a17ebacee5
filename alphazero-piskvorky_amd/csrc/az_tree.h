// az_tree.h -- per-wavefront MCTS kernels (select / expand / backup / move) over an array tree in HBM.
//
// One 64-lane wavefront owns one game slot.  A node that has been expanded owns one ROW of
// RW = roundup(n*n, 64) edge records (16 B each: W f64, P f32, N u16, child-row u16), indexed by
// board cell, so a level of the descent is CPL = RW/64 coalesced 16-byte loads per lane and the
// reference's "first maximal child in row-major order" (mcts.py:71) is a (max score, min cell)
// wave reduction.  Boards are two bit-planes of 4 x u64.  Reference semantics: mcts.py:25-183,
// games.py:35-166, self_play.py:48-73, evaluator.py:64-90 (cited inline).
#pragma once
#include "az_device.h"

enum { LEAF_NONE = 0, LEAF_EXPAND = 1, LEAF_TERM_LOSS = 2, LEAF_TERM_DRAW = 3, LEAF_ROOT = 4,
       LEAF_REUSE = 5,        // root retained from the previous ply's search (subtree reuse): no evaluation, noise mix only
       LEAF_EXPAND_HIT = 6, LEAF_ROOT_HIT = 7,   // evaluation cache hit: logits / hidden row already in place, the net kernels skip the slot
       LEAF_TERM_WIN = 8,     // az_set_solver: the descent stopped on an edge proven LOSS for its mover, the side to move below it has won (+1)
       LEAF_DUP_BASE = 16 };  // virtual-loss batching: LEAF_DUP_BASE + i = same leaf as item i of this batch (no second evaluation)
__host__ __device__ constexpr bool leaf_needs_net(int kind) { return kind == LEAF_ROOT || kind == LEAF_EXPAND; }
constexpr int VL_MAX = 32;             // leaves per batch in virtual-loss mode (5 spare bits of the edge's visit field)
constexpr int EDGE_N_BITS = 11, EDGE_N_MASK = (1 << EDGE_N_BITS) - 1;   // visit count 0..1024 in the low bits, in-flight count above
constexpr int REUSE_MAX_ROWS = 1024;   // rows per slot (S + 2) the in-place compaction of k_move can renumber
// Deep searches (az_create_deep): above DEFAULT_MAX_S simulations the narrow budgets of the default kernels no longer hold --
// the sqrt table outgrows k_step's LDS copy and the visit count outgrows EDGE_N_BITS -- so S > DEFAULT_MAX_S runs the DEEP
// instantiations of k_step / k_step_vl (sqrt table read from HBM / L2, in-flight counts in a byte array beside the tree).  Up to
// DEFAULT_MAX_S a deep engine runs the default instantiations, whose code and arguments the DEEP ones leave untouched.  The 16-bit child row, path row and visit fields bound S by 65534.
constexpr int DEFAULT_MAX_S = 1024;
constexpr int CNT_STRIDE = 8;  // per-slot counters: expansions, simulations, terminal hits, depth sum, reused roots, duplicate leaves,
                               // cache lookups, cache hits
enum { SLOT_IDLE = 0, SLOT_ACTIVE = 1, SLOT_FINISHED = 2 };
// az_set_solver: the status of an edge, seen from the side that makes the move (AZ_PROOF_* of include/az_engine.h)
enum { PROOF_UNKNOWN = 0, PROOF_WIN = 1, PROOF_LOSS = 2, PROOF_DRAW = 3 };
__host__ __device__ constexpr int proof_negate(int s) { return s == PROOF_WIN ? PROOF_LOSS : (s == PROOF_LOSS ? PROOF_WIN : s); }

struct __attribute__((aligned(16))) Edge {
    double W;              // mcts.py:38 total value (float64 like the reference)
    float P;               // mcts.py:63 prior (float32 value widened on use)
    unsigned short N;      // mcts.py:37 visit count
    unsigned short child;  // row of the expanded child node, 0 = not expanded (row 0 is the root)
};

// One start position of az_set_start_positions: the board a claimed game begins from instead of the empty one.
struct __attribute__((aligned(16))) StartPos {
    u64 w[8];              // absolute bit-planes like DevState.board: words 0-3 X, 4-7 O
    int ply, player, last, pad;   // stones on the board, side to move (1 / 2), last action (-1 none)
};

struct DevState {
    int B, R, S, k, max_plies, add_noise, arena, total_games;
    double c_puct, w_noise;
    float one_minus_w;
    int rule;              // az_set_win_rule: WIN_RULE_FREESTYLE (a run of k or more wins) | WIN_RULE_EXACT (exactly k), beside k in every win test
    // --- slots (current real game per slot) ---
    u64 *board;            // [B][8] absolute bit-planes: words 0-3 X, 4-7 O
    int *s_game, *s_ply, *s_player, *s_last, *s_status, *s_net;
    // --- search state per slot ---
    Edge *edges;           // [B][R][RW]
    int *rows_used;        // [B]
    unsigned *path;        // [B][PATH] (row << 16 | cell)
    int *depth;            // [B]
    int *leaf_kind;        // [B]
    u64 *leaf;             // [B][8] mover-relative planes of the pending leaf: words 0-3 side to move, 4-7 opponent
    int *leaf_last;        // [B]
    // --- evaluator outputs ---
    float *logits;         // [B][RW]
    float *vhid;           // [B][64]
    const float *v2w[2];   // value_fc2.weight per net slot
    const float *v2b[2];
    // --- RNG tapes per game (numpy legacy stream, see az_rng.cpp) ---
    const double *noise;   // [G][noise_stride]
    long long noise_stride;
    const double *u;       // [G][nn]
    const int *noise_off;  // [nn+1] offset of ply m inside a game's noise tape
    // --- tables ---
    const double *T_table; // temperature by ply (self-play) or step (arena)
    const float *log_table;   // float32 log(N + 1e-8), N = 0..S
    const double *sqrt_table; // sqrt(N + 1e-8), N = 0..S+1
    // --- records per game: index game*nn + ply ---
    u64 *rec_planes;       // [G*nn][8] mover-relative planes before the move
    short *rec_last, *rec_action;
    unsigned char *rec_mover;
    float *rec_pi;         // [G*nn][nn]
    unsigned short *rec_visits; // [G*nn][nn]
    int *g_nply, *g_result;
    // --- bookkeeping ---
    unsigned long long *cnt;   // [B][CNT_STRIDE] expansions, simulations, terminal hits, depth sum, reused roots
    // --- opt-in subtree reuse between plies (the reference's TODO, mcts.py:17-22,106) ---
    int reuse;             // 0: every ply searches from a fresh root like the reference
    int *carried;          // [B] visits the retained root already holds (sum of its children's N), -1 = fresh root
    int *next_game;        // device counter
    int *active;           // number of active slots after refill
    // --- opt-in evaluation cache (the reference's TODO, mcts.py:17 DEFAULT_CACHE_SIZE, mcts.py:22 "add caching") ---
    float *cache;          // [cache_mask + 1][CACHE_HDR + RW + 64] floats, nullptr = off; shared by the lanes of an engine
    unsigned cache_mask;   // entries - 1 (a power of two)
    unsigned cache_gen;    // bumped by every weight load: entries of older weights never match
    // --- opt-in virtual-loss batching (the reference's TODO, mcts.py:17-22): L leaves per game and evaluation batch ---
    int L;                 // 1 = the reference's sequential simulation loop (mcts.py:123-141)
    int *it_status, *it_net;   // [B*L] per evaluation item, what the net kernels read as s_status / s_net (alias them when L == 1)
    int *leaf_sym;         // [B] opt-in random-symmetry leaf evaluation (az_set_leaf_symmetry): symmetry 0..7 the net sees the pending leaf in; nullptr = off
    int ext_eval;          // the pending rows were filled by an evaluator outside the engine (az_ext.h): priors and value as given
    unsigned game_key0;    // leaf-symmetry hash key of game id 0 = low 32 bits of the episode's seed0: key(g) = game_key0 + g is the game's
                           // seed, a GLOBAL name of the game that does not depend on which rank / slot / lane plays it
    unsigned key_stride;   // key(g) = game_key0 + key_stride * g.  1 everywhere; 0 in az_search_batch, whose positions all carry
                           // key 0 like az_search's, so that a result never depends on the position's index in the batch
    const double *T_game;  // [G] temperature per game, preferred over T_table by k_move when set (az_search_batch: positions with
                           // the same stone count may ask for different temperatures); nullptr everywhere else
    // --- opt-in start positions (az_set_start_positions), read by k_refill only; nullptr / 0 on every path but self-play and arena ---
    const StartPos *start_pos;   // [start_count]; nullptr = every game starts from the empty board
    int start_count;
    int start_first;       // `first` mod 2 * start_count: game g starts from position (start_first + g) % start_count, in the
                           // arena from ((start_first + g) >> 1) % start_count with the colours exchanged for odd g
    // --- search value per record and opt-in resignation (az_set_resign), written / applied by k_move only ---
    double resign_thr;     // a ply crosses when ply >= resign_min_ply and v < -resign_thr; 0 = off (and on every preset episode)
    float *rec_value;      // [G*nn] (float)v of every record, v = W[a*] / N[a*] of the root's most visited legal cell
    int *g_cross;          // [G] first crossing ply of the game, exempt games included; -1 = none
    int resign_min_ply;
    int resign_permille;   // game g is exempt (plays on) when fmix32(key(g)) % 1000 < resign_permille; no arena game is
    // --- opt-in playout cap randomisation (az_set_playout_cap): self-play episodes only, cap_fast = 0 on every other path ---
    int cap_fast;          // simulations of a FAST ply; 0 = off: nothing below is read or written
    int cap_permille;      // ply p of game g is FULL when fmix32(key(g) ^ fmix32(p + 0x9E3779B9)) % 1000 < cap_permille
    int *s_budget;         // [B] written by k_begin for the slot's ply: +S = a FULL ply, -cap_fast = a FAST one (no root noise)
    u64 *cp_board;         // [B][8] / [B][4] staging of k_refill's full-first partition: board; game, ply, player, last
    int *cp_state;
    // --- opt-in forced playouts and policy target pruning (az_set_forced_playouts): noised roots only, 0.0 on every other path ---
    double forced_k;       // root child c is forced while n_c^2 < forced_k * P[c] * (parent count); 0.0 = off: nothing new is executed
    int forced_prune;      // k_move makes pi and the move from the pruned counts N' (the record's visits stay the raw ones)
    // --- opt-in Gumbel root search (az_set_gumbel): noised roots only, gumbel_m = 0 on every other path ---
    int gumbel_m;          // candidates sampled without replacement; 0 = off: nothing below is read or written
    double gumbel_cv, gumbel_cs;       // sigma(q) = (c_visit + max N) * c_scale * q
    const unsigned short *gumbel_seq;  // [gumbel_m][S] sequential-halving schedules: row k - 1 serves a root with k candidates
    float *root_logits;    // [B][RW] the root's logits by board cell, written when the root evaluation is consumed, read by k_move
    float *root_v;         // [B] ... and the root's value
    // --- opt-in MCTS-Solver (az_set_solver): proof = nullptr on every other path, nothing below is read or written then ---
    unsigned char *proof;  // [B][R][RW] status of every edge, beside the tree like the DEEP in-flight counts; a new row starts all UNKNOWN
    unsigned char *proof_buf;  // the slot's array, as az_set_solver allocated it: proof = proof_buf while the option is on (host side only)
    signed char *root_proof;   // [B] status of the root of the running ply, seen from its side to move
    signed char *rec_proof;    // [G*nn] ... and of every record's root, written by k_move
    unsigned long long *proof_stops;   // [B] simulations that ended on a proven edge (a terminal hit in cnt as well)
    // --- opt-in root threat search (az_set_threat_search, csrc/az_threat.h): threat_edges = nullptr with the option off, nothing below
    // is read, written or executed then.  k_threat writes them for the slot's ply before the root expansion ---
    unsigned char *threat_edges;   // [B][RW] premarked status of every root edge: the SOLVER k_step copies the row in at root expansion
    signed char *threat_root;      // [B] ... and of the root itself
    signed char *threat_depth;     // [B] depth of the win found, 0 = none
    short *threat_move;            // [B] its first move, -1 = none
    int *threat_nodes;             // [B] fours tried; > threat_budget = the search of this root was exhausted
    unsigned long long *threat_stat;   // [B][THREAT_STATS] roots proven WIN / LOSS, block-only roots, exhausted searches, nodes
    signed char *rec_threat;       // [G*nn] threat_depth of every record's root, written by k_move
    int threat_max_depth, threat_budget;
    // --- opt-in selection rule (az_set_selection): sel_cpuct = nullptr with the option off, nothing below is read then.  The SEL
    // tree kernels score an unvisited child V_X - r_X mass_table[visited prior mass] and use c(count) = sel_cpuct[count]; they
    // keep the root's value in root_v (above).  k_move reads sel_cpuct in the pruning pass only ---
    const double *sel_cpuct;       // [S+3] c_puct + factor * log((i + base + 1) / base), beside sqrt_table and indexed like it
    const double *sel_mass;        // [SEL_MASS_STEPS + 1] sqrt(i / SEL_MASS_STEPS)
    double sel_fpu, sel_fpu_root;  // r_X below the root / at the root
    // --- opt-in candidate moves (az_set_candidates): 0 = off, nothing reads it then.  The CAND tree kernels expand, noise and
    // select over the empty cells within this Chebyshev distance of a stone (cand_plane below) ---
    int cand_radius;
};
constexpr int SEL_MASS_STEPS = 4096, SEL_MASS_SHIFT = 12;      // mass is a sum of floor(P * 2^24): 2^24 >> 12 = 4096 steps for a mass of 1
// the visited prior mass of one child, an integer so that the wave sum has no order
__host__ __device__ __forceinline__ unsigned sel_mass_of(float P) { return (unsigned)((double)P * 16777216.0); }
__host__ __device__ __forceinline__ int sel_mass_index(unsigned mass)
{
    const unsigned i = mass >> SEL_MASS_SHIFT;
    return i > (unsigned)SEL_MASS_STEPS ? SEL_MASS_STEPS : (int)i;
}
// what a SEL descent carries from level to level: c(count) of the level, V_X of its node, and this lane's Q of its best child.
// The SEL kernels take one as a last argument of their own (its value is ignored), so that a kernel without the rule declares
// nothing for it and keeps its code instruction for instruction.
struct SelLevel { double cp, vx, bQ; };
template <class... Rest>
__device__ __forceinline__ SelLevel &sel_level(SelLevel &s, Rest &...) { return s; }
// Q of an unvisited child: the node's own value less the reduction (two separate float64 operations)
__host__ __device__ __forceinline__ double sel_unvisited(double vx, double r, double m)
{
    const double red = r * m;
    return vx - red;
}
__device__ __forceinline__ int game_key(const DevState &d, int game) { return (int)(d.game_key0 + d.key_stride * (unsigned)game); }
// az_set_playout_cap's rule, a function of the game's global name and the absolute ply only (the host's az_playout_cap_full)
__device__ __forceinline__ bool cap_full_ply(const DevState &d, int game, int ply)
{
    return az_fmix32((unsigned)game_key(d, game) ^ az_fmix32((unsigned)ply + 0x9E3779B9u)) % 1000u < (unsigned)d.cap_permille;
}

// az_set_forced_playouts: a root child with n visits (in-flight ones included) is forced -- it scores +infinity instead of its
// PUCT value -- while n^2 < (k P) total.  No sqrt: exact in float64, and a 16-bit count squared would overflow an int.
__host__ __device__ __forceinline__ bool forced_child(double n, double k, float P, int total)
{
    return n * n < (k * (double)P) * (double)total;
}

// ... and policy target pruning, shared by k_move and the host's az_forced_prune.  score(c, m) = Q_c + ((c_puct P_c) sq) / (1 + m) is
// the child's PUCT value had it m visits, Q_c held fixed; it is monotone non-increasing in m (correctly rounded division and
// addition are monotone), so the smallest m of a range with score < target is found by bisection.
__host__ __device__ __forceinline__ double forced_score(double Q, double c_puct, float P, double sq, int m)
{
    return Q + ((c_puct * (double)P) * sq) / (double)(1 + m);
}
// N' of one child other than a* with n > 0 visits: at most F = ceil(sqrt((k P) total)) of them -- what the forced rule could have
// given it -- are taken back, down to the smallest count whose score is still below `target`; a child left with one is emptied
__host__ __device__ inline int forced_pruned(double k, double c_puct, double Q, float P, int n, int total, double sq, double target)
{
    if (forced_score(Q, c_puct, P, sq, n) >= target) return n;
    const double thr = (k * (double)P) * (double)total;
    int lo = 0, hi = n;                                       // score(hi) < target holds
    if (thr < (double)n * (double)n) {                        // else F >= n: every visit may go
        int F = thr > 0.0 ? (int)sqrt(thr) : 0;               // a guess, then made exact: the smallest F >= 0 with F * F >= thr
        while (F > 0 && (double)(F - 1) * (double)(F - 1) >= thr) F--;
        while ((double)F * (double)F < thr) F++;
        lo = n - F;
    }
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (forced_score(Q, c_puct, P, sq, mid) < target) hi = mid; else lo = mid + 1;
    }
    return (lo == 1 && lo < n) ? 0 : lo;
}

// az_set_gumbel (Danihelka et al., ICLR 2022): the scalar pieces of the root rule, shared by the tree kernels, k_move and the host's
// az_gumbel_target.  Every operation is a separate float64 one (the build keeps -ffp-contract=off).
__host__ __device__ __forceinline__ double gumbel_sigma(double c_visit, double c_scale, int max_n)
{
    return (c_visit + (double)max_n) * c_scale;
}
// score = h + sig q (selection and move: h = g + logit; policy target: h = logit, q completed with v_mix)
__host__ __device__ __forceinline__ double gumbel_score(double h, double sig, double q)
{
    const double t = sig * q;
    return h + t;
}
__host__ __device__ __forceinline__ double gumbel_vmix(float v0, double sum_n, double pv, double pq)
{
    return ((double)v0 + (sum_n / pv) * pq) / (1.0 + sum_n);
}

template <int N>
struct TreeGeo {
    static constexpr int n = N, nn = N * N, RW = ((nn + 63) / 64) * 64, CPL = RW / 64, PATH = nn + 1;
};

__device__ __forceinline__ void wave_mem_sync()
{
    // orders this wave's global/LDS writes before its later reads (cross-lane hand-off inside one wave)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------
// Candidate moves (az_set_candidates, the rule is in include/az_engine.h): C(X) = the empty cells within Chebyshev distance
// `radius` of a stone, every cell of an empty board.  A separable dilation of the occupancy on the 4 x u64 plane: `radius`
// steps of one column to either side (the column masks keep a row's end out of its neighbour row), then `radius` steps of
// one row up and down (256-bit shifts by N), every step clipped to the n*n bits of the board; less the stones.  The plane
// and the loop count are wave-uniform, the words are named (no run-time index), so all of it is scalar work.
// ------------------------------------------------------------------------------------------------
template <int N>
struct CandGeo {
    // word q of: the board's n*n bits less column `skip` (-1: less nothing)
    static constexpr u64 keep(int q, int skip)
    {
        u64 m = 0ull;
        for (int b = 0; b < 64; b++) {
            const int j = 64 * q + b;
            if (j < N * N && j % N != skip) m |= 1ull << b;
        }
        return m;
    }
    static constexpr u64 B0 = keep(0, -1), B1 = keep(1, -1), B2 = keep(2, -1), B3 = keep(3, -1);                  // the board
    static constexpr u64 L0 = keep(0, 0), L1 = keep(1, 0), L2 = keep(2, 0), L3 = keep(3, 0);                      // ... less column 0
    static constexpr u64 R0 = keep(0, N - 1), R1 = keep(1, N - 1), R2 = keep(2, N - 1), R3 = keep(3, N - 1);      // ... less the last column
};
template <int N>
__device__ __forceinline__ Plane cand_plane(const Plane &occ, int radius)
{
    typedef CandGeo<N> C;
    Plane h = occ;
    if ((occ.w[0] | occ.w[1] | occ.w[2] | occ.w[3]) == 0ull) {
        h.w[0] = C::B0; h.w[1] = C::B1; h.w[2] = C::B2; h.w[3] = C::B3;
        return h;
    }
    for (int s = 0; s < radius; s++) {                        // one column to the right (<< 1) and to the left (>> 1)
        Plane t;
        t.w[0] = ((h.w[0] << 1) & C::L0) | (((h.w[0] >> 1) | (h.w[1] << 63)) & C::R0);
        t.w[1] = (((h.w[1] << 1) | (h.w[0] >> 63)) & C::L1) | (((h.w[1] >> 1) | (h.w[2] << 63)) & C::R1);
        t.w[2] = (((h.w[2] << 1) | (h.w[1] >> 63)) & C::L2) | (((h.w[2] >> 1) | (h.w[3] << 63)) & C::R2);
        t.w[3] = (((h.w[3] << 1) | (h.w[2] >> 63)) & C::L3) | ((h.w[3] >> 1) & C::R3);
        h.w[0] |= t.w[0]; h.w[1] |= t.w[1]; h.w[2] |= t.w[2]; h.w[3] |= t.w[3];
    }
    for (int s = 0; s < radius; s++) {                        // one row down (<< N) and up (>> N)
        Plane t;
        t.w[0] = ((h.w[0] << N) | (h.w[0] >> N) | (h.w[1] << (64 - N))) & C::B0;
        t.w[1] = ((h.w[1] << N) | (h.w[0] >> (64 - N)) | (h.w[1] >> N) | (h.w[2] << (64 - N))) & C::B1;
        t.w[2] = ((h.w[2] << N) | (h.w[1] >> (64 - N)) | (h.w[2] >> N) | (h.w[3] << (64 - N))) & C::B2;
        t.w[3] = ((h.w[3] << N) | (h.w[2] >> (64 - N)) | (h.w[3] >> N)) & C::B3;
        h.w[0] |= t.w[0]; h.w[1] |= t.w[1]; h.w[2] |= t.w[2]; h.w[3] |= t.w[3];
    }
    h.w[0] &= ~occ.w[0]; h.w[1] &= ~occ.w[1]; h.w[2] &= ~occ.w[2]; h.w[3] &= ~occ.w[3];
    return h;
}
// What a CAND kernel keeps beside the shared body: C(X) of the level being selected, and of the node being expanded.  Like
// SelLevel it is a last kernel argument of the CAND kernels only (its value is ignored), so that a kernel without the option
// declares nothing for it and keeps its code.
struct CandLevel { Plane lvl, exp; };
template <class... Rest>
__device__ __forceinline__ CandLevel &cand_level(CandLevel &c, Rest &...) { return c; }
// cell j is in the level's / the expanded node's plane; the overloads without a CandLevel are never called for their value
template <class... A> __device__ __forceinline__ bool cand_lvl(int, A &...) { return false; }
template <class... A> __device__ __forceinline__ bool cand_lvl(int j, CandLevel &c, A &...) { return pl_get(c.lvl, j); }
template <class... A> __device__ __forceinline__ bool cand_exp(int, A &...) { return false; }
template <class... A> __device__ __forceinline__ bool cand_exp(int j, CandLevel &c, A &...) { return pl_get(c.exp, j); }
// The root's Dirichlet mix under CAND: the tape and legal_rank stay, the sample is cut down to the candidates and renormalised
// by its float64 canonical wave sum (lane partials over its cells in ascending order, then the butterfly); nothing is fused.
template <int CPL>
__device__ __forceinline__ void cand_mix_noise(const DevState &d, const Plane &occ, const Plane &cand, const double *nz, int lane,
                                               float (&P)[CPL])
{
    double nc[CPL], part = 0.0;
#pragma unroll
    for (int i = 0; i < CPL; i++) {
        const int j = lane + 64 * i;
        nc[i] = 0.0;
        if (pl_get(cand, j)) {
            nc[i] = nz[j - pl_rank(occ, j)];
            part = part + nc[i];
        }
    }
    const double t = wave_sum_butterfly_d(part);
#pragma unroll
    for (int i = 0; i < CPL; i++) {
        if (pl_get(cand, lane + 64 * i)) {
            const float scaled = d.one_minus_w * P[i];
            const double share = nc[i] / t;
            P[i] = (float)((double)scaled + d.w_noise * share);
        }
    }
}


// ------------------------------------------------------------------------------------------------
// Evaluation cache (opt-in; the reference only names it: mcts.py:17 DEFAULT_CACHE_SIZE = 500_000, mcts.py:22 "TODO: add
// caching").  Key = what the net sees: mover planes, opponent planes, last move (games.py:86-129 encode) + which net +
// the weights generation.  Value = the net's raw outputs for that input, policy logits and value-head hidden row, i.e.
// exactly the floats the trunk + FC kernels would produce again, so a hit changes nothing downstream (visit counts are
// bit-identical with the cache on or off).  Direct-mapped table in HBM shared by every lane of the engine; entries are
// written and read by whole wavefronts with plain loads/stores and carry a checksum bound to the key: an entry torn by
// a concurrent writer (another lane's kernel) fails the check and counts as a miss.
//   entry = [9 x u64 key][u64 checksum][pad to 128 B][RW logits][64 hidden]
// ------------------------------------------------------------------------------------------------
constexpr int CACHE_HDR = 32;      // floats
template <int N>
struct CacheGeo {
    static constexpr int CES = CACHE_HDR + TreeGeo<N>::RW + 64;     // floats per entry
};
__device__ __forceinline__ u64 cache_mix(u64 h, u64 v)
{
    h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return h;
}
__device__ __forceinline__ u64 cache_key8(int last, int net, unsigned gen)
{
    return (u64)(unsigned)(last + 1) | ((u64)(unsigned)net << 16) | ((u64)gen << 32);
}
__device__ __forceinline__ u64 cache_hash(const Plane &me, const Plane &opp, u64 k8)
{
    u64 h = 0x243F6A8885A308D3ull;
#pragma unroll
    for (int q = 0; q < 4; q++) h = cache_mix(h, me.w[q]);
#pragma unroll
    for (int q = 0; q < 4; q++) h = cache_mix(h, opp.w[q]);
    return cache_mix(h, k8);
}
// the key word lane `lane` (0..8) is responsible for
__device__ __forceinline__ u64 cache_keyword(const Plane &me, const Plane &opp, u64 k8, int lane)
{
    u64 w = k8;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        w = lane == q ? me.w[q] : w;
        w = lane == 4 + q ? opp.w[q] : w;
    }
    return w;
}
template <int CPL>
__device__ __forceinline__ u64 cache_checksum(const float (&x)[CPL], float h, int lane, u64 hsh)
{
    unsigned a = 0u, b = 0u;
#pragma unroll
    for (int i = 0; i <= CPL; i++) {
        const unsigned w = __float_as_uint(i < CPL ? x[i < CPL ? i : 0] : h);
        const unsigned pos = (unsigned)(lane + 64 * i);
        a ^= az_fmix32(w + pos * 0x9E3779B1u);
        b ^= az_fmix32((w ^ 0xA5A5A5A5u) + pos * 0x85EBCA77u + 0x5BD1E995u);
    }
    a = wave_xor_u(a);
    b = wave_xor_u(b);
    return ((((u64)a) << 32) | (u64)b) ^ hsh;
}
// wave-uniform call: true = the entry of (me, opp, last, net) was found intact; its rows are then in x / h
template <int N>
__device__ __forceinline__ bool cache_lookup(const DevState &d, const Plane &me, const Plane &opp, int last, int net, int lane,
                                             float (&x)[TreeGeo<N>::CPL], float &h)
{
    typedef TreeGeo<N> G;
    const u64 k8 = cache_key8(last, net, d.cache_gen);
    const u64 hsh = cache_hash(me, opp, k8);
    const float *ent = d.cache + (size_t)((unsigned)hsh & d.cache_mask) * CacheGeo<N>::CES;
    const u64 *kp = reinterpret_cast<const u64 *>(ent);
    const u64 mine = cache_keyword(me, opp, k8, lane);
    const u64 got = lane < 10 ? kp[lane] : 0ull;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) x[i] = ent[CACHE_HDR + lane + 64 * i];
    h = ent[CACHE_HDR + G::RW + lane];
    const bool key_ok = __ballot(lane < 9 && got != mine) == 0ull;
    const u64 cs = cache_checksum<G::CPL>(x, h, lane, hsh);
    const u64 stored = (u64)__shfl((long long)got, 9, 64);
    return key_ok && cs == stored;
}
template <int N>
__device__ __forceinline__ void cache_insert(const DevState &d, const Plane &me, const Plane &opp, int last, int net, int lane,
                                             const float (&x)[TreeGeo<N>::CPL], float h)
{
    typedef TreeGeo<N> G;
    const u64 k8 = cache_key8(last, net, d.cache_gen);
    const u64 hsh = cache_hash(me, opp, k8);
    float *ent = d.cache + (size_t)((unsigned)hsh & d.cache_mask) * CacheGeo<N>::CES;
    u64 *kp = reinterpret_cast<u64 *>(ent);
    const u64 cs = cache_checksum<G::CPL>(x, h, lane, hsh);
    const u64 mine = lane == 9 ? cs : cache_keyword(me, opp, k8, lane);
    if (lane < 10) kp[lane] = mine;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) ent[CACHE_HDR + lane + 64 * i] = x[i];
    ent[CACHE_HDR + G::RW + lane] = h;
}

// With random-symmetry leaf evaluation (az_set_leaf_symmetry) the net's outputs depend on the symmetry it was shown, so the
// symmetry is part of the key (folded into the net field), and a hit lands in the logits row the way the net would have written
// it -- in image coordinates, board cell j at image cell sym_src(t^-1, j) -- because the tree step maps every row back.
__device__ __forceinline__ int cache_net_key(int net, int sym) { return net | (sym << 1); }
template <int N>
__device__ __forceinline__ void cache_hit_store(float *lg, const float (&cx)[TreeGeo<N>::CPL], int lane, bool sym_on, int sym)
{
    typedef TreeGeo<N> G;
    if (sym_on) {
        const int ti = sym_inverse(sym);
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            const int j = lane + 64 * i, r = j / N;
            if (j < G::nn) lg[sym_src(ti, r, j - r * N, N)] = cx[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < G::CPL; i++) lg[lane + 64 * i] = cx[i];
    }
}

// controller.py:49 softmax over all n^2 logits (no legality mask) in the canonical wave order, and the
// value tail value_fc2 + tanh (net.py:70) as one k-ordered fma chain.  P[i] is the prior of cell lane+64*i.
template <int N>
__device__ __forceinline__ void eval_tail(const DevState &d, int b, int lane, float (&P)[TreeGeo<N>::CPL], float &v)
{
    typedef TreeGeo<N> G;
    const float *lg = d.logits + (size_t)b * G::RW;
    float x[G::CPL];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        int j = lane + 64 * i;
        x[i] = j < G::nn ? lg[j] : -INFINITY;
        mx = fmaxf(mx, x[i]);
    }
    mx = wave_max_f(mx);
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        int j = lane + 64 * i;
        P[i] = 0.0f;
        if (j < G::nn) {
            P[i] = az_expf(x[i] - mx);
            part = part + P[i];
        }
    }
    float s = wave_sum_butterfly(part);
#pragma unroll
    for (int i = 0; i < G::CPL; i++) P[i] = P[i] / s;
    const float *h = d.vhid + (size_t)b * 64;
    const float *w2 = d.v2w[d.s_net[b]];
    float acc = 0.0f;
    for (int i = 0; i < 64; i++) acc = __builtin_fmaf(h[i], w2[i], acc);
    v = az_tanhf(acc + d.v2b[d.s_net[b]][0]);
}

// az_net_eval: softmax policy + value for boards staged as pending leaves (controller.py:39-53)
template <int N>
__global__ __launch_bounds__(256) void k_eval_tail(DevState d, int count, float *policy, float *value)
{
    typedef TreeGeo<N> G;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= count) return;
    float P[G::CPL], v;
    eval_tail<N>(d, b, lane, P, v);
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        int j = lane + 64 * i;
        if (j < G::nn) policy[(size_t)b * G::nn + j] = P[i];
    }
    if (lane == 0) value[b] = v;
}

#ifdef AZ_ENGINE_TU   // size-independent kernels live in the engine translation unit only
// ------------------------------------------------------------------------------------------------
// k_begin: the root of every active slot becomes the pending evaluation (mcts.py:106-109)
// ------------------------------------------------------------------------------------------------
__global__ void k_begin(DevState d)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.B) return;
    const int L = d.L;
    const size_t it = (size_t)b * L;                     // evaluation items of this game: the root is item 0
    if (d.s_status[b] != SLOT_ACTIVE) {
        for (int j = 0; j < L; j++) {
            d.leaf_kind[it + j] = LEAF_NONE;
            if (L > 1) d.it_status[it + j] = SLOT_IDLE;
        }
        return;
    }
    int pl = d.s_player[b];
    const u64 *bd = d.board + (size_t)b * 8;
    u64 *lf = d.leaf + it * 8;
    for (int i = 0; i < 4; i++) {
        lf[i] = pl == 1 ? bd[i] : bd[4 + i];
        lf[4 + i] = pl == 1 ? bd[4 + i] : bd[i];
    }
    d.leaf_last[it] = d.s_last[b];
    if (d.cap_fast) d.s_budget[b] = cap_full_ply(d, d.s_game[b], d.s_ply[b]) ? d.S : -d.cap_fast;   // this ply's simulations
    if (d.leaf_sym) d.leaf_sym[it] = leaf_sym_of(game_key(d, d.s_game[b]), d.s_ply[b], 0);
    d.leaf_kind[it] = (d.reuse && d.carried[b] >= 0) ? LEAF_REUSE : LEAF_ROOT;
    d.depth[it] = 0;
    const int netid = d.arena ? (pl == 1 ? 0 : 1) : 0;   // evaluator.py:73-79: each side searches with its own net
    d.s_net[b] = netid;
    for (int j = 1; j < L; j++) d.leaf_kind[it + j] = LEAF_NONE;
    if (L > 1)
        for (int j = 0; j < L; j++) { d.it_status[it + j] = SLOT_ACTIVE; d.it_net[it + j] = netid; }
}

#endif  // AZ_ENGINE_TU

// ------------------------------------------------------------------------------------------------
// k_step: consume the evaluation of the pending leaf (expand + backup), then select the next leaf.
// Latency-bound (one wave per game, ~4 waves per CU): every load that does not depend on another load is
// issued up front in one round trip; the sqrt table lives in LDS; the chosen edge is broadcast by shuffle.
// Dynamic LDS: (S + 2) doubles.  DEEP (S > DEFAULT_MAX_S): no LDS table; each level's sqrt(N_parent + 1e-8) is read from
// the global table (L2-resident) right after the chosen edge is known, so it is in flight with that level's win test
// and the next level's edge loads (same values: results are bit-identical).
// ------------------------------------------------------------------------------------------------
// SOLVER (az_set_solver): instantiations of their own, so that the default ones keep their code.  One status byte per edge
// beside the tree (d.proof).  Selection masks the scores with the row's statuses (a WIN edge +inf, a LOSS edge -inf while
// the row has a legal edge that is not LOSS: one more wave vote per level); a descent that lands on a proven edge ends there
// like a terminal; and the launch that backs a real terminal up whose edge was still UNKNOWN marks that edge and walks the
// path upwards, replaying the occupancy of each level from the root planes and the path (proof_mark).  A simulation that
// ends in an expansion only pays for the status loads.
constexpr int STEP_WAVES = 4;      // games (wavefronts) per k_step workgroup

// the status of a node, seen from its side to move, from this lane's CPL statuses of its row: WIN if any legal edge is WIN,
// else DRAW / LOSS once every legal edge is proven
template <int N>
__device__ __forceinline__ int proof_node(const int (&st)[TreeGeo<N>::CPL], const Plane &occ, int lane)
{
    typedef TreeGeo<N> G;
    bool anyw = false, anyd = false, anyu = false;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        const int j = lane + 64 * i;
        if (j < G::nn && !pl_get(occ, j)) {
            anyw = anyw || st[i] == PROOF_WIN;
            anyd = anyd || st[i] == PROOF_DRAW;
            anyu = anyu || st[i] == PROOF_UNKNOWN;
        }
    }
    if (__ballot(anyw)) return PROOF_WIN;
    if (__ballot(anyu)) return PROOF_UNKNOWN;
    return __ballot(anyd) ? PROOF_DRAW : PROOF_LOSS;
}

// The marking walk (wave-uniform).  The simulation whose path[0 .. depth) is given ended on a real terminal: `status` (WIN:
// the move made the line, DRAW: it filled the board) goes to its last edge when that edge is still UNKNOWN, and upwards as
// long as the owning node's status is known.  occ0 = the root's occupancy.  prf = this slot's statuses, RS bytes per row (the
// HBM array pads a row to RW, k_search's LDS copy does not).  Returns the root's status when the walk reaches it, else UNKNOWN.
template <int N, int RS = TreeGeo<N>::RW>
__device__ __forceinline__ int proof_mark(unsigned char *prf, const unsigned *path, int depth, Plane occ0, int status, int lane)
{
    typedef TreeGeo<N> G;
    if (depth < 1 || depth > G::nn) return PROOF_UNKNOWN;
    const unsigned last = path[depth - 1];
    if (prf[(size_t)(last >> 16) * RS + (last & 0xFFFFu)] != PROOF_UNKNOWN) return PROOF_UNKNOWN;
    Plane occ = occ0;                                         // the occupancy of level depth - 1: the root's and the moves above it
    for (int dd = 0; dd < depth - 1; dd++) pl_set(occ, (int)(path[dd] & 0xFFFFu));
    for (int lvl = depth - 1; lvl >= 0; lvl--) {
        const unsigned pe = path[lvl];
        const int cell = (int)(pe & 0xFFFFu);
        unsigned char *row = prf + (size_t)(pe >> 16) * RS;
        int st[G::CPL];
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            const int j = lane + 64 * i;
            st[i] = j == cell ? status : (j < G::nn ? (int)row[j] : PROOF_UNKNOWN);
        }
        if (lane == 0) row[cell] = (unsigned char)status;
        const int ns = proof_node<N>(st, occ, lane);
        if (ns == PROOF_UNKNOWN) return PROOF_UNKNOWN;
        if (lvl == 0) return ns;
        status = proof_negate(ns);
        const int up = (int)(path[lvl - 1] & 0xFFFFu);        // the level above had this cell still empty
        const u64 bit = 1ull << (up & 63);
#pragma unroll
        for (int q = 0; q < 4; q++) occ.w[q] &= (up >> 6) == q ? ~bit : ~0ull;
    }
    return PROOF_UNKNOWN;
}

// SEL (az_set_selection): instantiations of their own as well, never together with SOLVER.  Per level one 32-bit wave sum (the
// visited prior mass), two uniform table reads from HBM (c(count) beside the sqrt, issued with it; the mass table once the
// sum is known) and the chosen edge's Q carried down as the next node's value; the root's value stays in d.root_v for the ply.
// CAND (az_set_candidates): instantiations of their own again, never together with SOLVER or SEL.  The root's and every leaf's
// softmax, the root's noise and every level's argmax run over the node's candidate plane (cand_plane) instead of the board /
// the empty cells; the plane is formed from the position where it is needed, per expansion and per level of the descent.
template <int N, bool SYNTH, bool DEEP = false, bool SOLVER = false, bool SEL = false, bool CAND = false, class... Sel>
__global__ __launch_bounds__(STEP_WAVES * 64) void k_step(DevState d, int rootN, int do_select, Sel... sel)
{
    static_assert(sizeof...(Sel) == (SEL || CAND ? 1 : 0) && !(SEL && SOLVER), "the SEL kernels take a SelLevel; never with SOLVER");
    static_assert(!(CAND && (SEL || SOLVER)), "the CAND kernels take a CandLevel; they carry neither the solver nor the selection rule");
    typedef TreeGeo<N> G;
    extern __shared__ double sq_lds[];                 // np.sqrt(N + 1e-8), N = 0..S+1 (mcts.py:73)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * STEP_WAVES + (threadIdx.x >> 6);
    const bool inb = b < d.B;
    const int bb = inb ? b : 0;
    if constexpr (!DEEP)
        for (int i = threadIdx.x; i < d.S + 2; i += STEP_WAVES * 64) sq_lds[i] = d.sqrt_table[i];

    // ---- independent loads, all in flight together ----
    const int status = d.s_status[bb];
    const int kind_raw = d.leaf_kind[bb];
    // a cache hit (LEAF_*_HIT) is consumed exactly like the evaluation it stands for; it is just not inserted again
    const int kind = kind_raw == LEAF_EXPAND_HIT ? LEAF_EXPAND : (kind_raw == LEAF_ROOT_HIT ? LEAF_ROOT : kind_raw);
    const int depth0 = d.depth[bb];
    const int rows0 = d.rows_used[bb];
    const int pl = d.s_player[bb];
    const int slast = d.s_last[bb];
    const int netid = d.s_net[bb];
    const int leaf_last = d.leaf_last[bb];
    const int game = d.s_game[bb];
    const int ply = d.s_ply[bb];
    const int carried = d.reuse ? d.carried[bb] : -1;
    const int budget_raw = d.cap_fast ? d.s_budget[bb] : d.S;     // playout cap (kernel-argument test, uniform): < 0 = a FAST ply
    const Plane lme = pl_load(d.leaf + (size_t)bb * 8), lopp = pl_load(d.leaf + (size_t)bb * 8 + 4);
    const Plane bX = pl_load(d.board + (size_t)bb * 8), bO = pl_load(d.board + (size_t)bb * 8 + 4);
    unsigned *path = d.path + (size_t)bb * G::PATH;
    const unsigned path_l = path[lane];                // PATH = n*n+1 >= 26 entries; lanes beyond read a neighbour's slot (unused)
    float x[G::CPL];
    float h_l = 0.0f, w2a = 0.0f, w2b = 0.0f, b2a = 0.0f, b2b = 0.0f;
    if (!SYNTH) {
        const float *lg = d.logits + (size_t)bb * G::RW;
        if (d.leaf_sym) {
            // the net saw the leaf under symmetry t: board cell j sits at image cell sym_src(t^-1, j)
            const int ti = sym_inverse(d.leaf_sym[bb]);
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                const int j = lane + 64 * i, r = j / N;
                x[i] = j < G::nn ? lg[sym_src(ti, r, j - r * N, N)] : 0.0f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < G::CPL; i++) x[i] = lg[lane + 64 * i];
        }
        h_l = d.vhid[(size_t)bb * 64 + lane];
        if (d.v2w[0]) { w2a = d.v2w[0][lane]; b2a = d.v2b[0][0]; }
        if (d.v2w[1]) { w2b = d.v2w[1][lane]; b2b = d.v2b[1][0]; }
    }
    __syncthreads();
    if (!inb || status != SLOT_ACTIVE) return;
    Edge *rows = d.edges + (size_t)b * d.R * G::RW;
    const int budget = budget_raw < 0 ? -budget_raw : budget_raw;     // simulations of this slot's ply: S unless the cap says less
    const bool root_noise = d.add_noise && budget_raw > 0;            // a FAST ply uses the priors as they are
    const bool gumbel = !SYNTH && !CAND && d.gumbel_m > 0 && root_noise;      // Gumbel root search (kernel-argument test, uniform): the noised root only

    // ---------------- stage 1: evaluation -> expand -> backup ----------------
    if (kind == LEAF_REUSE) {
        // retained root: its row (compacted to row 0 by k_move) already holds the un-noised priors and the visit
        // statistics of the previous search; only the fresh Dirichlet sample is mixed in (same arithmetic as a new root)
        if (d.add_noise) {
            Plane occ;
#pragma unroll
            for (int q = 0; q < 4; q++) occ.w[q] = bX.w[q] | bO.w[q];
            const double *nz = d.noise + (size_t)game * d.noise_stride + d.noise_off[ply];
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                int j = lane + 64 * i;
                if (j < G::nn && !pl_get(occ, j)) {
                    int rank = j - pl_rank(occ, j);
                    Edge *e = rows + j;
                    float scaled = d.one_minus_w * e->P;
                    e->P = (float)((double)scaled + d.w_noise * nz[rank]);
                }
            }
        }
        if (lane == 0) d.cnt[(size_t)b * CNT_STRIDE + 4] += 1ull;
        wave_mem_sync();
    } else if (kind != LEAF_NONE) {
        float v = 0.0f;
        if (kind == LEAF_ROOT || kind == LEAF_EXPAND) {
            float P[G::CPL];
            if constexpr (CAND) {                             // C(X) of the node being expanded
                Plane occx;
#pragma unroll
                for (int q = 0; q < 4; q++) occx.w[q] = lme.w[q] | lopp.w[q];
                cand_level(sel...).exp = cand_plane<N>(occx, d.cand_radius);
            }
            if (SYNTH) {
                // build-owned deterministic evaluator (test hook behind the policy_value_fn seam, mcts.py:87-93)
                unsigned hx = 0;
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    int j = lane + 64 * i;
                    if (j < G::nn) {
                        unsigned code = pl_get(lme, j) ? 1u : (pl_get(lopp, j) ? 2u : 0u);
                        hx ^= az_fmix32((unsigned)j * 3u + code + 0x9E3779B9u);
                    }
                }
                unsigned hs = wave_xor_u(hx);
                hs ^= az_fmix32(0x51ED270Bu + (unsigned)(leaf_last + 1));
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    int j = lane + 64 * i;
                    unsigned r = az_fmix32(hs + (unsigned)(j + 1) * 0x9E3779B1u);
                    P[i] = (float)(((r >> 8) & 0xFFFFu) + 1u) * 0x1p-23f;
                }
                int vv = (int)(az_fmix32(hs ^ 0x7F4A7C15u) & 0x1FFu);
                v = (float)(vv - 256) / 256.0f;
                if constexpr (CAND) {                         // not normalised: candidates keep their prior, every other cell gets 0
#pragma unroll
                    for (int i = 0; i < G::CPL; i++) P[i] = cand_exp(lane + 64 * i, sel...) ? P[i] : 0.0f;
                }
            } else {
                if (d.cache && kind_raw == kind) {            // a fresh evaluation: remember it
                    float xc[G::CPL];
#pragma unroll
                    for (int i = 0; i < G::CPL; i++) xc[i] = lane + 64 * i < G::nn ? x[i] : 0.0f;
                    cache_insert<N>(d, lme, lopp, leaf_last, cache_net_key(netid, d.leaf_sym ? d.leaf_sym[bb] : 0), lane, xc, h_l);
                }
                if (d.ext_eval) {
                    // the evaluator lives outside the engine (policy_value_fn seam, mcts.py:87-93,109,137): the row holds
                    // the priors it returned, as they are, and the first hidden entry its value
#pragma unroll
                    for (int i = 0; i < G::CPL; i++) P[i] = lane + 64 * i < G::nn ? x[i] : 0.0f;
                    v = __shfl(h_l, 0, 64);
                } else {
                // controller.py:49 softmax over all n^2 logits (no legality mask), canonical wave order; CAND: over C(X)
                float mx = -INFINITY;
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    if (CAND ? !cand_exp(lane + 64 * i, sel...) : lane + 64 * i >= G::nn) x[i] = -INFINITY;
                    mx = fmaxf(mx, x[i]);
                }
                mx = wave_max_f(mx);
                float part = 0.0f;
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    P[i] = 0.0f;
                    if (CAND ? cand_exp(lane + 64 * i, sel...) : lane + 64 * i < G::nn) {
                        P[i] = az_expf(x[i] - mx);
                        part = part + P[i];
                    }
                }
                const float ssum = wave_sum_butterfly(part);
#pragma unroll
                for (int i = 0; i < G::CPL; i++) P[i] = P[i] / ssum;
                // value tail: value_fc2 + tanh (net.py:70), one k-ordered fma chain over the lane-held operands
                const float w2_l = netid ? w2b : w2a;
                const float acc = value_fc2_chain(h_l, w2_l);
                v = az_tanhf(acc + (netid ? b2b : b2a));
                }
            }
            if (kind == LEAF_ROOT && gumbel) {
                // az_set_gumbel: the edges keep the plain softmax priors; the root's logits (by board cell) and value stay with
                // the slot for the selections of this ply and for k_move
#pragma unroll
                for (int i = 0; i < G::CPL; i++) d.root_logits[(size_t)b * G::RW + lane + 64 * i] = lane + 64 * i < G::nn ? x[i] : 0.0f;
                if (lane == 0) d.root_v[b] = v;
            } else if (kind == LEAF_ROOT && root_noise) {
                // mcts.py:113-116; float32 multiply, float64 add, float32 store
                Plane occ;
#pragma unroll
                for (int q = 0; q < 4; q++) occ.w[q] = lme.w[q] | lopp.w[q];
                const double *nz = d.noise + (size_t)game * d.noise_stride + d.noise_off[ply];
                if constexpr (CAND) {
                    cand_mix_noise<G::CPL>(d, occ, cand_level(sel...).exp, nz, lane, P);
                } else {
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    int j = lane + 64 * i;
                    if (j < G::nn && !pl_get(occ, j)) {
                        int rank = j - pl_rank(occ, j);
                        float scaled = d.one_minus_w * P[i];
                        P[i] = (float)((double)scaled + d.w_noise * nz[rank]);
                    }
                }
                }
            }
            if constexpr (SEL) {
                // az_set_selection: the value the root's evaluation gave (net, cache hit, synthetic or external alike)
                if (kind == LEAF_ROOT && lane == 0) d.root_v[b] = v;
            }
            // mcts.py:50-64 expand: one edge per cell (occupied cells are never selected)
            const int row = kind == LEAF_ROOT ? 0 : rows0;
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                int j = lane + 64 * i;
                Edge e;
                e.W = 0.0; e.P = P[i]; e.N = 0; e.child = 0;
                rows[(size_t)row * G::RW + j] = e;
            }
            if constexpr (SOLVER) {
                // a new row starts with every edge UNKNOWN, and a new root with its own status UNKNOWN
                unsigned char *prow = d.proof + ((size_t)b * d.R + row) * G::RW;
#pragma unroll
                for (int i = 0; i < G::CPL; i++) prow[lane + 64 * i] = PROOF_UNKNOWN;
                if (kind == LEAF_ROOT && lane == 0) d.root_proof[b] = PROOF_UNKNOWN;
                // az_set_threat_search: a root starts from the statuses the threat search premarked (a test of the pointer, the root only)
                if (kind == LEAF_ROOT && d.threat_edges) {
                    const unsigned char *pre = d.threat_edges + (size_t)b * G::RW;
#pragma unroll
                    for (int i = 0; i < G::CPL; i++) prow[lane + 64 * i] = pre[lane + 64 * i];
                    if (lane == 0) d.root_proof[b] = d.threat_root[b];
                }
            }
            if (lane == 0) d.rows_used[b] = row + 1;
            if (kind == LEAF_EXPAND) {
                const unsigned pe = depth0 - 1 < 64 ? (unsigned)__shfl((int)path_l, depth0 - 1, 64) : path[depth0 - 1];
                if (lane == 0) rows[(size_t)(pe >> 16) * G::RW + (pe & 0xFFFFu)].child = (unsigned short)row;
            }
        }
        if (kind != LEAF_ROOT) {
            // mcts.py:132-134,141,76-82: value w.r.t. the side to move at the leaf, backed up with alternating sign
            double value = kind == LEAF_EXPAND ? (double)v : (kind == LEAF_TERM_LOSS ? -1.0 : 0.0);
            if constexpr (SOLVER) value = kind == LEAF_TERM_WIN ? 1.0 : value;
            for (int dd = lane; dd < depth0; dd += 64) {
                const unsigned pe = dd < 64 ? path_l : path[dd];
                Edge *e = rows + (size_t)(pe >> 16) * G::RW + (pe & 0xFFFFu);
                const double val = ((depth0 - 1 - dd) & 1) ? value : -value;
                e->N = (unsigned short)(e->N + 1);
                e->W = e->W + val;
            }
            if constexpr (SOLVER) {
                // marking: a real terminal whose edge is still UNKNOWN (a stop on a proven edge never is) proves that edge
                if (kind == LEAF_TERM_LOSS || kind == LEAF_TERM_DRAW) {
                    Plane occ0;
#pragma unroll
                    for (int q = 0; q < 4; q++) occ0.w[q] = bX.w[q] | bO.w[q];
                    const int rs = proof_mark<N>(d.proof + (size_t)b * d.R * G::RW, path, depth0, occ0,
                                                 kind == LEAF_TERM_LOSS ? PROOF_WIN : PROOF_DRAW, lane);
                    if (rs != PROOF_UNKNOWN && lane == 0) d.root_proof[b] = (signed char)rs;
                }
            }
            if (lane == 0) {
                unsigned long long *c = d.cnt + (size_t)b * CNT_STRIDE;
                c[0] += kind == LEAF_EXPAND ? 1ull : 0ull;
                c[1] += 1ull;
                c[2] += kind == LEAF_EXPAND ? 0ull : 1ull;
                c[3] += (unsigned long long)depth0;
            }
        }
        wave_mem_sync();
    }

    // ---------------- stage 2: selection (mcts.py:124-129) ----------------
    // a retained root tops its visits up to S: idle until simulation `carried`; a slot whose budget is spent stays idle
    if (!do_select || rootN < carried || rootN >= budget) {
        if (lane == 0) d.leaf_kind[b] = LEAF_NONE;
        return;
    }
    Plane me = pl == 1 ? bX : bO;
    Plane opp = pl == 1 ? bO : bX;
    int row = 0, npar = rootN, depth = 0, last = slast, out_kind = LEAF_NONE;
    double sq_next = DEEP ? d.sqrt_table[rootN] : 0.0;
    if constexpr (SEL) {                                      // c(count) of the level, read like DEEP's sqrt; V_X of its node
        SelLevel &sl = sel_level(sel...);
        sl.cp = d.sel_cpuct[rootN];
        sl.vx = (double)d.root_v[b];                          // after stage 1's wave_mem_sync: this launch may have written it
    }
    const bool forced = d.forced_k > 0.0 && root_noise;       // forced playouts (kernel-argument test, uniform): the noised root only
    for (;;) {
        Plane occ;
#pragma unroll
        for (int q = 0; q < 4; q++) occ.w[q] = me.w[q] | opp.w[q];
        const double sq = DEEP ? sq_next : sq_lds[npar];      // np.sqrt(self.N + 1e-8), mcts.py:73
        if constexpr (CAND) cand_level(sel...).lvl = cand_plane<N>(occ, d.cand_radius);     // C(X) of this level's node, from its position
        double best = 0.0;
        int bi = -1, bN = 0, bC = 0, bS = 0;
        if constexpr (SEL) {
            // az_set_selection: an unvisited child is worth the node's own value less r sqrt(visited prior mass)
            SelLevel &sl = sel_level(sel...);
            Edge er[G::CPL];
            unsigned ms = 0u;
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                const int j = lane + 64 * i;
                if (j < G::nn && !pl_get(occ, j)) {
                    er[i] = rows[(size_t)row * G::RW + j];
                    ms += er[i].N ? sel_mass_of(er[i].P) : 0u;
                }
            }
            ms = (unsigned)wave_sum_i((int)ms);
            const double unv = sel_unvisited(sl.vx, row == 0 ? d.sel_fpu_root : d.sel_fpu, d.sel_mass[sel_mass_index(ms)]);
            sl.bQ = 0.0;
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                const int j = lane + 64 * i;
                if (j < G::nn && !pl_get(occ, j)) {
                    const Edge e = er[i];
                    const double Q = e.N ? e.W / (double)e.N : unv;
                    double sc = Q + ((sl.cp * (double)e.P) * sq) / (double)(1 + (int)e.N);
                    if (forced && row == 0 && forced_child((double)(int)e.N, d.forced_k, e.P, rootN)) sc = INFINITY;
                    if (bi < 0 || sc > best) { best = sc; bi = j; bN = e.N; bC = e.child; sl.bQ = Q; }
                }
            }
        } else if (gumbel && row == 0) {
            // az_set_gumbel: sequential halving at the root.  Among the legal children whose visit count is the schedule's entry
            // for this simulation, the first maximum of (g + logit) + sigma q; they all have equal N, so the choice is exact.
            Edge er[G::CPL];
            unsigned mxn = 0u;
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                const int j = lane + 64 * i;
                if (j < G::nn && !pl_get(occ, j)) {
                    er[i] = rows[j];
                    mxn = (unsigned)er[i].N > mxn ? (unsigned)er[i].N : mxn;
                }
            }
            mxn = wave_max_u(mxn);
            const int kk = min_i(d.gumbel_m, G::nn - pl_count(occ));          // >= 1: an active slot has a legal cell
            const int need = (int)d.gumbel_seq[(size_t)(kk > 0 ? kk - 1 : 0) * d.S + rootN];
            const double sig = gumbel_sigma(d.gumbel_cv, d.gumbel_cs, (int)mxn);
            const double *nz = d.noise + (size_t)game * d.noise_stride + d.noise_off[ply];
            const float *rl = d.root_logits + (size_t)b * G::RW;
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                const int j = lane + 64 * i;
                if (j < G::nn && !pl_get(occ, j) && (int)er[i].N == need) {
                    const double h = nz[j - pl_rank(occ, j)] + (double)rl[j];
                    const double Q = er[i].N ? er[i].W / (double)er[i].N : 0.0;
                    const double sc = gumbel_score(h, sig, Q);
                    if (bi < 0 || sc > best) { best = sc; bi = j; bN = er[i].N; bC = er[i].child; }
                }
            }
        } else {
        int pst[G::CPL];                                      // SOLVER: the row's statuses; the vote: some legal edge is not LOSS
        bool masked = false;
        if constexpr (SOLVER) {
            const unsigned char *prow = d.proof + ((size_t)b * d.R + row) * G::RW;
            bool alive = false;
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                const int j = lane + 64 * i;
                pst[i] = prow[j];
                alive = alive || (j < G::nn && !pl_get(occ, j) && pst[i] != PROOF_LOSS);
            }
            masked = __ballot(alive) != 0ull;                 // every legal edge LOSS (the root only): the plain scores decide
        }
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            int j = lane + 64 * i;
            if (CAND ? cand_lvl(j, sel...) : (j < G::nn && !pl_get(occ, j))) {
                Edge e = rows[(size_t)row * G::RW + j];
                double Q = e.N ? e.W / (double)e.N : 0.0;     // mcts.py:80 Q = W/N (0.0 while unvisited)
                double sc = Q + ((d.c_puct * (double)e.P) * sq) / (double)(1 + (int)e.N);
                if (forced && row == 0 && forced_child((double)(int)e.N, d.forced_k, e.P, rootN)) sc = INFINITY;
                int key = 0;
                if constexpr (SOLVER) {
                    if (pst[i] == PROOF_WIN) sc = INFINITY;
                    else if (pst[i] == PROOF_LOSS && masked) sc = -INFINITY;
                    key = pst[i];
                }
                if (bi < 0 || sc > best) { best = sc; bi = j; bN = e.N; bC = e.child; bS = key; }
            }
        }
        }
        wave_argmax(best, bi);
        const int a = __builtin_amdgcn_readfirstlane(bi);
        if (a < 0) { out_kind = LEAF_NONE; break; }            // unreachable for a non-terminal root; never index with -1
        // the lane that owns cell a (a & 63) holds its edge: the global best is also that lane's best
        const int child = __builtin_amdgcn_readlane(bC, a & 63);
        const int an = __builtin_amdgcn_readlane(bN, a & 63);
        const int ast = SOLVER ? __builtin_amdgcn_readlane(bS, a & 63) : PROOF_UNKNOWN;
        if (DEEP) sq_next = d.sqrt_table[an];                 // the next level's parent visits: issued before the win test
        if constexpr (SEL) {
            SelLevel &sl = sel_level(sel...);
            sl.cp = d.sel_cpuct[an];
            sl.vx = -lane_d(sl.bQ, a & 63);                   // the node below, for its side to move (the edge has a visit when a row hangs on it)
        }
        if (lane == 0) path[depth] = ((unsigned)row << 16) | (unsigned)a;
        depth++;
        pl_set(me, a);                                        // games.py:79-81 place, flip player, remember action
        Plane t = me; me = opp; opp = t;
        last = a;
        if (wins_through_wave(opp, a, N, d.k, d.rule, lane)) { out_kind = LEAF_TERM_LOSS; break; }  // the side to move has lost
        if (pl_count(me) + pl_count(opp) == G::nn) { out_kind = LEAF_TERM_DRAW; break; }
        if constexpr (SOLVER) {
            // a proven edge ends the simulation like a terminal: no evaluation, no row; the value of the side to move below it
            if (ast != PROOF_UNKNOWN) {
                out_kind = ast == PROOF_WIN ? LEAF_TERM_LOSS : (ast == PROOF_LOSS ? LEAF_TERM_WIN : LEAF_TERM_DRAW);
                if (lane == 0) d.proof_stops[b] += 1ull;
                break;
            }
        }
        if (child == 0) { out_kind = LEAF_EXPAND; break; }    // mcts.py:127 node.is_leaf()
        npar = an;
        row = child;
    }
    if (!SYNTH && d.cache && out_kind == LEAF_EXPAND) {
        // the leaf's evaluation may be known already (an earlier ply's search, another game, a transposition)
        float cx[G::CPL], ch;
        const int sym = d.leaf_sym ? leaf_sym_of(game_key(d, game), ply, rootN + 1) : 0;     // as stored below
        const bool hit = cache_lookup<N>(d, me, opp, last, cache_net_key(netid, sym), lane, cx, ch);
        if (hit) {
            cache_hit_store<N>(d.logits + (size_t)b * G::RW, cx, lane, d.leaf_sym != nullptr, sym);
            d.vhid[(size_t)b * 64 + lane] = ch;
            out_kind = LEAF_EXPAND_HIT;
        }
        if (lane == 0) {
            d.cnt[(size_t)b * CNT_STRIDE + 6] += 1ull;
            d.cnt[(size_t)b * CNT_STRIDE + 7] += hit ? 1ull : 0ull;
        }
    }
    if (lane == 0) {
        pl_store(d.leaf + (size_t)b * 8, me);
        pl_store(d.leaf + (size_t)b * 8 + 4, opp);
        d.leaf_last[b] = last;
        d.leaf_kind[b] = out_kind;
        d.depth[b] = depth;
        if (d.leaf_sym) d.leaf_sym[b] = leaf_sym_of(game_key(d, game), ply, rootN + 1);     // this leaf is evaluation rootN + 1 of the search
    }
}

// Evaluation cache for ROOT evaluations: runs after k_begin, one wave per slot.
template <int N>
__global__ __launch_bounds__(256) void k_root_cache(DevState d)
{
    typedef TreeGeo<N> G;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= d.B || d.s_status[b] != SLOT_ACTIVE) return;
    const size_t it = (size_t)b * d.L;                 // the root is item 0 of its game
    if (d.leaf_kind[it] != LEAF_ROOT) return;
    const Plane me = pl_load(d.leaf + it * 8), opp = pl_load(d.leaf + it * 8 + 4);
    float cx[G::CPL], ch;
    const int sym = d.leaf_sym ? d.leaf_sym[it] : 0;
    const bool hit = cache_lookup<N>(d, me, opp, d.leaf_last[it], cache_net_key(d.s_net[b], sym), lane, cx, ch);
    if (hit) {
        cache_hit_store<N>(d.logits + it * G::RW, cx, lane, d.leaf_sym != nullptr, sym);
        d.vhid[it * 64 + lane] = ch;
    }
    if (lane == 0) {
        if (hit) d.leaf_kind[it] = LEAF_ROOT_HIT;
        d.cnt[(size_t)b * CNT_STRIDE + 6] += 1ull;
        d.cnt[(size_t)b * CNT_STRIDE + 7] += hit ? 1ull : 0ull;
    }
}

// ------------------------------------------------------------------------------------------------
// k_step_vl: the tree step with virtual-loss batching (opt-in; the reference's loop mcts.py:123-141 is strictly
// sequential and only lists "virtual loss" as a TODO, mcts.py:17-22).  A game owns L evaluation items; every launch
//   stage 1: finishes the simulations of the pending batch in selection order -- takes the in-flight visit back from the
//            path, expands the leaf with its evaluation and backs the value up exactly like mcts.py:136-141; a
//            "duplicate" (its leaf was already pending for an earlier item of the batch) backs up that item's value;
//   stage 2: selects the next batch: item j descends with every edge on the paths of items 0..j-1 counting one extra
//            visit that lost (N + 1, W - 1), and leaves its own in-flight mark on the edges it takes.
// The in-flight count lives in the 5 spare bits of the edge's 16-bit visit field; W is never touched by it, so taking
// a virtual visit back is exact.  Same arithmetic and operator order as the oracle's restatement (orc_cfg.vl); with
// L = 1 it reproduces k_step.  Dynamic LDS: (S + 2) doubles.
// DEEP (S > DEFAULT_MAX_S, visit counts beyond EDGE_N_MASK): the edge's N is a plain 16-bit count and the in-flight count
// lives in a byte array beside the tree (the DEEP kernel's extra argument, [B][R][RW], when L > 1), read with the edge, raised where the
// narrow kernel adds 1 << EDGE_N_BITS, lowered at backup, zeroed with every new row; the sqrt table is read from HBM as in
// k_step<.., DEEP>.  Mechanically the same rule: bit-identical to the oracle at any S.
// ------------------------------------------------------------------------------------------------
// CAND: the caller's CandLevel (and whatever follows it) comes last; its exp plane is formed here, as in k_step
template <int N, bool SYNTH, bool CAND = false, class... Cand>
__device__ __forceinline__ void vl_leaf_eval(const DevState &d, size_t it, const Plane &lme, const Plane &lopp, int leaf_last,
                                             int netid, bool fresh, int lane, float (&P)[TreeGeo<N>::CPL], float &v, Cand &... cand)
{
    typedef TreeGeo<N> G;
    if constexpr (CAND) {
        Plane occx;
#pragma unroll
        for (int q = 0; q < 4; q++) occx.w[q] = lme.w[q] | lopp.w[q];
        cand_level(cand...).exp = cand_plane<N>(occx, d.cand_radius);
    }
    if (SYNTH) {
        unsigned hx = 0;
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            int j = lane + 64 * i;
            if (j < G::nn) {
                unsigned code = pl_get(lme, j) ? 1u : (pl_get(lopp, j) ? 2u : 0u);
                hx ^= az_fmix32((unsigned)j * 3u + code + 0x9E3779B9u);
            }
        }
        unsigned hs = wave_xor_u(hx);
        hs ^= az_fmix32(0x51ED270Bu + (unsigned)(leaf_last + 1));
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            int j = lane + 64 * i;
            unsigned r = az_fmix32(hs + (unsigned)(j + 1) * 0x9E3779B1u);
            P[i] = (float)(((r >> 8) & 0xFFFFu) + 1u) * 0x1p-23f;
        }
        int vv = (int)(az_fmix32(hs ^ 0x7F4A7C15u) & 0x1FFu);
        v = (float)(vv - 256) / 256.0f;
        if constexpr (CAND) {
#pragma unroll
            for (int i = 0; i < G::CPL; i++) P[i] = cand_exp(lane + 64 * i, cand...) ? P[i] : 0.0f;
        }
        return;
    }
    float x[G::CPL];
    const float *lg = d.logits + it * G::RW;
    if (d.leaf_sym) {
        // the net saw this leaf under symmetry t: board cell j sits at image cell sym_src(t^-1, j)
        const int ti = sym_inverse(d.leaf_sym[it]);
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            const int j = lane + 64 * i, r = j / N;
            x[i] = j < G::nn ? lg[sym_src(ti, r, j - r * N, N)] : 0.0f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < G::CPL; i++) x[i] = lane + 64 * i < G::nn ? lg[lane + 64 * i] : 0.0f;
    }
    const float h_l = d.vhid[it * 64 + lane];
    if (d.ext_eval) {
        // the evaluator lives outside the engine (az_set_external_evaluator): the row holds the priors it returned, as they
        // are, and the first hidden entry its value -- no softmax, no value head, no cache, no weights
#pragma unroll
        for (int i = 0; i < G::CPL; i++) P[i] = x[i];
        v = __shfl(h_l, 0, 64);
        return;
    }
    const float w2_l = d.v2w[netid][lane];
    const float b2 = d.v2b[netid][0];
    if (d.cache && fresh) cache_insert<N>(d, lme, lopp, leaf_last, cache_net_key(netid, d.leaf_sym ? d.leaf_sym[it] : 0), lane, x, h_l);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        if (CAND ? !cand_exp(lane + 64 * i, cand...) : lane + 64 * i >= G::nn) x[i] = -INFINITY;
        mx = fmaxf(mx, x[i]);
    }
    mx = wave_max_f(mx);
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        P[i] = 0.0f;
        if (CAND ? cand_exp(lane + 64 * i, cand...) : lane + 64 * i < G::nn) {
            P[i] = az_expf(x[i] - mx);
            part = part + P[i];
        }
    }
    const float ssum = wave_sum_butterfly(part);
#pragma unroll
    for (int i = 0; i < G::CPL; i++) P[i] = P[i] / ssum;
    const float acc = value_fc2_chain(h_l, w2_l);
    v = az_tanhf(acc + b2);
}

__device__ __forceinline__ unsigned char *inflight_arg() { return nullptr; }
__device__ __forceinline__ unsigned char *inflight_arg(unsigned char *p) { return p; }
__device__ __forceinline__ unsigned char *inflight_arg(SelLevel &) { return nullptr; }
__device__ __forceinline__ unsigned char *inflight_arg(SelLevel &, unsigned char *p) { return p; }
__device__ __forceinline__ unsigned char *inflight_arg(CandLevel &) { return nullptr; }
__device__ __forceinline__ unsigned char *inflight_arg(CandLevel &, unsigned char *p) { return p; }
// InFlight is empty for the default kernel (its arguments stay those of the narrow kernel) and `unsigned char *` for DEEP
// SEL (az_set_selection): k_step's rule on the counts and totals this kernel scores with, N + in-flight and W - in-flight; a
// SelLevel goes in front of the extra arguments
// CAND (az_set_candidates): as in k_step, never with SEL; a CandLevel goes in front of the extra arguments
template <int N, bool SYNTH, bool DEEP = false, bool SEL = false, bool CAND = false, class... InFlight>
__global__ __launch_bounds__(256) void k_step_vl(DevState d, int sims_done, int nb_next, InFlight... inflight)
{
    static_assert(!(CAND && SEL), "the CAND kernels do not carry the selection rule");
    typedef TreeGeo<N> G;
    extern __shared__ double sq_lds[];                 // np.sqrt(N + 1e-8), N = 0..S+1 (mcts.py:73)
    __shared__ float vals_lds[4][VL_MAX];              // leaf values of the batch being finished (duplicates read them)
    __shared__ unsigned pend_lds[4][VL_MAX];           // leaf edge (row << 16 | cell) of every item waiting for an evaluation
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wv;
    if constexpr (!DEEP)
        for (int i = threadIdx.x; i < d.S + 2; i += 256) sq_lds[i] = d.sqrt_table[i];
    __syncthreads();
    if (b >= d.B || d.s_status[b] != SLOT_ACTIVE) return;
    const int L = d.L;
    const size_t it0 = (size_t)b * L;
    Edge *rows = d.edges + (size_t)b * d.R * G::RW;
    // DEEP: in-flight counts of this slot's edges (L == 1 never has any: no array, nothing read or written)
    unsigned char *infl = DEEP && L > 1 ? inflight_arg(inflight...) + (size_t)b * d.R * G::RW : nullptr;
    const int pl = d.s_player[b], slast = d.s_last[b], netid = d.s_net[b], game = d.s_game[b], ply = d.s_ply[b];
    // playout cap: this slot's simulations, < 0 = a FAST ply (no root noise); it selects min(L, budget - done) leaves per batch
    const int budget_raw = d.cap_fast ? d.s_budget[b] : d.S;
    const bool root_noise = d.add_noise && budget_raw > 0;
    nb_next = min(nb_next, max((budget_raw < 0 ? -budget_raw : budget_raw) - sims_done, 0));
    const Plane bX = pl_load(d.board + (size_t)b * 8), bO = pl_load(d.board + (size_t)b * 8 + 4);
    float *vals = vals_lds[wv];
    unsigned *pend = pend_lds[wv];
    int rows_used = d.rows_used[b];
    unsigned long long c_exp = 0, c_sim = 0, c_term = 0, c_depth = 0, c_dup = 0, c_look = 0, c_hit = 0;

    // ---------------- stage 1: finish the pending batch in selection order ----------------
    for (int j = 0; j < L; j++) {
        const size_t it = it0 + j;
        const int kind_raw = d.leaf_kind[it];
        if (kind_raw == LEAF_NONE) continue;
        const int kind = kind_raw == LEAF_EXPAND_HIT ? LEAF_EXPAND : (kind_raw == LEAF_ROOT_HIT ? LEAF_ROOT : kind_raw);
        const int depth0 = d.depth[it];
        unsigned *path = d.path + it * G::PATH;
        float v = 0.0f;
        if (kind == LEAF_ROOT || kind == LEAF_EXPAND) {
            const Plane lme = pl_load(d.leaf + it * 8), lopp = pl_load(d.leaf + it * 8 + 4);
            const int leaf_last = d.leaf_last[it];
            float P[G::CPL];
            if constexpr (CAND) vl_leaf_eval<N, SYNTH, true>(d, it, lme, lopp, leaf_last, netid, kind_raw == kind, lane, P, v, inflight...);
            else vl_leaf_eval<N, SYNTH>(d, it, lme, lopp, leaf_last, netid, kind_raw == kind, lane, P, v);
            if constexpr (SEL) {
                if (kind == LEAF_ROOT && lane == 0) d.root_v[b] = v;      // az_set_selection: the root's value for the ply
            }
            if (kind == LEAF_ROOT && root_noise) {
                // mcts.py:113-116; float32 multiply, float64 add, float32 store
                Plane occ;
#pragma unroll
                for (int q = 0; q < 4; q++) occ.w[q] = lme.w[q] | lopp.w[q];
                const double *nz = d.noise + (size_t)game * d.noise_stride + d.noise_off[ply];
                if constexpr (CAND) {
                    cand_mix_noise<G::CPL>(d, occ, cand_level(inflight...).exp, nz, lane, P);
                } else {
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    int c = lane + 64 * i;
                    if (c < G::nn && !pl_get(occ, c)) {
                        int rank = c - pl_rank(occ, c);
                        float scaled = d.one_minus_w * P[i];
                        P[i] = (float)((double)scaled + d.w_noise * nz[rank]);
                    }
                }
                }
            }
            // mcts.py:50-64 expand: one edge per cell (occupied cells are never selected)
            const int row = kind == LEAF_ROOT ? 0 : rows_used;
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                Edge e;
                e.W = 0.0; e.P = P[i]; e.N = 0; e.child = 0;
                rows[(size_t)row * G::RW + lane + 64 * i] = e;
                if (DEEP && infl) infl[(size_t)row * G::RW + lane + 64 * i] = 0;
            }
            rows_used = row + 1;
            if (kind == LEAF_EXPAND) {
                const unsigned pe = path[depth0 - 1];
                if (lane == 0) rows[(size_t)(pe >> 16) * G::RW + (pe & 0xFFFFu)].child = (unsigned short)row;
            }
        }
        vals[j] = v;                                    // every lane holds the same v
        if (kind != LEAF_ROOT) {
            // mcts.py:132-134,141,76-82: value w.r.t. the side to move at the leaf, backed up with alternating sign
            double value;
            if (kind == LEAF_EXPAND) value = (double)v;
            else if (kind >= LEAF_DUP_BASE) value = (double)vals[kind - LEAF_DUP_BASE];
            else value = kind == LEAF_TERM_LOSS ? -1.0 : 0.0;
            for (int dd = lane; dd < depth0; dd += 64) {
                const unsigned pe = path[dd];
                Edge *e = rows + (size_t)(pe >> 16) * G::RW + (pe & 0xFFFFu);
                const double val = ((depth0 - 1 - dd) & 1) ? value : -value;
                if (DEEP) {
                    if (infl) { unsigned char *f = infl + (size_t)(pe >> 16) * G::RW + (pe & 0xFFFFu); *f = (unsigned char)(*f - 1); }
                    e->N = (unsigned short)(e->N + 1);                        // the in-flight visit becomes a real one
                } else {
                    e->N = (unsigned short)(e->N - (1 << EDGE_N_BITS) + 1);  // the in-flight visit becomes a real one
                }
                e->W = e->W + val;
            }
            c_exp += kind == LEAF_EXPAND ? 1ull : 0ull;
            c_dup += kind >= LEAF_DUP_BASE ? 1ull : 0ull;
            c_term += (kind == LEAF_TERM_LOSS || kind == LEAF_TERM_DRAW) ? 1ull : 0ull;
            c_sim += 1ull;
            c_depth += (unsigned long long)depth0;
        }
        wave_mem_sync();
    }

    // ---------------- stage 2: select the next batch (mcts.py:124-129 with in-flight visits counted as losses) ----------------
    const Plane rme = pl == 1 ? bX : bO, ropp = pl == 1 ? bO : bX;
    const bool forced = d.forced_k > 0.0 && root_noise;       // forced playouts (kernel-argument test, uniform): the noised root only
    for (int j = 0; j < L; j++) {
        const size_t it = it0 + j;
        if (j >= nb_next) {
            if (lane == 0) d.leaf_kind[it] = LEAF_NONE;
            continue;
        }
        Plane me = rme, opp = ropp;
        int row = 0, npar = sims_done + j, depth = 0, last = slast, out_kind = LEAF_NONE;
        unsigned *path = d.path + it * G::PATH;
        unsigned leaf_edge = 0xFFFFFFFFu;
        double sq_next = DEEP ? d.sqrt_table[npar] : 0.0;
        if constexpr (SEL) {                                  // as in k_step
            SelLevel &sl = sel_level(inflight...);
            sl.cp = d.sel_cpuct[npar];
            sl.vx = (double)d.root_v[b];                          // after stage 1's wave_mem_sync: this launch may have written it
        }
        for (;;) {
            Plane occ;
#pragma unroll
            for (int q = 0; q < 4; q++) occ.w[q] = me.w[q] | opp.w[q];
            const double sq = DEEP ? sq_next : sq_lds[npar];      // np.sqrt(self.N + 1e-8), mcts.py:73
            if constexpr (CAND) cand_level(inflight...).lvl = cand_plane<N>(occ, d.cand_radius);     // C(X) of this level's node
            double best = 0.0;
            int bi = -1, bN = 0, bC = 0;
            if constexpr (SEL) {
                SelLevel &sl = sel_level(inflight...);
                Edge er[G::CPL];
                int nvs[G::CPL];
                unsigned ms = 0u;
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    const int c = lane + 64 * i;
                    nvs[i] = 0;
                    if (c < G::nn && !pl_get(occ, c)) {
                        er[i] = rows[(size_t)row * G::RW + c];
                        const int fl = DEEP ? (infl ? (int)infl[(size_t)row * G::RW + c] : 0) : (int)er[i].N >> EDGE_N_BITS;
                        nvs[i] = (DEEP ? (int)er[i].N : ((int)er[i].N & EDGE_N_MASK)) + fl;
                        ms += nvs[i] ? sel_mass_of(er[i].P) : 0u;
                    }
                }
                ms = (unsigned)wave_sum_i((int)ms);
                const double unv = sel_unvisited(sl.vx, row == 0 ? d.sel_fpu_root : d.sel_fpu, d.sel_mass[sel_mass_index(ms)]);
                sl.bQ = 0.0;
#pragma unroll
                for (int i = 0; i < G::CPL; i++) {
                    const int c = lane + 64 * i;
                    if (c < G::nn && !pl_get(occ, c)) {
                        const Edge e = er[i];
                        const int nv = nvs[i];
                        const int fl = nv - (DEEP ? (int)e.N : ((int)e.N & EDGE_N_MASK));
                        const double wvv = e.W - (double)fl;
                        const double Q = nv ? wvv / (double)nv : unv;
                        double sc = Q + ((sl.cp * (double)e.P) * sq) / (double)(1 + nv);
                        if (forced && row == 0 && forced_child((double)nv, d.forced_k, e.P, sims_done + j)) sc = INFINITY;
                        if (bi < 0 || sc > best) { best = sc; bi = c; bN = nv; bC = e.child; sl.bQ = Q; }
                    }
                }
            } else {
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                int c = lane + 64 * i;
                if (CAND ? cand_lvl(c, inflight...) : (c < G::nn && !pl_get(occ, c))) {
                    Edge e = rows[(size_t)row * G::RW + c];
                    // simulations of this batch in flight through the edge
                    const int fl = DEEP ? (infl ? (int)infl[(size_t)row * G::RW + c] : 0) : (int)e.N >> EDGE_N_BITS;
                    const int nv = (DEEP ? (int)e.N : ((int)e.N & EDGE_N_MASK)) + fl;
                    const double wvv = e.W - (double)fl;
                    double Q = nv ? wvv / (double)nv : 0.0;
                    double sc = Q + ((d.c_puct * (double)e.P) * sq) / (double)(1 + nv);
                    if (forced && row == 0 && forced_child((double)nv, d.forced_k, e.P, sims_done + j)) sc = INFINITY;
                    if (bi < 0 || sc > best) { best = sc; bi = c; bN = nv; bC = e.child; }
                }
            }
            }
            wave_argmax(best, bi);
            const int a = __builtin_amdgcn_readfirstlane(bi);
            if (a < 0) { out_kind = LEAF_NONE; break; }
            const int child = __builtin_amdgcn_readlane(bC, a & 63);
            const int an = __builtin_amdgcn_readlane(bN, a & 63);
            if (DEEP) sq_next = d.sqrt_table[an];                 // the next level's parent visits: issued before the win test
            if constexpr (SEL) {
                SelLevel &sl = sel_level(inflight...);
                sl.cp = d.sel_cpuct[an];
                sl.vx = -lane_d(sl.bQ, a & 63);
            }
            if (lane == (a & 63)) {
                if (DEEP) {
                    if (infl) { unsigned char *f = infl + (size_t)row * G::RW + a; *f = (unsigned char)(*f + 1); }
                } else {
                    Edge *e = rows + (size_t)row * G::RW + a;
                    e->N = (unsigned short)(e->N + (1 << EDGE_N_BITS));
                }
            }
            if (lane == 0) path[depth] = ((unsigned)row << 16) | (unsigned)a;
            leaf_edge = ((unsigned)row << 16) | (unsigned)a;
            depth++;
            pl_set(me, a);                                        // games.py:79-81 place, flip player, remember action
            Plane t = me; me = opp; opp = t;
            last = a;
            if (wins_through_wave(opp, a, N, d.k, d.rule, lane)) { out_kind = LEAF_TERM_LOSS; break; }
            if (pl_count(me) + pl_count(opp) == G::nn) { out_kind = LEAF_TERM_DRAW; break; }
            if (child == 0) { out_kind = LEAF_EXPAND; break; }    // mcts.py:127 node.is_leaf()
            npar = an;
            row = child;
        }
        unsigned mark = 0xFFFFFFFFu;
        if (out_kind == LEAF_EXPAND) {
            int dup = -1;
            for (int i = 0; i < j; i++)
                if (dup < 0 && pend[i] == leaf_edge) dup = i;
            if (dup >= 0) {
                out_kind = LEAF_DUP_BASE + dup;
            } else {
                mark = leaf_edge;
                if (!SYNTH && d.cache) {
                    float cx[G::CPL], ch;
                    const int sym = d.leaf_sym ? leaf_sym_of(game_key(d, game), ply, sims_done + j + 1) : 0;
                    const bool hit = cache_lookup<N>(d, me, opp, last, cache_net_key(netid, sym), lane, cx, ch);
                    if (hit) {
                        cache_hit_store<N>(d.logits + it * G::RW, cx, lane, d.leaf_sym != nullptr, sym);
                        d.vhid[it * 64 + lane] = ch;
                        out_kind = LEAF_EXPAND_HIT;
                    }
                    c_look += 1ull;
                    c_hit += hit ? 1ull : 0ull;
                }
            }
        }
        pend[j] = mark;
        if (lane == 0) {
            pl_store(d.leaf + it * 8, me);
            pl_store(d.leaf + it * 8 + 4, opp);
            d.leaf_last[it] = last;
            d.leaf_kind[it] = out_kind;
            d.depth[it] = depth;
            // simulation sims_done + j of the search: its leaf is evaluation sims_done + j + 1 (0 = the root), as in k_step
            if (d.leaf_sym) d.leaf_sym[it] = leaf_sym_of(game_key(d, game), ply, sims_done + j + 1);
        }
        wave_mem_sync();
    }
    if (lane == 0) {
        d.rows_used[b] = rows_used;
        unsigned long long *c = d.cnt + (size_t)b * CNT_STRIDE;
        c[0] += c_exp; c[1] += c_sim; c[2] += c_term; c[3] += c_depth; c[5] += c_dup; c[6] += c_look; c[7] += c_hit;
    }
}

// numpy pairwise sum of a contiguous float64 block (n <= 128): np.add.reduce on a contiguous array accumulates in 8 lanes
// over blocks of <= 128 and combines them pairwise; probs.sum() at mcts.py:163 goes through it
__host__ __device__ inline double pw_block(const double *a, int n)
{
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; i++) r += a[i];
        return r;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; i++) res += a[i];
    return res;
}
// np.add.reduce of A <= 225 contiguous float64: one block up to 128 entries, else two halves (the first a multiple of 8)
__host__ __device__ inline double pw_sum(const double *a, int A)
{
    int n2 = A / 2;
    n2 -= n2 % 8;
    return A <= 128 ? 0.0 + pw_block(a, A) : 0.0 + (pw_block(a, n2) + pw_block(a + n2, A - n2));
}

// az_set_solver: N' of a root row, shared by k_move and the host's az_solver_counts.  any_win: some legal edge is WIN;
// survivor: some legal edge that is not LOSS has a visit.  A child keeps its count unless the rule empties it.
__host__ __device__ __forceinline__ bool solver_keeps(int st, bool any_win, bool survivor)
{
    return any_win ? st == PROOF_WIN : !(survivor && st == PROOF_LOSS);
}
template <int CPL>
__device__ __forceinline__ void solver_counts_wave(const int (&Nj)[CPL], const int (&st)[CPL], const bool (&legal)[CPL], int (&Np)[CPL])
{
    bool w = false, sv = false;
#pragma unroll
    for (int i = 0; i < CPL; i++) {
        w = w || (legal[i] && st[i] == PROOF_WIN);
        sv = sv || (legal[i] && st[i] != PROOF_LOSS && Nj[i] > 0);
    }
    const bool any_win = __ballot(w) != 0ull, survivor = __ballot(sv) != 0ull;
#pragma unroll
    for (int i = 0; i < CPL; i++) Np[i] = solver_keeps(st[i], any_win, survivor) ? Nj[i] : 0;
}

// ------------------------------------------------------------------------------------------------
// k_move: visit counts -> pi -> sampled action (mcts.py:144-177), record (self_play.py:63),
//         apply (games.py:64-82), terminal check (games.py:133-166).
// ------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void k_move(DevState d)
{
    typedef TreeGeo<N> G;
    __shared__ double ebuf_all[4][G::RW];
    __shared__ unsigned short idx_all[4][REUSE_MAX_ROWS];   // subtree reuse: new row index of every kept row
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wv;
    if (b >= d.B) return;
    if (d.s_status[b] != SLOT_ACTIVE) return;
    double *ebuf = ebuf_all[wv];
    const int g = d.s_game[b], ply = d.s_ply[b], pl = d.s_player[b];
    Plane X = pl_load(d.board + (size_t)b * 8), O = pl_load(d.board + (size_t)b * 8 + 4);
    Plane occ;
#pragma unroll
    for (int q = 0; q < 4; q++) occ.w[q] = X.w[q] | O.w[q];
    const int A = G::nn - pl_count(occ);
    const Edge *root = d.edges + (size_t)b * d.R * G::RW;
    const double T = d.T_game ? d.T_game[g] : d.T_table[d.arena ? ((ply + 1) >> 1) : ply];   // evaluator.py:71-90 step quirk
    const double u = d.u[(size_t)g * G::nn + ply];

    int Nj[G::CPL], rank[G::CPL];
    bool legal[G::CPL];
    double e[G::CPL];
    const int nmask = d.S > DEFAULT_MAX_S ? 0xFFFF : EDGE_N_MASK;     // deep searches: N is the whole 16-bit visit count
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        int j = lane + 64 * i;
        legal[i] = j < G::nn && !pl_get(occ, j);
        Nj[i] = legal[i] ? (int)root[j].N & nmask : 0;
        rank[i] = legal[i] ? j - pl_rank(occ, j) : 0;
    }
    // a* = the most visited legal cell, the lowest cell on ties: one order-independent reduction of (N << 16 | 0xFFFF - cell); N fits
    // 16 bits, a cell 8.  Every ply ends with at least one visit under the root, so N[a*] >= 1.
    unsigned best = 0u;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        const unsigned key = ((unsigned)Nj[i] << 16) | (unsigned)(0xFFFF - (lane + 64 * i));
        if (legal[i] && key > best) best = key;
    }
    best = wave_max_u(best);
    const int astar = best ? 0xFFFF - (int)(best & 0xFFFFu) : 0;      // an active slot always has a legal cell
    // ---- policy target pruning (az_set_forced_playouts, noised roots only): pi and the move are made from Np, which takes the
    // forced visits back from every child but a* as far as its PUCT score stays below a*'s; everything else keeps the raw Nj ----
    int Np[G::CPL];
#pragma unroll
    for (int i = 0; i < G::CPL; i++) Np[i] = Nj[i];
    if (d.forced_k > 0.0 && d.forced_prune && d.add_noise && (d.cap_fast ? d.s_budget[b] : 1) > 0) {
        int tot = 0;
#pragma unroll
        for (int i = 0; i < G::CPL; i++) tot += Nj[i];
        tot = wave_sum_i(tot);
        const double sq = d.sqrt_table[tot];
        const Edge es = root[astar];
        const double cp = d.sel_cpuct ? d.sel_cpuct[tot] : d.c_puct;     // az_set_selection: c(count), the count the sqrt takes
        const double target = forced_score(es.W / (double)(int)(best >> 16), cp, es.P, sq, (int)(best >> 16));
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            const int j = lane + 64 * i;
            if (legal[i] && Nj[i] > 0 && j != astar) {
                const Edge ec = root[j];
                Np[i] = forced_pruned(d.forced_k, cp, ec.W / (double)Nj[i], ec.P, Nj[i], tot, sq, target);
            }
        }
    }
    // ---- MCTS-Solver (az_set_solver, every root): pi and the move are made from Np = the counts of the WIN edges when there is
    // one, else the counts without the LOSS edges when a visited edge survives that, else the raw counts (solver_counts) ----
    int rproof = PROOF_UNKNOWN;
    if (d.proof) {
        const unsigned char *prow = d.proof + (size_t)b * d.R * G::RW;
        int st[G::CPL];
#pragma unroll
        for (int i = 0; i < G::CPL; i++) st[i] = legal[i] ? (int)prow[lane + 64 * i] : PROOF_UNKNOWN;
        solver_counts_wave<G::CPL>(Nj, st, legal, Np);
        rproof = d.root_proof[b];
    }
    // ---- Gumbel root search (az_set_gumbel, noised roots only): the move is the best g + logit + sigma(q) among the most visited
    // children, and pi the softmax of logit + sigma(completed q); the softmax itself is the temperature path's below ----
    const bool gumbel = d.gumbel_m > 0 && d.add_noise && (d.cap_fast ? d.s_budget[b] : 1) > 0;
    int ga = -1;
    if (gumbel) {
        const double *nz = d.noise + (size_t)g * d.noise_stride + d.noise_off[ply];
        const float *rl = d.root_logits + (size_t)b * G::RW;
        const int maxN = (int)(best >> 16);
        const double sig = gumbel_sigma(d.gumbel_cv, d.gumbel_cs, maxN);
        double q[G::CPL], Pd[G::CPL], lg[G::CPL];
        double sc = 0.0;
        int bi = -1, tot = 0;
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            const int j = lane + 64 * i;
            q[i] = 0.0; Pd[i] = 0.0; lg[i] = 0.0;
            if (legal[i]) {
                const Edge ec = root[j];
                lg[i] = (double)rl[j];
                Pd[i] = Nj[i] ? (double)ec.P : 0.0;
                q[i] = Nj[i] ? ec.W / (double)Nj[i] : 0.0;
                tot += Nj[i];
                if (Nj[i] == maxN) {
                    const double sj = gumbel_score(nz[rank[i]] + lg[i], sig, q[i]);
                    if (bi < 0 || sj > sc) { sc = sj; bi = j; }
                }
            }
        }
        wave_argmax(sc, bi);
        ga = __builtin_amdgcn_readfirstlane(bi);
        tot = wave_sum_i(tot);
        // pv = sum of the visited children's priors, pq = sum of prior * q, both in np.add.reduce order over the legal cells
        double pv = 0.0, pq = 0.0;
#pragma unroll
        for (int i = 0; i < G::CPL; i++)
            if (legal[i]) ebuf[rank[i]] = Pd[i];
        wave_mem_sync();
        if (lane == 0) pv = pw_sum(ebuf, A);
        wave_mem_sync();
#pragma unroll
        for (int i = 0; i < G::CPL; i++)
            if (legal[i]) ebuf[rank[i]] = Pd[i] * q[i];
        wave_mem_sync();
        if (lane == 0) pq = pw_sum(ebuf, A);
        wave_mem_sync();
        pv = __shfl(pv, 0, 64);
        pq = __shfl(pq, 0, 64);
        const double vmix = gumbel_vmix(d.root_v[b], (double)tot, pv, pq);
#pragma unroll
        for (int i = 0; i < G::CPL; i++) e[i] = legal[i] ? gumbel_score(lg[i], sig, Nj[i] ? q[i] : vmix) : -INFINITY;
    }
    bool uniform = false;
    double s = 1.0;
    if (!gumbel && T <= 1e-7) {
        // temperature clipped to the Python float 1e-7 -> float32 arithmetic, exp() is exactly 0 or 1
        float y[G::CPL], m = -INFINITY;
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            y[i] = legal[i] ? d.log_table[Np[i]] / 1e-7f : -INFINITY;
            m = fmaxf(m, y[i]);
        }
        m = wave_max_f(m);
        int ties = 0;
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            y[i] = legal[i] ? ((y[i] - m) == 0.0f ? 1.0f : az_expf(y[i] - m)) : 0.0f;
            ties += y[i] == 1.0f ? 1 : 0;
        }
        ties = wave_sum_i(ties);
#pragma unroll
        for (int i = 0; i < G::CPL; i++) e[i] = (double)(y[i] / (float)ties);
    } else {
        double m = -INFINITY;
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            if (!gumbel) e[i] = legal[i] ? (double)d.log_table[Np[i]] / T : -INFINITY;
            m = e[i] > m ? e[i] : m;
        }
        m = wave_max_d(m);
#pragma unroll
        for (int i = 0; i < G::CPL; i++) {
            e[i] = legal[i] ? az_exp(e[i] - m) : 0.0;
            if (legal[i]) ebuf[rank[i]] = e[i];
        }
        wave_mem_sync();
        if (lane == 0) {
            int n2 = A / 2;
            n2 -= n2 % 8;
            s = A <= 128 ? 0.0 + pw_block(ebuf, A) : 0.0 + (pw_block(ebuf, n2) + pw_block(ebuf + n2, A - n2));
        }
        s = __shfl(s, 0, 64);
        uniform = (s < 1e-8) || (s != s);
#pragma unroll
        for (int i = 0; i < G::CPL; i++) e[i] = uniform ? 1.0 / (double)A : e[i] / s;
        wave_mem_sync();
    }
    // RandomState.choice: cdf = p.cumsum(); cdf /= cdf[-1]; searchsorted(u, side='right')
#pragma unroll
    for (int i = 0; i < G::CPL; i++)
        if (legal[i]) ebuf[rank[i]] = e[i];
    wave_mem_sync();
    double lastc = 0.0;
    if (lane == 0) {
        double run = ebuf[0];
        for (int i = 1; i < A; i++) { run = run + ebuf[i]; ebuf[i] = run; }
        lastc = run;
    }
    lastc = __shfl(lastc, 0, 64);
    wave_mem_sync();
    int cntle = 0;
    for (int i = lane; i < A; i += 64) cntle += (ebuf[i] / lastc <= u) ? 1 : 0;
    int idx = wave_sum_i(cntle);
    if (idx >= A) idx = A - 1;
    int mycell = -1;
#pragma unroll
    for (int i = 0; i < G::CPL; i++)
        if (legal[i] && rank[i] == idx) mycell = lane + 64 * i;
    u64 bal = __ballot(mycell >= 0);
    int src = __ffsll((long long)bal) - 1;
    const int a = gumbel ? ga : __shfl(mycell, src, 64);      // a Gumbel ply uses neither the temperature nor u

    // ---- record (self_play.py:63): state before the move, pi, mover ----
    const size_t ri = (size_t)g * G::nn + ply;
#pragma unroll
    for (int i = 0; i < G::CPL; i++) {
        int j = lane + 64 * i;
        if (j < G::nn) {
            d.rec_pi[ri * G::nn + j] = legal[i] ? (float)e[i] : 0.0f;
            d.rec_visits[ri * G::nn + j] = (unsigned short)Nj[i];
        }
    }
    // ---- search value of the ply: v = W[a*] / N[a*] of the raw counts (a* found above) ----
    // (az_set_solver: exactly +1, -1 or 0 when the root is proven)
    const double v = rproof == PROOF_UNKNOWN ? root[astar].W / (double)(int)(best >> 16)
                                             : (rproof == PROOF_WIN ? 1.0 : (rproof == PROOF_LOSS ? -1.0 : 0.0));
    // resignation (az_set_resign): the ply crosses below -threshold; an exempt game only notes it and plays on
    const bool crossed = d.resign_thr > 0.0 && ply >= d.resign_min_ply && v < -d.resign_thr;
    const bool exempt = !d.arena && az_fmix32((unsigned)game_key(d, g)) % 1000u < (unsigned)d.resign_permille;
    // ---- apply + terminal ----
    Plane mine = pl == 1 ? X : O;
    pl_set(mine, a);
    Plane occ2 = occ;
    pl_set(occ2, a);
    bool win = wins_through(mine, a, N, d.k, d.rule);
    bool full = pl_count(occ2) == G::nn;
    const bool resign = crossed && !exempt && !(win || full);     // a natural end by this very move takes precedence
    if (lane == 0) {
        u64 *rp = d.rec_planes + ri * 8;
        for (int q = 0; q < 4; q++) {
            rp[q] = pl == 1 ? X.w[q] : O.w[q];
            rp[4 + q] = pl == 1 ? O.w[q] : X.w[q];
        }
        d.rec_last[ri] = (short)d.s_last[b];
        d.rec_mover[ri] = (unsigned char)pl;
        d.rec_action[ri] = (short)a;
        pl_store(d.board + (size_t)b * 8 + (pl == 1 ? 0 : 4), mine);
        d.s_player[b] = 3 - pl;
        d.s_last[b] = a;
        d.s_ply[b] = ply + 1;
        d.rec_value[ri] = (float)v;
        if (d.proof) d.rec_proof[ri] = (signed char)rproof;
        if (d.threat_edges) d.rec_threat[ri] = d.threat_depth[b];
        if (crossed && d.g_cross[g] < 0) d.g_cross[g] = ply;
        int res = win ? pl : (full ? 3 : 0);
        if (resign) res = 3 - pl;           // the mover resigns: on a crossing ply this is the result, max_plies or not
        bool cut = d.max_plies > 0 && ply + 1 >= d.max_plies;
        if (res != 0 || cut) {
            d.g_result[g] = res;
            d.g_nply[g] = ply + 1;
            d.s_status[b] = SLOT_FINISHED;
        }
        d.leaf_kind[(size_t)b * d.L] = LEAF_NONE;
    }
    if (!d.reuse) return;
    // ---- subtree reuse: the chosen child's subtree becomes the next ply's tree ----
    // Rows are created in visiting order, so a child row always has a larger index than its parent: one ascending
    // pass marks the rows reachable from the child, a second one moves them down in place (destination <= source)
    // and renumbers the child links (R <= REUSE_MAX_ROWS, checked by az_set_subtree_reuse).
    {
        const bool cont = !(win || full) && !resign && !(d.max_plies > 0 && ply + 1 >= d.max_plies) && !d.arena;
        Edge *rows = d.edges + (size_t)b * d.R * G::RW;
        const int c = cont ? (int)rows[a].child : 0;
        if (c == 0) {
            if (lane == 0) d.carried[b] = -1;
            return;
        }
        unsigned short *idx = idx_all[wv];
        const unsigned short NOT = 0xFFFFu, KEEP = 0xFFFEu;
        const int used = d.rows_used[b];
        wave_mem_sync();
        for (int r = lane; r < used; r += 64) idx[r] = r == c ? KEEP : NOT;
        wave_mem_sync();
        for (int r = c; r < used; r++) {
            if (idx[r] != KEEP) continue;                     // uniform: every lane reads the same LDS word
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                const unsigned short ch = rows[(size_t)r * G::RW + lane + 64 * i].child;
                if (ch) idx[ch] = KEEP;
            }
            wave_mem_sync();
        }
        int kept = 0;
        if (lane == 0) {
            for (int r = c; r < used; r++)
                if (idx[r] == KEEP) idx[r] = (unsigned short)kept++;
        }
        wave_mem_sync();
        kept = __shfl(kept, 0, 64);
        int csum = 0;
        for (int r = c; r < used; r++) {
            const unsigned short dst = idx[r];
            if (dst == NOT) continue;
            Edge e[G::CPL];
#pragma unroll
            for (int i = 0; i < G::CPL; i++) {
                e[i] = rows[(size_t)r * G::RW + lane + 64 * i];
                if (e[i].child) e[i].child = idx[e[i].child];
                if (dst == 0) csum += (int)e[i].N;
            }
#pragma unroll
            for (int i = 0; i < G::CPL; i++) rows[(size_t)dst * G::RW + lane + 64 * i] = e[i];
        }
        csum = wave_sum_i(csum);
        if (lane == 0) {
            d.rows_used[b] = kept;
            d.carried[b] = csum;
        }
    }
}

#ifdef AZ_ENGINE_TU
// ------------------------------------------------------------------------------------------------
// k_refill: finished/idle slots receive the next game ids in slot order (ballot + prefix sum), replacing the task
//           queue of self_play.py:114-118,41-45.  The queue is ONE device counter shared by the lanes (streams) of an
//           engine: a chunk of slots claims its ids with a single atomicAdd, so a slot freed in any lane takes the next
//           waiting game.  claim_cap bounds the ids this launch may take (the first refill of an episode spreads the
//           games evenly over the lanes).  One block of 1024 threads.
//           compact != 0: afterwards the active slots are moved to the front of the lane, in order (a slot between plies is
//           its board, game id, ply, side to move and last move; the tree is rebuilt every ply), so that the next ply's
//           kernels can be launched over the active slots only.  A workgroup of a slot without a game would exit at once, but
//           it still needs its LDS allocation to be dispatched and so queues behind the other lanes' working workgroups: in
//           the tail of an episode that head-of-line blocking cost 30 % of a ply.  Invisible in the results (records go by
//           game id).  Not with subtree reuse (the tree outlives the ply).  With the playout cap on (d.cap_fast) the order is
//           active FULL, active FAST, idle, and d.active[1] = the number of FULL ones (written without compaction as well).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_refill(DevState d, int claim_cap, int compact)
{
    __shared__ int wsum[16], wsum2[16];
    __shared__ int base_s, take_s, cap_s, active_s, cbase_s, fbase_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { cap_s = claim_cap; active_s = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < d.B; c0 += 1024) {
        int b = c0 + tid;
        bool need = b < d.B && d.s_status[b] != SLOT_ACTIVE;
        bool act = b < d.B && d.s_status[b] == SLOT_ACTIVE;
        u64 bal = __ballot(need);
        int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(bal);
        u64 bact = __ballot(act);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < 16; w++) { off += w < wv ? wsum[w] : 0; tot += wsum[w]; }
        if (tid == 0) {
            int want = min(tot, cap_s), base = 0, got = 0;
            if (want > 0 && *(volatile int *)d.next_game < d.total_games) {     // an exhausted queue is left alone (no overflow)
                base = atomicAdd(d.next_game, want);
                got = max(0, min(want, d.total_games - base));
            }
            base_s = base; take_s = got; cap_s -= want;
        }
        __syncthreads();
        int newact = 0;
        if (need) {
            const int idx = off + pre;
            if (idx < take_s) {
                u64 *bd = d.board + (size_t)b * 8;
                const int gid = base_s + idx;
                const int odd = (d.arena && (gid & 1)) ? 1 : 0;   // evaluator.py:64-69: the other side moves first
                d.s_game[b] = gid;
                if (d.start_pos) {
                    // the game continues a given position; odd arena games see it with the colours exchanged (the plane
                    // halves swapped, the other side to move), which for the empty board is the rule above
                    const unsigned f = (unsigned)d.start_first + (unsigned)gid;
                    const StartPos &sp = d.start_pos[(d.arena ? f >> 1 : f) % (unsigned)d.start_count];
                    for (int q = 0; q < 8; q++) bd[q] = sp.w[odd ? q ^ 4 : q];
                    d.s_ply[b] = sp.ply;
                    d.s_player[b] = odd ? 3 - sp.player : sp.player;
                    d.s_last[b] = sp.last;
                } else {
                    for (int q = 0; q < 8; q++) bd[q] = 0ull;
                    d.s_ply[b] = 0;
                    d.s_player[b] = odd ? 2 : 1;
                    d.s_last[b] = -1;
                }
                d.s_status[b] = SLOT_ACTIVE;
                d.leaf_kind[(size_t)b * d.L] = LEAF_NONE;
                d.carried[b] = -1;
                newact = 1;
            } else {
                d.s_status[b] = SLOT_IDLE;
                d.s_game[b] = -1;
            }
        }
        u64 bnew = __ballot(newact != 0);
        if (lane == 0) atomicAdd(&active_s, __popcll(bnew) + __popcll(bact));
        __syncthreads();
    }
    if (tid == 0) *d.active = active_s;
    if (d.cap_fast) {
        // Playout cap: the number of active slots whose coming ply is FULL goes next to *d.active, and the compaction is a
        // stable three-way partition -- active FULL, active FAST, idle -- so that the second phase of the ply (the batches
        // only a FULL search has) is launched over the first d.active[1] slots.  A FAST slot can move UP, onto a slot not
        // yet read, so the partition goes through the staging arrays: FULL slots are placed there from the front and FAST
        // slots from the back (entry d.B - 1 - j holds the j-th FAST slot; the two ends cannot meet, there are at most d.B
        // active slots), which needs no count beforehand, and everything is copied back afterwards.  Without compaction
        // only the count is made.
        if (tid == 0) { cbase_s = 0; fbase_s = 0; }
        __syncthreads();
        for (int c0 = 0; c0 < d.B; c0 += 1024) {
            const int b = c0 + tid;
            const bool act = b < d.B && d.s_status[b] == SLOT_ACTIVE;
            int g = 0, p = 0;
            if (act) { g = d.s_game[b]; p = d.s_ply[b]; }
            const bool fl = act && cap_full_ply(d, g, p), fs = act && !fl;
            const u64 balf = __ballot(fl), bals = __ballot(fs);
            const u64 below = (1ull << lane) - 1ull;
            if (lane == 0) { wsum[wv] = __popcll(balf); wsum2[wv] = __popcll(bals); }
            __syncthreads();
            int offf = 0, totf = 0, offs = 0, tots = 0;
            for (int w = 0; w < 16; w++) {
                offf += w < wv ? wsum[w] : 0; totf += wsum[w];
                offs += w < wv ? wsum2[w] : 0; tots += wsum2[w];
            }
            const int basef = cbase_s, bases = fbase_s;
            __syncthreads();
            if (act && compact) {
                const int nb = fl ? basef + offf + __popcll(balf & below) : d.B - 1 - (bases + offs + __popcll(bals & below));
                for (int q = 0; q < 8; q++) d.cp_board[(size_t)nb * 8 + q] = d.board[(size_t)b * 8 + q];
                d.cp_state[nb * 4 + 0] = g; d.cp_state[nb * 4 + 1] = p;
                d.cp_state[nb * 4 + 2] = d.s_player[b]; d.cp_state[nb * 4 + 3] = d.s_last[b];
            }
            if (tid == 0) { cbase_s = basef + totf; fbase_s = bases + tots; }
            __syncthreads();
        }
        const int n_full = cbase_s, n_act = n_full + fbase_s;
        if (tid == 0) d.active[1] = n_full;
        if (!compact) return;
        __threadfence_block();
        __syncthreads();
        for (int b = tid; b < d.B; b += 1024) {
            if (b < n_act) {
                const int src = b < n_full ? b : d.B - 1 - (b - n_full);
                for (int q = 0; q < 8; q++) d.board[(size_t)b * 8 + q] = d.cp_board[(size_t)src * 8 + q];
                d.s_game[b] = d.cp_state[src * 4 + 0]; d.s_ply[b] = d.cp_state[src * 4 + 1];
                d.s_player[b] = d.cp_state[src * 4 + 2]; d.s_last[b] = d.cp_state[src * 4 + 3];
                d.s_status[b] = SLOT_ACTIVE;
                d.carried[b] = -1;
            } else {
                d.s_status[b] = SLOT_IDLE;
                d.s_game[b] = -1;
            }
        }
        return;
    }
    if (!compact || d.reuse) return;
    if (tid == 0) cbase_s = 0;
    __syncthreads();
    for (int c0 = 0; c0 < d.B; c0 += 1024) {
        const int b = c0 + tid;
        const bool act = b < d.B && d.s_status[b] == SLOT_ACTIVE;
        u64 bd[8];
        int g = 0, p = 0, pl = 0, la = 0;
        if (act) {
            for (int q = 0; q < 8; q++) bd[q] = d.board[(size_t)b * 8 + q];
            g = d.s_game[b]; p = d.s_ply[b]; pl = d.s_player[b]; la = d.s_last[b];
        }
        const u64 bal = __ballot(act);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();                 // every thread holds its slot in registers; the chunk's counts are known
        int off = 0, tot = 0;
        for (int w = 0; w < 16; w++) { off += w < wv ? wsum[w] : 0; tot += wsum[w]; }
        const int base = cbase_s;
        __syncthreads();
        if (act) {
            const int nb = base + off + pre;             // <= b: only slots already read are overwritten
            if (nb != b) {
                for (int q = 0; q < 8; q++) d.board[(size_t)nb * 8 + q] = bd[q];
                d.s_game[nb] = g; d.s_ply[nb] = p; d.s_player[nb] = pl; d.s_last[nb] = la;
                d.s_status[nb] = SLOT_ACTIVE;
                d.carried[nb] = -1;
            }
        }
        if (tid == 0) cbase_s = base + tot;
        __syncthreads();
    }
    for (int b = cbase_s + tid; b < d.B; b += 1024) { d.s_status[b] = SLOT_IDLE; d.s_game[b] = -1; }
}

// az_rules_replay: Gomoku.apply_action / is_terminal / get_game_result (games.py:64-82,133-179) for whole action lists,
// one thread per game, with the bit-plane helpers the search kernels use (pl_set, wins_through, pl_count).  The winner is
// sticky like the reference's cached `winner` that clone() copies (games.py:140-141,206).
__global__ void k_rules_replay(int n, int k, int rule, int games, int max_len, const short *actions, unsigned char *term_before,
                               unsigned char *boards, int *players, int *results, int *status)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= games) return;
    const int nn = n * n;
    Plane X{}, O{};
    int pl = 1, res = 0, bad = -1;
    for (int i = 0; i < max_len; i++) {
        const int a = actions[(size_t)g * max_len + i];
        if (a < 0) break;
        if (term_before) term_before[(size_t)g * max_len + i] = res != 0;
        if (a >= nn || pl_get(X, a) || pl_get(O, a)) { bad = i; break; }       // games.py:76-77 ValueError("Invalid move")
        Plane &mine = pl == 1 ? X : O;
        pl_set(mine, a);
        if (res == 0) {
            if (wins_through(mine, a, n, k, rule)) res = pl;
            else if (pl_count(X) + pl_count(O) == nn) res = 3;
        }
        pl = 3 - pl;
    }
    for (int j = 0; j < nn; j++) boards[(size_t)g * nn + j] = pl_get(X, j) ? 1 : (pl_get(O, j) ? 2 : 0);
    players[g] = pl;
    results[g] = res;
    status[g] = bad;
}
#endif  // AZ_ENGINE_TU
