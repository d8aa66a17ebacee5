// az_engine.hip -- host side of the C-ABI (include/az_engine.h): device memory, weight packing into
// MFMA fragment order, the lock-step episode loop (root eval -> S x {net, expand/backup/select} -> move),
// record export.  gfx950 only; there is no CPU implementation of the path in this library.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#define AZ_ENGINE_TU 1
#include "../../include/az_engine.h"
#include "az_launch.h"

#include "az_host.h"

static thread_local std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct PackedNet {
    bool loaded = false;
    DevBuf c1, c2, c3, hd, hdq, pf, vf, c1b, c2b, c3b, hdb, pfb, vfb, v2w, v2b;
    DevBuf rblk[6], rblkb[6];          // ResidualBlock variant: the six 64->64 convs (c1/c1b hold the stem)
    DevBuf c1x[2], c2x[2], c3x[2], hdx[2];     // the convs (c1x: conv1 / stem) and head convs split into 16-bit MFMA fragments (az_net_emul.h): [0] bf16x3, [1] f16x2
    DevBuf rblkx[2][6];                // ... and the six 64 -> 64 convs of the ResidualBlock variant
    bool f16_ok = true;                // every weight of the emulated layers is inside float16's range (AZ_TRUNK_F16X2)
    // The split fragments are packed and uploaded when a scheme is first used (az_set_trunk_mode, or az_load_weights* while
    // a scheme is selected), not on every weight load: the training loop reloads weights every episode and mostly stays on
    // the float32 trunk.  Until then the float32 weights of the emulated layers wait here.
    bool emul_ready[2] = {false, false};
    std::vector<float> hw_first, hw_conv[6], hw_pol, hw_val;
    NetWeights w{};
    ResWeights rw{};
};

// One lane = one HIP stream with its own game slots and search state.  The lanes of an engine share the weights, the
// episode's record/tape buffers and ONE queue of game ids (a device counter every lane's refill claims from), and are
// driven by one host thread each: a lane's latency-bound tree / FC kernels run underneath another lane's conv trunk.
struct Lane {
    int index = 0;
    hipStream_t stream = nullptr;
    DevState d{};                  // the games' view (B = slots of this lane)
    DevState dv{};                 // the net kernels' view (B = evaluation items = slots x leaves per batch)
    DevBuf board, s_game, s_ply, s_player, s_last, s_status, s_net, edges, rows_used, cnt, active_dev, carried;   // per slot
    DevBuf path, depth, leaf_kind, leaf, leaf_last, logits, vhid, pol_feat, dbg, scratch, it_status, it_net, leaf_sym;       // per evaluation item
    DevBuf inflight;               // per slot, deep engines with virtual-loss batching only: in-flight count of every edge
    DevBuf budget, cp_board, cp_state;     // per slot, playout cap: the ply's simulation budget, and the staging of k_refill's partition
    DevBuf root_logits, root_v;            // per slot, az_set_gumbel: the root's logits row and value of the running ply (allocated by the setter)
    DevBuf proof, root_proof, proof_stops; // per slot, az_set_solver: the status of every edge and of the root, the stops on proven edges (allocated by the setter)
    DevBuf threat_edges, threat_root, threat_depth, threat_move, threat_nodes, threat_stat;   // per slot, the root threat search (allocated on first use)
    DevBuf delta_base, delta_done, delta_cnt;     // per slot, delta evaluation (az_delta.h): allocated by the first episode that is eligible with the switch on
    // one ply (k_begin, (S+1) x {trunk, fc, step}, k_move) captured once as a hipGraph and replayed every ply:
    // 3(S+1)+2 launches (6(S+1)+2 with the split trunk) become one submission.  Indexed [split trunk][arena].
    struct PlyGraph {
        hipGraphExec_t exec = nullptr;
        LaunchCtx key{};           // kernel arguments baked into the nodes; any change re-captures
    } graph[2][2];
    std::vector<hipEvent_t> ev;    // profiling events
    // progress of the open episode
    int active = 0;                // active slots after the last refill
    int n_full = 0;                // playout cap: how many of them search a FULL ply next (the first n_full after a compacting refill)
    int refill_out[2] = {0, 0};    // what k_refill reports: active slots, FULL ones among them
    int cur = 0;                   // slots the next ply is launched over: all of them, or (after a compacting refill) the active ones
    int plies_played = 0;          // plies this lane has played in the open episode
    int64_t steps = 0, trunk_launches = 0, plies = 0;
    double trunk_ms = 0.0, nn_ms = 0.0, step_ms = 0.0;
    double tape_wait_s = 0.0;      // host time this lane's thread was blocked on a tape wave (production or its upload)
    int rc = AZ_OK;                // result of the last threaded call on this lane
    int preset_m = 0;              // preset episodes (preset_search): the first preset_m slots hold given positions
    std::string err;
};

struct az_engine {
    az_config cfg{};
    int n = 0, nn = 0, RW = 0, R = 0, PATH = 0, num_cus = 256;
    std::string err;
    hipStream_t stream = nullptr;  // lane 0's stream: uploads and copies of the shared buffers
    const SizeOps *ops = nullptr;
    std::vector<Lane> lanes;
    // shared by the lanes: tables, the game-id queue, the episode's tapes and records
    DevBuf T_table, log_table, sqrt_table, noise_off, next_game;
    DevBuf noise, u, rec_planes, rec_last, rec_action, rec_mover, rec_pi, rec_visits, g_nply, g_result, src_index;
    DevBuf rec_value, g_cross;     // the search value of every record and the first crossing ply of every game (az_set_resign)
    int split_max = 64;            // use the tile-split (low-latency) trunk when at most this many slots of a lane are active (measured: 32 / 64 / 128 -> 102.0 / 102.3 / 101.0 games per second on the 1024-game episode; the 51-game arena 3.08 / 1.64 / 1.64 s)
    int episode_games = 0;
    int64_t tape_len = 0;          // doubles per game in the noise tape
    bool have_episode = false;
    int reuse = 0;
    bool deep = false;             // created by az_create_deep: num_simulations up to AZ_DEEP_MAX_SIMULATIONS
    int vl = 1;                    // leaves per game and evaluation batch (az_set_virtual_loss); 1 = the reference's sequential loop
    bool vl_kernel = false;        // the batched tree kernel is in use (vl > 1, or AZ_VL_FORCE=1 to run it with batches of one)
    bool persist_allowed = true;   // AZ_PERSIST=0: never use the persistent search kernel
    int leaf_symmetry = 0;         // az_set_leaf_symmetry: every evaluation shows the net a pseudo-random dihedral symmetry of the position
    int trunk_mode = AZ_TRUNK_F32; // az_set_trunk_mode: AZ_TRUNK_BF16X3 / AZ_TRUNK_F16X2 = the convs on the 16-bit MFMAs with split operands
    int persist_gp = 0;            // games per workgroup of the persistent search kernel for the open episode, 0 = lock-step pipeline
    DevBuf cache;                  // evaluation cache shared by the lanes (az_set_eval_cache)
    // az_set_external_evaluator: the caller's buffers and callback, the request's item map and count on the device, and
    // the requests / items of the last (or open) episode
    struct Ext {
        bool on = false;
        az_ext_evaluator ev{};
        DevBuf map, count;
        int64_t requests = 0, items = 0;
    } ext;
    // preset searches (az_search*), all sized by the slots: the wave's positions, temperatures and compact root statistics, and
    // the all-zero noise_off table that makes row g of the [wave][n*n] noise upload the tape of game g
    DevBuf bt_cells, bt_players, bt_lasts, bt_T, bt_zero_off, bt_visits, bt_W, bt_prior, bt_pi, bt_action;
    // az_search_callback: the buffers of the engine's own external evaluator, slots x leaves per batch entries as episode_begin
    // asks of any (allocated by the first callback search)
    DevBuf cb_planes, cb_policy, cb_value;
    unsigned cache_mask = 0, cache_gen = 1;
    // az_set_start_positions: the device table k_refill loads claimed games from, and each position's stone count on the host
    DevBuf start_tab;
    int start_count = 0, start_first = 0, start_max_ply = 0;     // start_first = first mod 2 * start_count
    std::vector<int> start_ply;
    // last episode per game: plies searched, result, and the ply the game started at (the device keeps absolute plies:
    // the records of game g sit at g * nn + h_start[g] + 0 .. h_nply[g])
    std::vector<int> h_nply, h_result, h_start;
    std::vector<int> h_cross;      // first crossing ply per game of the last episode (absolute ply), -1 = none
    unsigned h_key0 = 0;           // ... and the episode's game_key0 and playout share, what az_selfplay_resign_info names the exempt games by
    int h_permille = 0;
    // az_set_resign: 0 = off
    double resign_thr = 0.0;
    int resign_min_ply = 0, resign_permille = 0;
    // az_set_win_rule: AZ_RULE_FREESTYLE (the reference's game) | AZ_RULE_EXACT (standard Gomoku)
    int win_rule = AZ_RULE_FREESTYLE;
    // az_set_playout_cap: 0 = off; and what the last episode ran under (az_selfplay_sims and the export filter go by the hash)
    int cap_fast = 0, cap_permille = 0, cap_export_full = 0;
    int h_cap_fast = 0, h_cap_permille = 0, h_cap_export_full = 0;
    // az_set_forced_playouts: 0.0 = off
    double forced_k = 0.0;
    int forced_prune = 0;
    // az_set_gumbel: m = 0 = off; the schedule table u16[m][S] lives on the device
    int gumbel_m = 0;
    double gumbel_cv = 50.0, gumbel_cs = 1.0;
    DevBuf gumbel_seq;
    // az_set_selection: 0 = off; the parameters stay as last set; the two tables live on the device while it is on
    int sel_on = 0;
    double sel_fpu = 0.0, sel_fpu_root = 0.0, sel_base = 19652.0, sel_factor = 0.0;
    DevBuf sel_cpuct, sel_mass;
    // az_set_candidates: the Chebyshev radius, 0 = off
    int cand_radius = 0;
    // az_set_solver: 0 = off; the root status of every record, and what az_last_proof hands out (the root rows and root
    // statuses of the last az_search / az_search_batch, occupied cells 0)
    int solver = 0;
    int64_t solver_stops = 0;      // simulations of the last (or open) episode / search call that ended on a proven edge
    int episode_solver = 0;        // ... and whether the last (or open) episode ran with it: az_selfplay_proofs speaks of that one
    DevBuf rec_proof;
    std::vector<int8_t> proof_edges, proof_roots;
    // az_set_threat_search: max_depth = 0 = off; the depth of every record's root; the sums of the last (or open) episode / search call
    int threat_depth = 0, threat_budget = 0;
    int episode_threat = 0;        // whether the last (or open) episode ran with it: az_selfplay_threats speaks of that one
    DevBuf rec_threat;
    int64_t threat_stats[THREAT_STATS] = {0, 0, 0, 0, 0};
    // az_set_delta_eval: leaves evaluated as deltas from the ply's root activations where the episode is eligible (delta_eligible)
    bool delta_on = true;
    int delta_tiles = DELTA_TILES_DEFAULT;
    int64_t delta_stats[DELTA_CNT] = {};       // of the last (or open) episode: delta, full, conv3 tiles, base evaluations, delta evaluations by tile count
    PackedNet net[2];
    az_counters last{};
    // running episode (az_selfplay_begin .. az_selfplay_end)
    struct Run {
        bool open = false;
        int num_games = 0, max_plies = 0;
        bool add_noise = true, arena = false, preset = false, profile = true;
        bool ext = false;          // the episode's evaluations go to the external evaluator (az_set_external_evaluator)
        bool delta = false;        // the episode's lock-step trunk launches are base + delta evaluations (az_delta.h)
        int ext_net = -1;          // net id its requests carry instead of the items' own (az_search*: the slot argument), -1 = the items'
        az_counters c{};
        int64_t reused_roots = 0;
        unsigned game_key0 = 0;
        int cap_fast = 0, cap_permille = 0, cap_export_full = 0;     // the playout cap of this episode (self-play only), 0 = off
        std::vector<int> start;    // ply every game starts at (az_set_start_positions); empty = 0 for all
    } run;
    bool profile = false;          // HIP events around every trunk / FC launch (az_set_profiling); lanes then play one after another
    bool use_graph = true;         // AZ_GRAPH=0: launch kernel by kernel
    bool compact = true;           // AZ_COMPACT=0: never move the active slots to the front between plies (k_refill)
    void *comm = nullptr;          // RCCL communicator of az_dist_init (ncclComm_t), one rank per engine
    int dist_rank = 0, dist_world = 1;
    DevBuf dist_buf, dist_pack;    // small device scratch of the collectives; this rank's packed records
    TapeProducer *tapes = nullptr; // running while a self-play episode with engine-generated tapes is open
    bool stream_tapes = true;      // AZ_TAPE_STREAM=0: generate every tape before the first ply
    int tape_threads = 4;          // AZ_TAPE_THREADS: host threads of the tape producer
    int host_cpus = 1;             // CPUs this process may run on (affinity mask and cgroup quota), what the thread counts are sized from
    int rng_mode = AZ_RNG_NUMPY;   // az_set_rng: AZ_RNG_PHILOX fills the tapes with k_tape instead of the host producer
};

// az_philox.hip: k_tape over plies [m0, m1) of games seed0 + [0, G), on `stream`
hipError_t az_tape_launch(hipStream_t stream, uint64_t seed0, int G, int nn, int m0, int m1, double alpha, int kind, const int *done,
                          double *noise, int64_t noise_stride, double *u);

static void stop_tapes(az_engine *e)
{
    if (e->tapes) { e->tapes->shutdown(); delete e->tapes; e->tapes = nullptr; }
}

static LaunchCtx ctx_of_impl(const az_engine *e, const Lane &L)
{
    LaunchCtx c{};
    c.stream = L.stream;
    c.d = L.d;
    c.dv = L.dv;
    for (int i = 0; i < 2; i++) { c.w[i] = e->net[i].w; c.rw[i] = e->net[i].rw; }
    c.model = e->cfg.model;
    c.synthetic = e->cfg.eval_kind == AZ_EVAL_SYNTHETIC;
    c.persist_gp = e->persist_gp;
    c.vl_kernel = e->vl_kernel ? 1 : 0;
    c.emul = e->trunk_mode;        // AZ_TRUNK_F32 = 0, AZ_TRUNK_BF16X3 = EMUL_BF16X3, AZ_TRUNK_F16X2 = EMUL_F16X2
    c.feat = (float *)L.pol_feat.p;
    c.dbg = (unsigned long long *)L.dbg.p;
    c.scratch = (float *)L.scratch.p;
    c.inflight = (unsigned char *)L.inflight.p;
    if (e->run.delta && L.delta_base.p) {
        c.delta_base = (float *)L.delta_base.p;
        c.delta_done = (unsigned char *)L.delta_done.p;
        c.delta_cnt = (unsigned long long *)L.delta_cnt.p;
        c.delta_tiles = e->delta_tiles;
    }
    return c;
}

// ------------------------------------------------------------------------------------------------
static int fail(az_engine *e, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf; else g_create_error = buf;
    return code;
}
#define HIPCHECK(e, call)                                                                          \
    do {                                                                                           \
        hipError_t _r = (call);                                                                    \
        if (_r != hipSuccess)                                                                      \
            return fail(e, AZ_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

// The HIP current device is thread-local state the caller's framework (PyTorch) shares with this library: every entry
// point selects the engine's device for its own duration and puts the caller's device back on return.
struct DeviceGuard {
    int prev = -1;
    hipError_t rc;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        rc = prev == dev ? hipSuccess : hipSetDevice(dev);
        if (prev == dev) prev = -1;          // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define DEVICE_GUARD(e)                                                                            \
    DeviceGuard _guard((e)->cfg.device);                                                           \
    if (_guard.rc != hipSuccess) return fail(e, AZ_ERR_HIP, "hipSetDevice(%d) failed: %s", (e)->cfg.device, hipGetErrorString(_guard.rc))

static int dev_alloc(az_engine *e, DevBuf &b, size_t bytes, bool zero = true)
{
    if (b.p && b.bytes >= bytes) {
        if (zero) HIPCHECK(e, hipMemsetAsync(b.p, 0, bytes, e->stream));
        return AZ_OK;
    }
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    if (bytes == 0) bytes = 16;
    HIPCHECK(e, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    if (zero) HIPCHECK(e, hipMemsetAsync(b.p, 0, bytes, e->stream));
    return AZ_OK;
}
static void dev_free(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}
// one allocation of a run that stops at the first failure: the caller has `e` and an `int rc`; further arguments as dev_alloc
#define ALLOC(buf, ...) if (!rc) rc = dev_alloc(e, buf, __VA_ARGS__)

// Per-slot buffers an option brings with it: every lane gets the ones it does not have yet (zeroed), sized by its slots, then
// one stream sync.  rezero: a buffer that is already there is zeroed again.
struct LaneBuf {
    DevBuf Lane::*buf;
    size_t bytes_per_slot;
    bool rezero;
};
static int ensure_lane_buffers(az_engine *e, std::initializer_list<LaneBuf> list)
{
    int rc = AZ_OK;
    for (Lane &L : e->lanes)
        for (const LaneBuf &a : list)
            if (!(L.*a.buf).p || a.rezero) ALLOC(L.*a.buf, (size_t)L.d.B * a.bytes_per_slot);
    if (rc) return rc;
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    return AZ_OK;
}
// Blocking copies go through the engine's own (non-blocking) stream: nothing in the engine touches the legacy null
// stream, whose implicit synchronisation would couple the engines of a process to each other and to PyTorch's work.
static hipError_t az_memcpy(hipStream_t s, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    hipError_t rc = hipMemcpyAsync(dst, src, bytes, kind, s);
    return rc == hipSuccess ? hipStreamSynchronize(s) : rc;
}
static hipError_t az_memcpy2d(hipStream_t s, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                              size_t height, hipMemcpyKind kind)
{
    hipError_t rc = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, s);
    return rc == hipSuccess ? hipStreamSynchronize(s) : rc;
}
static int upload(az_engine *e, DevBuf &b, const void *src, size_t bytes)
{
    int rc = dev_alloc(e, b, bytes, false);
    if (rc) return rc;
    HIPCHECK(e, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    return AZ_OK;
}

// ------------------------------------------------------------------------------------------------
// Settings that cannot be combined: every pair once, with the text both setters refuse it with.  A setter that switches
// its setting ON calls refuse_conflicts; the first row with an active partner names the error.
// ------------------------------------------------------------------------------------------------
enum Setting {
    SET_REUSE, SET_VL, SET_VL_KERNEL, SET_SYMMETRY, SET_EXT, SET_CAP, SET_FORCED, SET_GUMBEL, SET_SOLVER, SET_SELECTION, SET_CANDIDATES,
    SET_SYNTHETIC, SET_NO_NET          // facts of az_config: the synthetic evaluator; any evaluator but the net
};
static const struct { Setting a, b; const char *message; } g_conflicts[] = {
    {SET_REUSE, SET_VL, "subtree reuse and virtual-loss batching cannot be combined"},
    {SET_REUSE, SET_EXT, "subtree reuse and the external evaluator cannot be combined"},
    {SET_CAP, SET_REUSE, "the playout cap and subtree reuse cannot be combined"},
    {SET_FORCED, SET_REUSE, "forced playouts and subtree reuse cannot be combined"},
    {SET_GUMBEL, SET_REUSE, "the Gumbel root search and subtree reuse cannot be combined"},
    {SET_SOLVER, SET_REUSE, "the solver and subtree reuse cannot be combined"},
    {SET_CAP, SET_EXT, "the playout cap and the external evaluator cannot be combined"},
    {SET_SYMMETRY, SET_NO_NET, "random-symmetry leaf evaluation needs the net evaluator"},
    {SET_SYMMETRY, SET_EXT, "random-symmetry leaf evaluation and the external evaluator cannot be combined"},
    {SET_GUMBEL, SET_VL_KERNEL, "the Gumbel root search and virtual-loss batching cannot be combined"},
    {SET_FORCED, SET_GUMBEL, "forced playouts and the Gumbel root search cannot be combined"},
    {SET_GUMBEL, SET_EXT, "the Gumbel root search and the external evaluator cannot be combined (it returns priors, not logits)"},
    {SET_GUMBEL, SET_SYNTHETIC, "the Gumbel root search needs a net: the synthetic evaluator has no logits"},
    {SET_SOLVER, SET_VL_KERNEL, "the solver and virtual-loss batching cannot be combined"},
    {SET_SOLVER, SET_FORCED, "the solver and forced playouts cannot be combined"},
    {SET_SOLVER, SET_GUMBEL, "the solver and the Gumbel root search cannot be combined"},
    {SET_SOLVER, SET_EXT, "the solver and the external evaluator cannot be combined"},
    {SET_SOLVER, SET_SYNTHETIC, "the solver and the synthetic evaluator cannot be combined"},
    {SET_SELECTION, SET_REUSE, "the selection rule and subtree reuse cannot be combined (a retained root has no fresh value)"},
    {SET_SELECTION, SET_SOLVER, "the selection rule and the solver cannot be combined"},
    {SET_SELECTION, SET_GUMBEL, "the selection rule and the Gumbel root search cannot be combined"},
    {SET_CANDIDATES, SET_REUSE, "candidate moves and subtree reuse cannot be combined (a retained root's priors and noise were not made under the rule)"},
    {SET_CANDIDATES, SET_GUMBEL, "candidate moves and the Gumbel root search cannot be combined (its top-m and target are defined over the legal cells)"},
    {SET_CANDIDATES, SET_SOLVER, "candidate moves and the solver cannot be combined (every move loses is no proof when moves were left out)"},
    {SET_CANDIDATES, SET_SELECTION, "candidate moves and the selection rule cannot be combined yet"},
    {SET_CANDIDATES, SET_EXT, "candidate moves and the external evaluator cannot be combined (it returns priors, not logits)"},
};

// bit s = setting s is on.  Virtual-loss batching has two: more than one leaf per batch, and the batched tree kernel being in
// use at all (AZ_VL_FORCE=1 runs it with batches of one), which is what the Gumbel root search and the solver go by.
static unsigned active_settings(const az_engine *e)
{
    const bool on[] = {e->reuse != 0, e->vl > 1, e->vl > 1 || e->vl_kernel, e->leaf_symmetry != 0, e->ext.on, e->cap_fast != 0,
                       e->forced_k > 0.0, e->gumbel_m > 0, e->solver != 0, e->sel_on != 0, e->cand_radius != 0,
                       e->cfg.eval_kind == AZ_EVAL_SYNTHETIC, e->cfg.eval_kind != AZ_EVAL_NET};
    unsigned m = 0;
    for (int s = 0; s <= SET_NO_NET; s++) m |= on[s] ? 1u << s : 0u;
    return m;
}

static int refuse_conflicts(az_engine *e, Setting s)
{
    const unsigned active = active_settings(e);
    for (const auto &c : g_conflicts)
        if ((c.a == s && (active >> c.b & 1u)) || (c.b == s && (active >> c.a & 1u))) return fail(e, AZ_ERR_INVALID, "%s", c.message);
    return AZ_OK;
}

// ------------------------------------------------------------------------------------------------
// weight packing:B-operand fragments of v_mfma_f32_16x16x4_f32.  Lane l supplies B[k = l>>4][j = l&15]
// of k-step s; four consecutive k-steps are stored together so one dwordx4 load feeds four MFMAs:
//   packed[((ntile*KS4 + s/4)*64 + lane)*4 + s%4]
// ------------------------------------------------------------------------------------------------
static std::vector<float> pack_conv(const float *w, int cout, int cin)
{
    // torch [co][ci][ky][kx]; k-step s = tap*(cin/4) + s', ci = 4*s' + (lane>>4)
    const int kst = cin / 4, ks = 9 * kst, ks4 = (ks + 3) / 4, nt = cout / 16;
    std::vector<float> out((size_t)nt * ks4 * 64 * 4, 0.0f);
    for (int t = 0; t < nt; t++)
        for (int s = 0; s < ks; s++)
            for (int lane = 0; lane < 64; lane++) {
                int tap = s / kst, sp = s % kst;
                int ci = 4 * sp + (lane >> 4), co = t * 16 + (lane & 15);
                out[(((size_t)t * ks4 + s / 4) * 64 + lane) * 4 + (s % 4)] = w[((size_t)co * cin + ci) * 9 + tap];
            }
    return out;
}
// fp32-emulating trunks (az_net_emul.h): A-operand fragments of the 16-bit MFMAs with every weight split into parts.
//   scheme 1 (AZ_TRUNK_BF16X3): w = hi + mid + lo, three bfloat16 parts, each the round-to-nearest-even bf16 of what the
//                               previous parts left over;
//   scheme 2 (AZ_TRUNK_F16X2):  w = hi + lo / 2048, two float16 parts, lo stored scaled by 2^11.
// Conv layers: lane l supplies A[row = l & 15][k = 8 (l >> 4) + j]; K-block kb = one tap x 32 input channels:
//   packed[(((ntile * KB + kb) * NS + part) * 64 + lane) * 8 + j]
static inline uint16_t bf16_rne(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_val(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline uint16_t f16_rne(float x)
{
    const _Float16 h = (_Float16)x;             // round to nearest even
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static inline float f16_val(uint16_t u)
{
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}
static inline int emul_parts(int scheme) { return scheme == AZ_TRUNK_F16X2 ? 2 : 3; }
// the parts of one weight; false when the value is outside the scheme's range
static inline bool emul_split(int scheme, float x, uint16_t *parts)
{
    if (scheme == AZ_TRUNK_F16X2) {
        if (!(std::fabs(x) < 65504.0f)) { parts[0] = parts[1] = 0; return false; }
        parts[0] = f16_rne(x);
        parts[1] = f16_rne((x - f16_val(parts[0])) * 2048.0f);
        return true;
    }
    parts[0] = bf16_rne(x);
    const float r1 = x - bf16_val(parts[0]);
    parts[1] = bf16_rne(r1);
    parts[2] = bf16_rne(r1 - bf16_val(parts[1]));
    return true;
}
// the first conv (cin = 4, K = 36 padded to two K-blocks of 32): k = tap * 4 + plane
static std::vector<uint16_t> pack_first_emul(int scheme, const float *w, int cout, bool *ok)
{
    const int ns = emul_parts(scheme), nt = cout / 16;
    std::vector<uint16_t> out((size_t)nt * 2 * ns * 64 * 8, 0);
    for (int t = 0; t < nt; t++)
        for (int kb = 0; kb < 2; kb++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int k = kb * 32 + 8 * (lane >> 4) + j, co = t * 16 + (lane & 15);
                    if (k >= 36) continue;
                    uint16_t parts[3];
                    if (!emul_split(scheme, w[((size_t)co * 4 + (k & 3)) * 9 + (k >> 2)], parts)) *ok = false;
                    const size_t base = (((size_t)t * 2 + kb) * ns * 64 + lane) * 8 + j;
                    for (int s2 = 0; s2 < ns; s2++) out[base + (size_t)s2 * 64 * 8] = parts[s2];
                }
    return out;
}
static std::vector<uint16_t> pack_conv_emul(int scheme, const float *w, int cout, int cin, bool *ok)
{
    const int ns = emul_parts(scheme), kbt = cin / 32, kb_n = 9 * kbt, nt = cout / 16;
    std::vector<uint16_t> out((size_t)nt * kb_n * ns * 64 * 8, 0);
    for (int t = 0; t < nt; t++)
        for (int kb = 0; kb < kb_n; kb++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int tap = kb / kbt, ci = (kb % kbt) * 32 + 8 * (lane >> 4) + j, co = t * 16 + (lane & 15);
                    uint16_t parts[3];
                    if (!emul_split(scheme, w[((size_t)co * cin + ci) * 9 + tap], parts)) *ok = false;
                    const size_t base = (((size_t)t * kb_n + kb) * ns * 64 + lane) * 8 + j;
                    for (int s2 = 0; s2 < ns; s2++) out[base + (size_t)s2 * 64 * 8] = parts[s2];
                }
    return out;
}
// The 1x1 head convs for the fused epilogue of the last emulated conv: A-operand fragments of the 16x16x16 MFMA, one per
// 16-channel tile of that conv's output; lane l supplies A[row = l & 15 = head channel][k = 4 (l >> 4) + j] = w[row][16 tile + k]:
//   packed[((tile * NS + part) * 64 + lane) * 4 + j]
static std::vector<uint16_t> pack_heads_emul(int scheme, const float *pw, int pc, const float *vw, int vc, int cin, bool *ok)
{
    const int ns = emul_parts(scheme), nt = cin / 16;
    std::vector<uint16_t> out((size_t)nt * ns * 64 * 4, 0);
    for (int t = 0; t < nt; t++)
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 4; j++) {
                const int row = lane & 15, ci = 16 * t + 4 * (lane >> 4) + j;
                const float x = row < pc ? pw[row * cin + ci] : (row < pc + vc ? vw[(row - pc) * cin + ci] : 0.0f);
                uint16_t parts[3];
                if (!emul_split(scheme, x, parts)) *ok = false;
                const size_t base = ((size_t)t * ns * 64 + lane) * 4 + j;
                for (int s2 = 0; s2 < ns; s2++) out[base + (size_t)s2 * 64 * 4] = parts[s2];
            }
    return out;
}
static std::vector<float> pack_heads(const float *pw, int pc, const float *vw, int vc, int cin)
{
    // policy_conv [pc][cin], value_conv [vc][cin] -> rows of one 16-row tile, cin/4 k-steps
    const int ks = cin / 4;
    std::vector<float> out((size_t)(ks / 4) * 64 * 4, 0.0f);
    for (int s = 0; s < ks; s++)
        for (int lane = 0; lane < 64; lane++) {
            int ci = 4 * s + (lane >> 4), j = lane & 15;
            float v = j < pc ? pw[j * cin + ci] : (j < pc + vc ? vw[(j - pc) * cin + ci] : 0.0f);
            out[(((size_t)s / 4) * 64 + lane) * 4 + (s % 4)] = v;
        }
    return out;
}
static std::vector<float> pack_heads_blocks(const float *pw, const float *vw)
{
    // the plain net's policy_conv [4][128] and value_conv [2][128] for the 4-row blocks of v_mfma_f32_4x4x1_16b_f32 (trunk_heads):
    // [k/4][8 rows][4] -- rows 0-3 policy_conv, 4-5 value_conv, 6-7 zeros; a lane takes four consecutive channels of its row at once
    std::vector<float> out(32 * 8 * 4, 0.0f);
    for (int k = 0; k < 128; k++)
        for (int r = 0; r < 6; r++)
            out[((size_t)(k / 4) * 8 + r) * 4 + (k % 4)] = r < 4 ? pw[r * 128 + k] : vw[(r - 4) * 128 + k];
    return out;
}
static std::vector<float> pack_fc(const float *w, int nout, int kin)
{
    // torch Linear [out][in]; tile t covers outputs 16t..16t+15; k-step s covers k = 4s..4s+3; group = 4 k-steps = 16 inputs.
    // Canonical order (az_net.h fc_chain_groups): 4 chains of qg groups each, zero-padded: [tile][4 qg][lane][4]
    const int nt = (nout + 15) / 16, ks = (kin + 3) / 4, qg = (((kin + 15) / 16) + 3) / 4, ks4 = 4 * qg;
    std::vector<float> out((size_t)nt * ks4 * 64 * 4, 0.0f);
    for (int t = 0; t < nt; t++)
        for (int s = 0; s < ks; s++)
            for (int lane = 0; lane < 64; lane++) {
                int k = 4 * s + (lane >> 4), j = t * 16 + (lane & 15);
                float v = (j < nout && k < kin) ? w[(size_t)j * kin + k] : 0.0f;
                out[(((size_t)t * ks4 + s / 4) * 64 + lane) * 4 + (s % 4)] = v;
            }
    return out;
}

// ------------------------------------------------------------------------------------------------
// kernel dispatch by board size: one translation unit per size (az_kernels.hip), selected once at az_create
// ------------------------------------------------------------------------------------------------
const SizeOps *az_size_ops(int n)
{
    switch (n) {
#define AZ_CASE(k) case k: return az_size_ops_##k ? az_size_ops_##k() : nullptr;
    AZ_CASE(3) AZ_CASE(4) AZ_CASE(5) AZ_CASE(6) AZ_CASE(7) AZ_CASE(8) AZ_CASE(9) AZ_CASE(10) AZ_CASE(11) AZ_CASE(12)
    AZ_CASE(13) AZ_CASE(14) AZ_CASE(15)
#undef AZ_CASE
    default: return nullptr;
    }
}


// ------------------------------------------------------------------------------------------------
// packed records + examples (self_play.py:94-108 augmentation fused into the encode)
// record layout: [8 x u64 planes (mover, opponent)] [pi f32 x nn] [last i16] [mover u8] [z i8], padded to 8 B
// ------------------------------------------------------------------------------------------------
static inline int64_t record_bytes(int nn) { return ((64 + 4 * (int64_t)nn + 4) + 7) / 8 * 8; }

__global__ void k_pack(DevState d, const int *src_index, int64_t records, int nn, int64_t rb, unsigned char *out)
{
    int64_t r = blockIdx.x;
    if (r >= records) return;
    int si = src_index[r];
    int g = si / nn;
    unsigned char *o = out + r * rb;
    u64 *op = reinterpret_cast<u64 *>(o);
    float *opi = reinterpret_cast<float *>(o + 64);
    if (threadIdx.x < 8) op[threadIdx.x] = d.rec_planes[(size_t)si * 8 + threadIdx.x];
    for (int j = threadIdx.x; j < nn; j += blockDim.x) opi[j] = d.rec_pi[(size_t)si * nn + j];
    if (threadIdx.x == 0) {
        short *ol = reinterpret_cast<short *>(o + 64 + 4 * nn);
        ol[0] = d.rec_last[si];
        int mover = d.rec_mover[si], res = d.g_result[g];
        o[64 + 4 * nn + 2] = (unsigned char)mover;
        // self_play.py:71: 0 if draw, +1 if the mover won, -1 otherwise; 99 marks a game cut by max_plies
        reinterpret_cast<signed char *>(o)[64 + 4 * nn + 3] = (signed char)(res == 0 ? 99 : (res == 3 ? 0 : (mover == res ? 1 : -1)));
    }
}

// the search value of every packed record, in k_pack's order
__global__ void k_pack_values(const float *__restrict__ rec_value, const int *__restrict__ src_index, int64_t records, float *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < records) out[r] = rec_value[src_index[r]];
}

__global__ void k_examples(const unsigned char *packed, int64_t records, int n, int64_t rb, int aug, float *states,
                           float *pis, float *zs)
{
    const int nn = n * n;
    int64_t r = blockIdx.x;
    if (r >= records) return;
    const unsigned char *o = packed + r * rb;
    const u64 *pl = reinterpret_cast<const u64 *>(o);
    const float *pi = reinterpret_cast<const float *>(o + 64);
    const int last = reinterpret_cast<const short *>(o + 64 + 4 * nn)[0];
    const int z = reinterpret_cast<const signed char *>(o)[64 + 4 * nn + 3];
    for (int k = 0; k < aug; k++) {
        float *so = states + ((size_t)r * aug + k) * 4 * nn;
        float *po = pis + ((size_t)r * aug + k) * nn;
        for (int c = threadIdx.x; c < nn; c += blockDim.x) {
            int i = c / n, j = c - i * n;
            int src = sym_src(k, i, j, n);
            so[c] = ((pl[src >> 6] >> (src & 63)) & 1ull) ? 1.0f : 0.0f;            // games.py:117-124
            so[nn + c] = ((pl[4 + (src >> 6)] >> (src & 63)) & 1ull) ? 1.0f : 0.0f;
            so[2 * nn + c] = (src == last) ? 1.0f : 0.0f;                              // games.py:126-128
            so[3 * nn + c] = 0.0f;
            // reference mode (aug == 4): pi is rotated exactly once for every k (self_play.py:105)
            int psrc = aug == AZ_AUG_REFERENCE4 ? sym_src(1, i, j, n) : src;
            po[c] = pi[psrc];
        }
        if (threadIdx.x == 0) zs[(size_t)r * aug + k] = (float)z;
    }
}

// Training batch straight from a device-resident ring of packed records: example i = symmetry sym[i] of record
// idx[i] (replay_buffer.py:26-39 sample_batch + controller.py:23-31 collate, without the host round trip).
__global__ void k_examples_gather(const unsigned char *packed, const long long *idx, const int *sym, int count, int n,
                                  int64_t rb, int reference_pi, float *states, float *pis, float *zs)
{
    const int nn = n * n;
    const int i = blockIdx.x;
    if (i >= count) return;
    const unsigned char *o = packed + idx[i] * rb;
    const u64 *pl = reinterpret_cast<const u64 *>(o);
    const float *pi = reinterpret_cast<const float *>(o + 64);
    const int last = reinterpret_cast<const short *>(o + 64 + 4 * nn)[0];
    const int z = reinterpret_cast<const signed char *>(o)[64 + 4 * nn + 3];
    const int k = sym[i];
    float *so = states + (size_t)i * 4 * nn;
    float *po = pis + (size_t)i * nn;
    for (int c = threadIdx.x; c < nn; c += blockDim.x) {
        int r = c / n, q = c - r * n;
        int src = sym_src(k, r, q, n);
        so[c] = ((pl[src >> 6] >> (src & 63)) & 1ull) ? 1.0f : 0.0f;
        so[nn + c] = ((pl[4 + (src >> 6)] >> (src & 63)) & 1ull) ? 1.0f : 0.0f;
        so[2 * nn + c] = (src == last) ? 1.0f : 0.0f;
        so[3 * nn + c] = 0.0f;
        po[c] = pi[reference_pi ? sym_src(1, r, q, n) : src];
    }
    if (threadIdx.x == 0) zs[i] = (float)z;
}

// ------------------------------------------------------------------------------------------------
// lifecycle
// ------------------------------------------------------------------------------------------------
extern "C" const char *az_last_error(const az_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

static int setup_tables(az_engine *e)
{
    const int S = e->cfg.num_simulations, nn = e->nn;
    std::vector<float> lt(S + 2);
    for (int i = 0; i <= S + 1; i++) lt[i] = e->cfg.log_table && i <= S ? e->cfg.log_table[i] : logf((float)i + 1e-8f);
    std::vector<double> st(S + 3);
    for (int i = 0; i <= S + 2; i++) st[i] = std::sqrt((double)i + 1e-8);
    std::vector<int> no(nn + 2);
    int off = 0;
    for (int m = 0; m <= nn; m++) { no[m] = off; off += nn - m; }
    e->tape_len = off;
    int rc;
    if ((rc = upload(e, e->log_table, lt.data(), lt.size() * sizeof(float)))) return rc;
    if ((rc = upload(e, e->sqrt_table, st.data(), st.size() * sizeof(double)))) return rc;
    if ((rc = upload(e, e->noise_off, no.data(), no.size() * sizeof(int)))) return rc;
    return AZ_OK;
}

// lanes of an engine when the caller leaves it to the library: small boards are launch-bound (one lane); otherwise one
// lane per 128 slots up to four (measured at 15x15 / 1024 slots: 1/2/3/4/6/8 lanes -> 2.38/2.47/2.53/2.58/1.95/2.11 M exp/s)
static int auto_lanes(int n, int slots)
{
    if (n <= 5) return 1;
    const int k = slots / 128;
    return k < 1 ? 1 : (k > 4 ? 4 : k);
}

// CPUs this process may run on: the affinity mask, capped by the cgroup CPU quota (v2 cpu.max, v1 cpu.cfs_quota_us);
// std::thread::hardware_concurrency() knows about neither on every libstdc++
static int usable_cpus()
{
    int n = 0;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    if (n <= 0) n = 1;
    double quota = 0.0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char a[64] = {0};
        long long period = 0;
        if (fscanf(f, "%63s %lld", a, &period) == 2 && strcmp(a, "max") != 0 && period > 0) quota = atof(a) / (double)period;
        fclose(f);
    } else if (FILE *f1 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        long long q = -1, period = 0;
        if (fscanf(f1, "%lld", &q) != 1) q = -1;
        fclose(f1);
        if (FILE *f2 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (fscanf(f2, "%lld", &period) != 1) period = 0;
            fclose(f2);
        }
        if (q > 0 && period > 0) quota = (double)q / (double)period;
    }
    if (quota >= 1.0 && quota < (double)n) n = (int)quota;
    return n;
}

// every lane's DevState carries the shared pointers and scalars
template <class F>
static void each_state(az_engine *e, F f)
{
    for (Lane &L : e->lanes) {
        f(L.d);
        L.dv = L.d;                                  // the net kernels see evaluation items instead of slots
        L.dv.B = L.d.B * L.d.L;
        L.dv.s_status = L.d.it_status;
        L.dv.s_net = L.d.it_net;
    }
}

// (re)allocates the per-item buffers of a lane for `leaves` leaves per game and batch
static int alloc_items(az_engine *e, Lane &L, int leaves)
{
    const size_t NI = (size_t)L.d.B * leaves;
    int rc = AZ_OK;
    ALLOC(L.path, (NI * (size_t)e->PATH + 64) * 4);   // +64: k_step's speculative path[lane] read of the last slot
    ALLOC(L.depth, NI * 4);
    ALLOC(L.leaf_kind, NI * 4); ALLOC(L.leaf, NI * 8 * sizeof(u64)); ALLOC(L.leaf_last, NI * 4); ALLOC(L.leaf_sym, NI * 4);
    ALLOC(L.logits, NI * (size_t)e->RW * 4); ALLOC(L.vhid, NI * 64 * 4);
    ALLOC(L.pol_feat, NI * (size_t)((((e->cfg.model == AZ_MODEL_RESNET ? 3 : 6) * e->nn + 3) / 4) * 4) * 4);   // feature rows [NI][FROW], zero tail stays zero
#ifdef AZ_STAMPS
    ALLOC(L.dbg, (NI * 16 + 4096 * 32 + NI * 32) * sizeof(unsigned long long));     // trunk stamps | k_fc stamps | conv3 per-wave stamps
#endif
    if (e->split_max > 0)    // zeroed once: the padding ring of the packed images is never written afterwards
        ALLOC(L.scratch, (size_t)e->ops->split_scratch_floats((int)NI, e->cfg.model) * sizeof(float));
    if (leaves > 1) { ALLOC(L.it_status, NI * 4); ALLOC(L.it_net, NI * 4); }
    if (rc) return rc;
    DevState &d = L.d;
    d.L = leaves;
    d.path = (unsigned *)L.path.p; d.depth = (int *)L.depth.p; d.leaf_kind = (int *)L.leaf_kind.p; d.leaf = (u64 *)L.leaf.p;
    d.leaf_last = (int *)L.leaf_last.p; d.logits = (float *)L.logits.p; d.vhid = (float *)L.vhid.p;
    d.leaf_sym = e->leaf_symmetry ? (int *)L.leaf_sym.p : nullptr;
    d.it_status = leaves > 1 ? (int *)L.it_status.p : d.s_status;
    d.it_net = leaves > 1 ? (int *)L.it_net.p : d.s_net;
    return AZ_OK;
}

// Deep engines: device memory that grows with num_simulations has to fit before anything is allocated, so that a search
// too deep for the device is refused with its byte count instead of failing halfway with AZ_ERR_HIP
static int deep_memory_guard(const char *what, size_t need, az_engine *e)
{
    size_t free_b = 0, total_b = 0;
    hipError_t hr = hipMemGetInfo(&free_b, &total_b);
    if (hr != hipSuccess) return fail(e, AZ_ERR_HIP, "hipMemGetInfo failed: %s", hipGetErrorString(hr));
    if (need > free_b)
        return fail(e, AZ_ERR_INVALID, "%s needs %zu bytes of device memory, %zu bytes are free", what, need, free_b);
    return AZ_OK;
}

static int create_engine(const az_config *cfg, az_engine **out, bool deep)
{
    if (!cfg || !out) return fail(nullptr, AZ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->board_size < 3 || cfg->board_size > 15)
        return fail(nullptr, AZ_ERR_INVALID, "board_size must be 3..15 (got %d)", cfg->board_size);
    if (cfg->win_length < 2 || cfg->win_length > cfg->board_size) return fail(nullptr, AZ_ERR_INVALID, "bad win_length");
    if (!deep && (cfg->num_simulations < 1 || cfg->num_simulations > 1024))
        return fail(nullptr, AZ_ERR_INVALID, "num_simulations must be 1..1024 (az_create_deep takes up to %d)", AZ_DEEP_MAX_SIMULATIONS);
    if (deep && (cfg->num_simulations < 1 || cfg->num_simulations > AZ_DEEP_MAX_SIMULATIONS))
        return fail(nullptr, AZ_ERR_INVALID, "num_simulations must be 1..%d", AZ_DEEP_MAX_SIMULATIONS);
    if (cfg->slots < 1 || cfg->slots > 65536) return fail(nullptr, AZ_ERR_INVALID, "slots must be 1..65536");
    if (cfg->model != AZ_MODEL_PLAIN && cfg->model != AZ_MODEL_RESNET) return fail(nullptr, AZ_ERR_INVALID, "unknown model kind %d", cfg->model);
    if (cfg->engines < 0 || cfg->engines > 16) return fail(nullptr, AZ_ERR_INVALID, "engines must be 0 (auto) .. 16");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, AZ_ERR_NO_DEVICE, "no HIP device: this engine has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, AZ_ERR_INVALID, "device %d out of range (%d devices)", cfg->device, ndev);
    az_engine *e = new az_engine();
    e->cfg = *cfg;
    e->deep = deep;
    e->n = cfg->board_size;
    e->nn = e->n * e->n;
    e->RW = (e->nn + 63) / 64 * 64;
    e->R = cfg->num_simulations + 1;
    e->PATH = e->nn + 1;
    e->ops = az_size_ops(e->n);
    if (!e->ops) {
        delete e;
        return fail(nullptr, AZ_ERR_INVALID, "board size %d is not built into this library", cfg->board_size);
    }
    if (deep) {
        // what grows with S: every slot's tree, (S + 1) rows of RW edges, and the log / sqrt tables
        const size_t need = (size_t)cfg->slots * (size_t)e->R * (size_t)e->RW * sizeof(Edge) +
                            (size_t)(cfg->num_simulations + 3) * (sizeof(float) + sizeof(double));
        DeviceGuard g(cfg->device);
        int rc = g.rc != hipSuccess ? fail(nullptr, AZ_ERR_HIP, "hipSetDevice(%d) failed", cfg->device)
                                    : deep_memory_guard("the trees of this deep engine", need, nullptr);
        if (rc) {
            delete e;
            return rc;
        }
    }
    int K = cfg->engines > 0 ? cfg->engines : auto_lanes(e->n, cfg->slots);
    if (K > cfg->slots) K = cfg->slots;
    const int per = (cfg->slots + K - 1) / K;
    K = (cfg->slots + per - 1) / per;              // no empty lane
    e->cfg.engines = K;
    e->lanes.resize(K);
    DeviceGuard guard(cfg->device);          // the caller's current device is restored on return
    hipError_t hr = guard.rc;
    // Own hardware queue per lane: the runtime multiplexes the streams of one priority level over a small pool of
    // hardware queues, so next to a framework that has already created streams (PyTorch's context) two lanes can
    // land on one queue and stop overlapping (measured: episode 11.6 -> 15.3 s).  High-priority streams draw from
    // their own pool.  AZ_STREAM_PRIORITY=0 keeps the default priority.
    for (int i = 0; i < K && hr == hipSuccess; i++) {
        e->lanes[i].index = i;
        hr = g_streams.acquire(cfg->device, true, &e->lanes[i].stream);
    }
    if (hr != hipSuccess) {
        int rc = fail(nullptr, AZ_ERR_HIP, "device init failed: %s", hipGetErrorString(hr));
        az_destroy(e);
        return rc;
    }
    e->stream = e->lanes[0].stream;
    {
        const char *sm = getenv("AZ_SPLIT_MAX");      // 0 disables the split trunk, a large value forces it
        if (sm) e->split_max = atoi(sm);
    }
    int rc = AZ_OK;
    for (int i = 0; i < K && !rc; i++) {
        Lane &L = e->lanes[i];
        const size_t B = (size_t)std::min(per, cfg->slots - i * per);
        ALLOC(L.board, B * 8 * sizeof(u64));
        ALLOC(L.s_game, B * 4); ALLOC(L.s_ply, B * 4); ALLOC(L.s_player, B * 4); ALLOC(L.s_last, B * 4);
        ALLOC(L.s_status, B * 4); ALLOC(L.s_net, B * 4);
        ALLOC(L.edges, B * (size_t)e->R * e->RW * sizeof(Edge));
        ALLOC(L.rows_used, B * 4);
        ALLOC(L.cnt, B * CNT_STRIDE * sizeof(unsigned long long)); ALLOC(L.active_dev, 16);
        ALLOC(L.carried, B * 4);
        ALLOC(L.budget, B * 4); ALLOC(L.cp_board, B * 8 * sizeof(u64)); ALLOC(L.cp_state, B * 4 * 4);
        DevState &d = L.d;
        d.B = (int)B; d.R = e->R; d.S = cfg->num_simulations; d.k = cfg->win_length; d.rule = WIN_RULE_FREESTYLE;
        d.c_puct = cfg->c_puct; d.w_noise = cfg->dirichlet_weight;
        d.one_minus_w = (float)(1.0 - cfg->dirichlet_weight);   // Python float (1 - w) as a weak scalar -> float32 (Q8)
        d.board = (u64 *)L.board.p;
        d.s_game = (int *)L.s_game.p; d.s_ply = (int *)L.s_ply.p; d.s_player = (int *)L.s_player.p;
        d.s_last = (int *)L.s_last.p; d.s_status = (int *)L.s_status.p; d.s_net = (int *)L.s_net.p;
        d.edges = (Edge *)L.edges.p; d.rows_used = (int *)L.rows_used.p;
        d.cnt = (unsigned long long *)L.cnt.p; d.active = (int *)L.active_dev.p;
        d.carried = (int *)L.carried.p; d.reuse = 0;
        d.v2w[0] = d.v2w[1] = d.v2b[0] = d.v2b[1] = nullptr;
        d.cache = nullptr; d.cache_mask = 0; d.cache_gen = e->cache_gen; d.ext_eval = 0; d.leaf_sym = nullptr; d.game_key0 = 0;
        d.key_stride = 1; d.T_game = nullptr;
        d.start_pos = nullptr; d.start_count = 0; d.start_first = 0;
        d.resign_thr = 0.0; d.resign_min_ply = 0; d.resign_permille = 0; d.rec_value = nullptr; d.g_cross = nullptr;
        d.cap_fast = 0; d.cap_permille = 0;
        d.forced_k = 0.0; d.forced_prune = 0;
        d.gumbel_m = 0; d.gumbel_cv = 0.0; d.gumbel_cs = 0.0; d.gumbel_seq = nullptr; d.root_logits = nullptr; d.root_v = nullptr;
        d.proof = nullptr; d.proof_buf = nullptr; d.root_proof = nullptr; d.rec_proof = nullptr; d.proof_stops = nullptr;
        d.sel_cpuct = nullptr; d.sel_mass = nullptr; d.sel_fpu = 0.0; d.sel_fpu_root = 0.0;
        d.cand_radius = 0;
        d.s_budget = (int *)L.budget.p; d.cp_board = (u64 *)L.cp_board.p; d.cp_state = (int *)L.cp_state.p;
        if (!rc) rc = alloc_items(e, L, 1);
    }
    if (!rc) rc = dev_alloc(e, e->next_game, 16);
    if (!rc) rc = dev_alloc(e, e->T_table, (size_t)(e->nn + 4) * sizeof(double));
    if (!rc) rc = setup_tables(e);
    if (rc) {
        g_create_error = e->err;
        az_destroy(e);
        return rc;
    }
    each_state(e, [&](DevState &d) {
        d.T_table = (const double *)e->T_table.p; d.log_table = (const float *)e->log_table.p;
        d.sqrt_table = (const double *)e->sqrt_table.p; d.noise_off = (const int *)e->noise_off.p;
        d.next_game = (int *)e->next_game.p;
    });
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) e->num_cus = prop.multiProcessorCount;
    }
    const char *pe = getenv("AZ_PROFILE_EVENTS");
    e->profile = pe && pe[0] == '1';
    const char *pz = getenv("AZ_PERSIST");
    e->persist_allowed = !(pz && pz[0] == '0');
    // AZ_DELTA=0: engines start with delta evaluation switched off; AZ_DELTA_TILES=t: with the threshold t (measurements
    // through programs that do not call az_set_delta_eval / az_delta_max_tiles)
    const char *dz = getenv("AZ_DELTA");
    e->delta_on = !(dz && dz[0] == '0');
    const char *dt = getenv("AZ_DELTA_TILES");
    if (dt && atoi(dt) >= 1 && atoi(dt) <= 15) e->delta_tiles = atoi(dt);
    const char *cz = getenv("AZ_COMPACT");
    e->compact = !(cz && cz[0] == '0');
    const char *ge = getenv("AZ_GRAPH");
    e->use_graph = !(ge && ge[0] == '0');
    const char *ts = getenv("AZ_TAPE_STREAM");
    e->stream_tapes = !(ts && ts[0] == '0');
    {
        // Tape producer threads.  What this process may use is its affinity mask and cgroup CPU quota, not the machine's
        // hardware threads (a GPU box grants a job a share of its cores); the ranks of a node split that between them
        // unless the launcher already pinned each rank to its own cores (then the mask is per rank and the split would
        // count twice -- AZ_HOST_CPUS_PER_RANK=1 says so).  K lane threads drive the play streams; the rest, up to 32,
        // produce tapes.
        e->host_cpus = usable_cpus();
        const char *lw = getenv("LOCAL_WORLD_SIZE");
        const char *pr = getenv("AZ_HOST_CPUS_PER_RANK");
        const int ranks = (pr && pr[0] == '1') ? 1 : (lw && atoi(lw) > 0 ? atoi(lw) : 1);
        int t = e->host_cpus / ranks - K;
        const char *tt = getenv("AZ_TAPE_THREADS");
        if (tt) t = atoi(tt);
        e->tape_threads = t < 1 ? 1 : (t > 32 ? 32 : t);
    }
    if (hipStreamSynchronize(e->stream) != hipSuccess) {
        g_create_error = "stream sync failed in az_create";
        az_destroy(e);
        return AZ_ERR_HIP;
    }
    *out = e;
    return AZ_OK;
}

extern "C" int az_create(const az_config *cfg, az_engine **out) { return create_engine(cfg, out, false); }
extern "C" int az_create_deep(const az_config *cfg, az_engine **out) { return create_engine(cfg, out, true); }

static void dist_destroy(az_engine *e);

extern "C" void az_destroy(az_engine *e)
{
    if (!e) return;
    DeviceGuard guard(e->cfg.device);
    stop_tapes(e);
    for (Lane &L : e->lanes)
        if (L.stream) (void)hipStreamSynchronize(L.stream);
    dist_destroy(e);
    for (Lane &L : e->lanes) {
        DevBuf *all[] = {&L.board, &L.s_game, &L.s_ply, &L.s_player, &L.s_last, &L.s_status, &L.s_net, &L.edges, &L.rows_used,
                         &L.path, &L.depth, &L.leaf_kind, &L.leaf, &L.leaf_last, &L.logits, &L.vhid, &L.pol_feat, &L.cnt,
                         &L.active_dev, &L.carried, &L.dbg, &L.scratch, &L.it_status, &L.it_net, &L.leaf_sym, &L.inflight,
                         &L.budget, &L.cp_board, &L.cp_state, &L.root_logits, &L.root_v, &L.proof, &L.root_proof, &L.proof_stops,
                         &L.threat_edges, &L.threat_root, &L.threat_depth, &L.threat_move, &L.threat_nodes, &L.threat_stat,
                         &L.delta_base, &L.delta_done, &L.delta_cnt};
        for (DevBuf *b : all) dev_free(*b);
        for (hipEvent_t ev : L.ev) (void)hipEventDestroy(ev);
        for (int i = 0; i < 4; i++)
            if (L.graph[i >> 1][i & 1].exec) (void)hipGraphExecDestroy(L.graph[i >> 1][i & 1].exec);
    }
    DevBuf *shared[] = {&e->T_table, &e->log_table, &e->sqrt_table, &e->noise_off, &e->next_game, &e->noise, &e->u,
                        &e->rec_planes, &e->rec_last, &e->rec_action, &e->rec_mover, &e->rec_pi, &e->rec_visits, &e->g_nply,
                        &e->g_result, &e->src_index, &e->rec_value, &e->g_cross, &e->cache, &e->start_tab, &e->bt_cells, &e->bt_players, &e->bt_lasts, &e->bt_T,
                        &e->bt_zero_off, &e->bt_visits, &e->bt_W, &e->bt_prior, &e->bt_pi, &e->bt_action, &e->ext.map, &e->ext.count, &e->gumbel_seq, &e->rec_proof, &e->rec_threat,
                        &e->cb_planes, &e->cb_policy, &e->cb_value, &e->sel_cpuct, &e->sel_mass};
    for (DevBuf *b : shared) dev_free(*b);
    for (int s = 0; s < 2; s++) {
        PackedNet &p = e->net[s];
        DevBuf *nb[] = {&p.c1, &p.c2, &p.c3, &p.hd, &p.hdq, &p.pf, &p.vf, &p.c1b, &p.c2b, &p.c3b, &p.hdb, &p.pfb, &p.vfb, &p.v2w, &p.v2b, &p.c1x[0], &p.c1x[1], &p.c2x[0], &p.c2x[1], &p.c3x[0], &p.c3x[1], &p.hdx[0], &p.hdx[1]};
        for (DevBuf *b : nb) dev_free(*b);
        for (int i = 0; i < 6; i++) { dev_free(p.rblk[i]); dev_free(p.rblkb[i]); dev_free(p.rblkx[0][i]); dev_free(p.rblkx[1][i]); }
    }
    for (Lane &L : e->lanes)
        if (L.stream) g_streams.release(e->cfg.device, true, L.stream);
    delete e;
}

// every weight of the layers the emulated trunks run is inside float16's range (the only part of the split that is checked
// eagerly at az_load_weights*; NaN counts as outside)
static bool in_f16_range(const PackedNet &p)
{
    auto ok = [](const std::vector<float> &v) {
        for (float x : v)
            if (!(std::fabs(x) < 65504.0f)) return false;
        return true;
    };
    bool r = ok(p.hw_first) && ok(p.hw_pol) && ok(p.hw_val);
    for (int i = 0; i < 6; i++) r = r && ok(p.hw_conv[i]);
    return r;
}

// packs and uploads the split fragments of weight slot `slot` for `scheme` unless that has been done since the last load
static int ensure_emul(az_engine *e, int slot, int scheme)
{
    PackedNet &p = e->net[slot];
    const int si = scheme - 1;
    if (!p.loaded || scheme == AZ_TRUNK_F32 || p.emul_ready[si]) return AZ_OK;
    bool ok = true;
    int rc = AZ_OK;
    auto upx = [&](DevBuf &b, const std::vector<uint16_t> &x) { if (!rc) rc = upload(e, b, x.data(), x.size() * 2); };
    if (e->cfg.model == AZ_MODEL_PLAIN) {
        upx(p.c1x[si], pack_first_emul(scheme, p.hw_first.data(), 32, &ok));
        upx(p.c2x[si], pack_conv_emul(scheme, p.hw_conv[0].data(), 64, 32, &ok));
        upx(p.c3x[si], pack_conv_emul(scheme, p.hw_conv[1].data(), 128, 64, &ok));
        upx(p.hdx[si], pack_heads_emul(scheme, p.hw_pol.data(), 4, p.hw_val.data(), 2, 128, &ok));
        if (rc) return rc;
        p.w.c1x[si] = p.c1x[si].p; p.w.c2x[si] = p.c2x[si].p; p.w.c3x[si] = p.c3x[si].p; p.w.hdx[si] = p.hdx[si].p;
    } else {
        upx(p.c1x[si], pack_first_emul(scheme, p.hw_first.data(), 64, &ok));
        for (int i = 0; i < 6; i++) upx(p.rblkx[si][i], pack_conv_emul(scheme, p.hw_conv[i].data(), 64, 64, &ok));
        upx(p.hdx[si], pack_heads_emul(scheme, p.hw_pol.data(), 2, p.hw_val.data(), 1, 64, &ok));
        if (rc) return rc;
        for (int i = 0; i < 6; i++) p.rw.blkx[si][i] = p.rblkx[si][i].p;
        p.rw.hdx[si] = p.hdx[si].p;
        p.rw.stemx[si] = p.c1x[si].p;
    }
    p.emul_ready[si] = true;
    return AZ_OK;
}

extern "C" int az_load_weights(az_engine *e, int slot, const float *const *t)
{
    if (!e || !t || slot < 0 || slot > 1) return fail(e, AZ_ERR_INVALID, "az_load_weights: bad argument");
    if (e->cfg.model != AZ_MODEL_PLAIN) return fail(e, AZ_ERR_INVALID, "az_load_weights: engine was created for the ResidualBlock model");
    for (int i = 0; i < 16; i++)
        if (!t[i]) return fail(e, AZ_ERR_INVALID, "az_load_weights: tensor %d is null", i);
    DEVICE_GUARD(e);
    const int nn = e->nn;
    PackedNet &p = e->net[slot];
    int rc = AZ_OK;
    auto up = [&](DevBuf &b, const std::vector<float> &v) { if (!rc) rc = upload(e, b, v.data(), v.size() * sizeof(float)); };
    auto upraw = [&](DevBuf &b, const float *v, size_t cnt) { if (!rc) rc = upload(e, b, v, cnt * sizeof(float)); };
    up(p.c1, pack_conv(t[0], 32, 4));   upraw(p.c1b, t[1], 32);
    up(p.c2, pack_conv(t[2], 64, 32));  upraw(p.c2b, t[3], 64);
    up(p.c3, pack_conv(t[4], 128, 64)); upraw(p.c3b, t[5], 128);
    p.hw_first.assign(t[0], t[0] + 32 * 4 * 9);
    p.hw_conv[0].assign(t[2], t[2] + 64 * 32 * 9);
    p.hw_conv[1].assign(t[4], t[4] + 128 * 64 * 9);
    p.hw_pol.assign(t[6], t[6] + 4 * 128);
    p.hw_val.assign(t[10], t[10] + 2 * 128);
    p.emul_ready[0] = p.emul_ready[1] = false;
    p.f16_ok = in_f16_range(p);
    up(p.hd, pack_heads(t[6], 4, t[10], 2, 128));
    up(p.hdq, pack_heads_blocks(t[6], t[10]));
    float hb[6] = {t[7][0], t[7][1], t[7][2], t[7][3], t[11][0], t[11][1]};
    upraw(p.hdb, hb, 6);
    up(p.pf, pack_fc(t[8], nn, 4 * nn));  upraw(p.pfb, t[9], nn);
    up(p.vf, pack_fc(t[12], 64, 2 * nn)); upraw(p.vfb, t[13], 64);
    upraw(p.v2w, t[14], 64); upraw(p.v2b, t[15], 1);
    if (rc) return rc;
    p.w.c1 = (const float *)p.c1.p; p.w.c2 = (const float *)p.c2.p; p.w.c3 = (const float *)p.c3.p;
    p.w.hd = (const float *)p.hd.p; p.w.hdq = (const float *)p.hdq.p; p.w.pf = (const float *)p.pf.p; p.w.vf = (const float *)p.vf.p;
    p.w.c1b = (const float *)p.c1b.p; p.w.c2b = (const float *)p.c2b.p; p.w.c3b = (const float *)p.c3b.p;
    p.w.hdb = (const float *)p.hdb.p; p.w.pfb = (const float *)p.pfb.p; p.w.vfb = (const float *)p.vfb.p;
    e->cache_gen++;           // evaluations cached under the previous weights never match again
    each_state(e, [&](DevState &d) { d.v2w[slot] = (const float *)p.v2w.p; d.v2b[slot] = (const float *)p.v2b.p; d.cache_gen = e->cache_gen; });
    p.loaded = true;
    if (e->trunk_mode == AZ_TRUNK_F16X2 && !p.f16_ok) {
        e->trunk_mode = AZ_TRUNK_F32;       // never run a net outside float16's range in the float16 scheme
        return fail(e, AZ_ERR_INVALID, "weights outside float16's range (|w| >= 65504): AZ_TRUNK_F16X2 switched off, the engine is back on AZ_TRUNK_F32");
    }
    return e->trunk_mode != AZ_TRUNK_F32 ? ensure_emul(e, slot, e->trunk_mode) : AZ_OK;
}

extern "C" int az_load_weights_resnet(az_engine *e, int slot, const float *const *t)
{
    if (!e || !t || slot < 0 || slot > 1) return fail(e, AZ_ERR_INVALID, "az_load_weights_resnet: bad argument");
    if (e->cfg.model != AZ_MODEL_RESNET) return fail(e, AZ_ERR_INVALID, "az_load_weights_resnet: engine was created for the plain model");
    for (int i = 0; i < 24; i++)
        if (!t[i]) return fail(e, AZ_ERR_INVALID, "az_load_weights_resnet: tensor %d is null", i);
    DEVICE_GUARD(e);
    const int nn = e->nn;
    PackedNet &p = e->net[slot];
    int rc = AZ_OK;
    auto up = [&](DevBuf &b, const std::vector<float> &v) { if (!rc) rc = upload(e, b, v.data(), v.size() * sizeof(float)); };
    auto upraw = [&](DevBuf &b, const float *v, size_t cnt) { if (!rc) rc = upload(e, b, v, cnt * sizeof(float)); };
    up(p.c1, pack_conv(t[0], 64, 4)); upraw(p.c1b, t[1], 64);
    for (int i = 0; i < 6; i++) { up(p.rblk[i], pack_conv(t[2 + 2 * i], 64, 64)); upraw(p.rblkb[i], t[3 + 2 * i], 64); }
    p.hw_first.assign(t[0], t[0] + 64 * 4 * 9);
    for (int i = 0; i < 6; i++) p.hw_conv[i].assign(t[2 + 2 * i], t[2 + 2 * i] + 64 * 64 * 9);
    p.hw_pol.assign(t[14], t[14] + 2 * 64);
    p.hw_val.assign(t[16], t[16] + 64);
    p.emul_ready[0] = p.emul_ready[1] = false;
    p.f16_ok = in_f16_range(p);
    up(p.hd, pack_heads(t[14], 2, t[16], 1, 64));
    float hb[3] = {t[15][0], t[15][1], t[17][0]};
    upraw(p.hdb, hb, 3);
    up(p.pf, pack_fc(t[18], nn, 2 * nn)); upraw(p.pfb, t[19], nn);
    up(p.vf, pack_fc(t[20], 64, nn));     upraw(p.vfb, t[21], 64);
    upraw(p.v2w, t[22], 64); upraw(p.v2b, t[23], 1);
    if (rc) return rc;
    p.rw.stem = (const float *)p.c1.p; p.rw.stemb = (const float *)p.c1b.p;
    for (int i = 0; i < 6; i++) { p.rw.blk[i] = (const float *)p.rblk[i].p; p.rw.blkb[i] = (const float *)p.rblkb[i].p; }
    p.rw.hd = (const float *)p.hd.p; p.rw.hdb = (const float *)p.hdb.p;
    p.w = NetWeights{};
    p.w.pf = (const float *)p.pf.p; p.w.vf = (const float *)p.vf.p;
    p.w.pfb = (const float *)p.pfb.p; p.w.vfb = (const float *)p.vfb.p;
    e->cache_gen++;           // evaluations cached under the previous weights never match again
    each_state(e, [&](DevState &d) { d.v2w[slot] = (const float *)p.v2w.p; d.v2b[slot] = (const float *)p.v2b.p; d.cache_gen = e->cache_gen; });
    p.loaded = true;
    if (e->trunk_mode == AZ_TRUNK_F16X2 && !p.f16_ok) {
        e->trunk_mode = AZ_TRUNK_F32;       // never run a net outside float16's range in the float16 scheme
        return fail(e, AZ_ERR_INVALID, "weights outside float16's range (|w| >= 65504): AZ_TRUNK_F16X2 switched off, the engine is back on AZ_TRUNK_F32");
    }
    return e->trunk_mode != AZ_TRUNK_F32 ? ensure_emul(e, slot, e->trunk_mode) : AZ_OK;
}

// ------------------------------------------------------------------------------------------------
// episode machinery
// ------------------------------------------------------------------------------------------------
static int ensure_episode_buffers(az_engine *e, int games, bool need_noise)
{
    const size_t nn = e->nn, G = (size_t)games;
    int rc = AZ_OK;
    stop_tapes(e);            // a producer of an abandoned episode still writes into the buffers below
    ALLOC(e->rec_planes, G * nn * 8 * sizeof(u64), false);
    ALLOC(e->rec_last, G * nn * 2, false); ALLOC(e->rec_action, G * nn * 2, false); ALLOC(e->rec_mover, G * nn, false);
    ALLOC(e->rec_pi, G * nn * nn * 4, false); ALLOC(e->rec_visits, G * nn * nn * 2, false);
    ALLOC(e->g_nply, G * 4, true); ALLOC(e->g_result, G * 4, true);
    ALLOC(e->rec_value, G * nn * 4, false); ALLOC(e->g_cross, G * 4, false);
    if (e->solver) ALLOC(e->rec_proof, G * nn, false);
    if (e->threat_depth) ALLOC(e->rec_threat, G * nn, false);
    if (!rc) HIPCHECK(e, hipMemsetAsync(e->g_cross.p, 0xFF, G * 4, e->stream));      // -1: no game has crossed
    ALLOC(e->u, G * nn * sizeof(double), false);
    if (need_noise) ALLOC(e->noise, G * (size_t)e->tape_len * sizeof(double), false);
    if (rc) return rc;
    each_state(e, [&](DevState &d) {
        d.rec_planes = (u64 *)e->rec_planes.p; d.rec_last = (short *)e->rec_last.p; d.rec_action = (short *)e->rec_action.p;
        d.rec_mover = (unsigned char *)e->rec_mover.p; d.rec_pi = (float *)e->rec_pi.p;
        d.rec_visits = (unsigned short *)e->rec_visits.p; d.g_nply = (int *)e->g_nply.p; d.g_result = (int *)e->g_result.p;
        d.rec_value = (float *)e->rec_value.p; d.g_cross = (int *)e->g_cross.p;
        d.u = (const double *)e->u.p; d.noise = (const double *)e->noise.p; d.noise_stride = e->tape_len;
    });
    return AZ_OK;
}

struct EpisodeSpec {
    int num_games = 0, max_plies = 0;
    bool add_noise = true, arena = false;
    bool preset = false;      // the first Lane::preset_m slots of every lane already hold positions (preset_search); skip the initial refill
    bool batch = false;       // ... of az_search_batch: the ply runs over the preset slots only, throughput kernel choices as in self-play
    bool profile = true;      // this episode may be timed with HIP events (only when az_set_profiling is on)
    unsigned game_key0 = 0;   // low 32 bits of seed0: the leaf-symmetry hash names game g by its seed, seed0 + g
    int ext_net = -1;         // external evaluator: the net id of the requests (az_search*: the slot argument), -1 = the items' own
};

static int host_threads()
{
    int t = usable_cpus();
    const char *ev = getenv("AZ_HOST_THREADS");
    if (ev) t = atoi(ev);
    return t < 1 ? 1 : (t > 64 ? 64 : t);
}

// errors inside a lane's host thread are kept on the lane and reported by the joining caller
static int lane_fail(Lane &L, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    L.err = buf;
    L.rc = code;
    return code;
}
#define HIPCHECK_L(L, call)                                                                        \
    do {                                                                                           \
        hipError_t _r = (call);                                                                    \
        if (_r != hipSuccess)                                                                      \
            return lane_fail(L, AZ_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

// the threat search's view of a lane's buffers (L = nullptr: the option is off, every pointer null)
static void set_threat_state(DevState &d, const Lane *L, int max_depth, int budget)
{
    d.threat_edges = L ? (unsigned char *)L->threat_edges.p : nullptr;
    d.threat_root = L ? (signed char *)L->threat_root.p : nullptr;
    d.threat_depth = L ? (signed char *)L->threat_depth.p : nullptr;
    d.threat_move = L ? (short *)L->threat_move.p : nullptr;
    d.threat_nodes = L ? (int *)L->threat_nodes.p : nullptr;
    d.threat_stat = L ? (unsigned long long *)L->threat_stat.p : nullptr;
    d.threat_max_depth = L ? max_depth : 0;
    d.threat_budget = L ? budget : 0;
}

static int ensure_threat_buffers(az_engine *e)
{
    return ensure_lane_buffers(e, {{&Lane::threat_edges, (size_t)e->RW, false}, {&Lane::threat_root, 1, false}, {&Lane::threat_depth, 1, false},
                                   {&Lane::threat_move, 2, false}, {&Lane::threat_nodes, 4, false},
                                   {&Lane::threat_stat, THREAT_STATS * sizeof(unsigned long long), false}});
}

// Delta evaluation serves the lock-step path of the plain float32 trunk at the size that has the kernels (n = 15), one net, one
// leaf per game and batch, positions shown to the net as they are; everything else evaluates in full.
static bool delta_eligible(const az_engine *e, bool arena, bool ext, bool capped)
{
    return e->delta_on && e->ops->trunk_delta && e->cfg.eval_kind == AZ_EVAL_NET && e->cfg.model == AZ_MODEL_PLAIN &&
           e->trunk_mode == AZ_TRUNK_F32 && e->vl == 1 && !e->vl_kernel && !e->leaf_symmetry && !e->reuse && !arena && !ext && !capped &&
           e->cfg.num_simulations <= DEFAULT_MAX_S;
}
static int ensure_delta_buffers(az_engine *e)
{
    // every call starts from no base evaluation done and counters at zero; the activations themselves are written before they are read
    return ensure_lane_buffers(e, {{&Lane::delta_base, (size_t)e->ops->delta_floats_per_slot * sizeof(float), false},
                                   {&Lane::delta_done, 1, true}, {&Lane::delta_cnt, DELTA_CNT * sizeof(unsigned long long), true}});
}

static int episode_begin(az_engine *e, const EpisodeSpec &sp)
{
    const bool ext = e->ext.on;            // the evaluator is outside the engine: no weights, no cache, priors as given
    const bool net = !ext && e->cfg.eval_kind == AZ_EVAL_NET;
    if (net && !e->net[0].loaded) return fail(e, AZ_ERR_NO_WEIGHTS, "weights slot 0 not loaded");
    if (net && sp.arena && !e->net[1].loaded) return fail(e, AZ_ERR_NO_WEIGHTS, "weights slot 1 (baseline) not loaded");
    if (ext) {
        const int need = e->cfg.slots * e->vl;       // az_set_virtual_loss may have raised it since the evaluator was set
        if (e->ext.ev.capacity < need) stop_tapes(e);    // az_selfplay_begin has started them already
        if (e->ext.ev.capacity < need)
            return fail(e, AZ_ERR_INVALID, "the external evaluator's buffers hold %d items, %d slots x %d leaves per batch need %d",
                        e->ext.ev.capacity, e->cfg.slots, e->vl, need);
        int rc = dev_alloc(e, e->ext.map, (size_t)need * sizeof(int), false);
        if (!rc) rc = dev_alloc(e, e->ext.count, 16, true);
        if (rc) return rc;
        e->ext.requests = e->ext.items = 0;
    }
    // the root threat search is for every search the solver serves; its buffers were allocated by az_set_threat_search
    for (Lane &L : e->lanes) set_threat_state(L.d, e->threat_depth ? &L : nullptr, e->threat_depth, e->threat_budget);
    each_state(e, [&](DevState &d) {
        d.rec_threat = e->threat_depth ? (signed char *)e->rec_threat.p : nullptr;
        d.max_plies = sp.max_plies; d.add_noise = sp.add_noise ? 1 : 0; d.arena = sp.arena ? 1 : 0;
        d.total_games = sp.num_games; d.reuse = e->reuse; d.game_key0 = sp.game_key0;
        d.cache = ext ? nullptr : (float *)e->cache.p; d.cache_mask = e->cache_mask; d.cache_gen = e->cache_gen;
        d.ext_eval = ext ? 1 : 0;
        d.rule = e->win_rule;      // which game is played: every search, self-play, arena and preset episode alike
        // start positions are for the games k_refill claims: a preset episode (az_search, az_search_batch) brings its own
        const bool sps = !sp.preset && e->start_count > 0;
        d.start_pos = sps ? (const StartPos *)e->start_tab.p : nullptr;
        d.start_count = sps ? e->start_count : 0;
        d.start_first = sps ? e->start_first : 0;
        // resignation is for self-play and the arena: a preset episode searches given positions, it plays no game
        d.resign_thr = sp.preset ? 0.0 : e->resign_thr;
        d.resign_min_ply = sp.preset ? 0 : e->resign_min_ply;
        d.resign_permille = sp.preset || sp.arena ? 0 : e->resign_permille;
        // the playout cap is for self-play games only: the arena and the preset searches run every ply in full
        d.cap_fast = sp.preset || sp.arena ? 0 : e->cap_fast;
        d.cap_permille = d.cap_fast ? e->cap_permille : 0;
        // forced playouts are for the searches whose root is noised (the arena's never is); k_step exempts the cap's FAST plies
        d.forced_k = sp.add_noise && !sp.arena ? e->forced_k : 0.0;
        d.forced_prune = d.forced_k > 0.0 ? e->forced_prune : 0;
        // ... and so is the Gumbel root search; the buffers it reads were set by az_set_gumbel
        d.gumbel_m = sp.add_noise && !sp.arena ? e->gumbel_m : 0;
        d.gumbel_cv = d.gumbel_m ? e->gumbel_cv : 0.0;
        d.gumbel_cs = d.gumbel_m ? e->gumbel_cs : 0.0;
        // the solver is for every search; the slot's status arrays were put into the state by az_set_solver
        d.proof = e->solver ? d.proof_buf : nullptr;
        d.rec_proof = e->solver ? (signed char *)e->rec_proof.p : nullptr;
        // the selection rule is for every search as well; its tables and root_v were put up by az_set_selection
        d.sel_cpuct = e->sel_on ? (const double *)e->sel_cpuct.p : nullptr;
        d.sel_mass = e->sel_on ? (const double *)e->sel_mass.p : nullptr;
        d.sel_fpu = e->sel_on ? e->sel_fpu : 0.0;
        d.sel_fpu_root = e->sel_on ? e->sel_fpu_root : 0.0;
        // ... and so are candidate moves: self-play, the arena and the preset searches alike
        d.cand_radius = e->cand_radius;
    });
    e->episode_solver = e->solver;
    e->solver_stops = 0;
    e->episode_threat = e->threat_depth;
    for (int64_t &x : e->threat_stats) x = 0;
    if (!sp.preset) { e->proof_edges.clear(); e->proof_roots.clear(); }     // az_last_proof speaks of the last preset search only
    const bool capped = !sp.preset && !sp.arena && e->cap_fast > 0;
    // persistent search kernel: plain net or synthetic evaluator, the reference's sequential search, trees that fit into LDS
    e->persist_gp = 0;
    if (e->persist_allowed && !ext && !e->vl_kernel && !capped && !e->threat_depth && !e->sel_on && !e->cand_radius && e->trunk_mode == AZ_TRUNK_F32) {
        const int synth = e->cfg.eval_kind == AZ_EVAL_SYNTHETIC ? 1 : 0;
        const int S = e->cfg.num_simulations;
        if (!sp.arena && (!sp.preset || sp.batch) && e->ops->search_prepare(S, 2, synth, e->cfg.model, e->solver)) e->persist_gp = 2;
        else if (e->ops->search_prepare(S, 1, synth, e->cfg.model, e->solver)) e->persist_gp = 1;     // arena: a workgroup's games must share one net
    }
    az_engine::Run &r = e->run;
    r = az_engine::Run();
    r.num_games = sp.num_games; r.max_plies = sp.max_plies; r.add_noise = sp.add_noise; r.arena = sp.arena;
    r.preset = sp.preset; r.profile = sp.profile;
    r.ext = ext; r.ext_net = sp.ext_net;
    r.game_key0 = sp.game_key0;
    if (capped) { r.cap_fast = e->cap_fast; r.cap_permille = e->cap_permille; r.cap_export_full = e->cap_export_full; }
    for (int64_t &x : e->delta_stats) x = 0;
    if (!e->persist_gp && delta_eligible(e, sp.arena, ext, capped)) {
        int rcd = ensure_delta_buffers(e);
        if (rcd) return rcd;
        r.delta = true;
    }
    if (!sp.preset && e->start_count > 0) {
        r.start.resize(sp.num_games);
        for (int g = 0; g < sp.num_games; g++) {
            const unsigned f = (unsigned)e->start_first + (unsigned)g;
            r.start[g] = e->start_ply[(sp.arena ? f >> 1 : f) % (unsigned)e->start_count];
        }
    }
    HIPCHECK(e, hipMemsetAsync(e->next_game.p, 0, 16, e->stream));
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    // the first refill hands every lane an equal share of the games (as many as its slots hold); afterwards a freed
    // slot of ANY lane takes the next id of the shared queue, so no lane idles while another still has games waiting
    const int K = (int)e->lanes.size();
    const int share = (sp.num_games + K - 1) / K;
    for (Lane &L : e->lanes) {
        L.active = 0; L.n_full = 0; L.refill_out[0] = L.refill_out[1] = 0; L.cur = L.d.B; L.plies_played = 0; L.steps = L.trunk_launches = L.plies = 0;
        L.trunk_ms = L.nn_ms = L.step_ms = 0.0; L.tape_wait_s = 0.0; L.rc = AZ_OK; L.err.clear();
        HIPCHECK(e, hipMemsetAsync(L.cnt.p, 0, L.cnt.bytes, L.stream));
        if (e->solver) HIPCHECK(e, hipMemsetAsync(L.proof_stops.p, 0, L.proof_stops.bytes, L.stream));
        if (e->threat_depth) HIPCHECK(e, hipMemsetAsync(L.threat_stat.p, 0, L.threat_stat.bytes, L.stream));
        HIPCHECK(e, hipMemsetAsync(L.carried.p, 0xFF, L.carried.bytes, L.stream));      // -1: every slot starts from a fresh root
        if (!sp.preset) {
            HIPCHECK(e, hipMemsetAsync(L.s_status.p, 0, L.s_status.bytes, L.stream));
            hipLaunchKernelGGL(k_refill, dim3(1), dim3(1024), 0, L.stream, L.d, share, e->compact ? 1 : 0);
            HIPCHECK(e, hipMemcpyAsync(L.refill_out, L.active_dev.p, 8, hipMemcpyDeviceToHost, L.stream));
        } else {
            if (L.preset_m == 0) HIPCHECK(e, hipMemsetAsync(L.s_status.p, 0, L.s_status.bytes, L.stream));
            L.active = L.preset_m;
            if (sp.batch && L.preset_m > 0) L.cur = L.preset_m;
        }
        HIPCHECK(e, hipStreamSynchronize(L.stream));
        if (!sp.preset) { L.active = L.refill_out[0]; L.n_full = L.refill_out[1]; }
        if (!sp.preset && e->compact && !e->reuse) L.cur = L.active;       // the active slots are the first L.active ones
    }
    r.open = true;
    e->have_episode = false;
    return AZ_OK;
}

// Evaluation batches of one ply: the root's evaluation, then the simulations -- one per batch in the reference's
// sequential loop (mcts.py:123-141), `vl` per batch with virtual-loss batching.
static int sims_batches(const az_engine *e, int sims) { return 1 + (e->vl_kernel ? (sims + e->vl - 1) / e->vl : sims); }
static int ply_batches(const az_engine *e) { return sims_batches(e, e->cfg.num_simulations); }

// The two phases of a ply under the playout cap (az_set_playout_cap).  Phase A, the batches a FAST search needs, runs over
// every slot of the ply; phase B, the remaining batches of a FULL search, over the first slots_b ones only: the FULL slots
// after a compacting refill, every slot without compaction (the budgets keep the FAST ones idle), none when no ply is FULL.
struct CapPly {
    int nb_a = 0, slots_b = 0;
    bool split_b = false;          // the trunk choice of phase B, made for its own slot count
};
static int cap_batches(const az_engine *e, const CapPly *cap) { return !cap ? ply_batches(e) : (cap->slots_b > 0 ? ply_batches(e) : cap->nb_a); }

// the tree kernel that consumes evaluation batch `idx` (0 = the root evaluation) and selects the leaves of batch idx + 1
static void launch_step(const az_engine *e, const LaunchCtx &lc, int idx)
{
    const int S = lc.d.S;
    if (e->vl_kernel) {
        const int done = std::min(idx * e->vl, S);             // simulations finished once batch idx is consumed
        e->ops->step_vl(lc, done, std::min(S - done, e->vl));
    } else {
        e->ops->step(lc, idx, idx < S ? 1 : 0);                // root N = idx for the next selection
    }
}

// the kernel sequence of one ply.  ev (eager profiling runs only): four events per evaluation batch, recorded in front of the
// trunk, between trunk and FC, between FC and tree step and after the tree step; the persistent search kernel is timed as
// a whole by the first four (it contains the trunk, the FC layers and the tree steps of every batch).  A failed event record
// returns its error at once, with the rest of the ply not enqueued.
static hipError_t launch_ply(az_engine *e, const LaunchCtx &lc, bool use_split, int nnets, bool net, const hipEvent_t *ev = nullptr,
                             const CapPly *cap = nullptr)
{
    const DevState &d = lc.d;
    hipError_t rc = hipSuccess;
    auto record = [&](int i) { if (ev) rc = hipEventRecord(ev[i], lc.stream); return rc == hipSuccess; };
    hipLaunchKernelGGL(k_begin, dim3((d.B + 255) / 256), dim3(256), 0, lc.stream, d);
    if (d.threat_edges) e->ops->threat(lc);     // the root threat search premarks the root statuses before the root expansion
    if (e->persist_gp) {               // small boards: the whole search of the ply in one persistent kernel (az_search.h)
        if (!record(0)) return rc;
        e->ops->search(lc, e->persist_gp);
        if (!record(1) || !record(2) || !record(3)) return rc;
        e->ops->move(lc);
        return rc;
    }
    if (net && d.cache) e->ops->root_cache(lc);
    // delta evaluation: the two base evaluations of every active slot, then every batch as deltas from them (also where the
    // tile-split trunk would run: a delta workgroup is shorter than a split stage)
    const bool delta = net && lc.delta_base && nnets == 1 && !cap;
    if (delta) e->ops->trunk_base(lc, 0);
    const int nb = cap_batches(e, cap), nb_a = cap ? cap->nb_a : nb;
    LaunchCtx lcb = lc;                // phase B of a capped ply: the same kernels over fewer slots
    if (cap) { lcb.d.B = cap->slots_b; lcb.dv.B = cap->slots_b * d.L; }
    for (int idx = 0; idx < nb; idx++) {
        const LaunchCtx &c = idx < nb_a ? lc : lcb;
        const bool split = idx < nb_a ? use_split : cap->split_b;
        if (net) {
            if (!record(4 * idx)) return rc;
            for (int id = 0; id < nnets; id++) { if (delta) e->ops->trunk_delta(c, id); else if (split) e->ops->trunk_split(c, id); else e->ops->trunk(c, id); }
            if (!record(4 * idx + 1)) return rc;
            for (int id = 0; id < nnets; id++) e->ops->fc(c, id);
            if (!record(4 * idx + 2)) return rc;
        }
        launch_step(e, c, idx);
        if (!record(4 * idx + 3)) return rc;
    }
    e->ops->move(lc);
    return rc;
}

static std::mutex g_capture_mutex;     // lanes of one process capture one at a time (instantiate is not cheap, and rare)

// returns the instantiated graph of one ply for these kernel arguments, capturing it on first use
static int ply_graph(az_engine *e, Lane &L, const LaunchCtx &lc, bool use_split, int nnets, bool net, hipGraphExec_t *out)
{
    Lane::PlyGraph &g = L.graph[use_split ? 1 : 0][nnets - 1];
    if (g.exec && memcmp(&g.key, &lc, sizeof(LaunchCtx)) == 0) { *out = g.exec; return AZ_OK; }
    std::lock_guard<std::mutex> lock(g_capture_mutex);
    if (g.exec) { HIPCHECK_L(L, hipGraphExecDestroy(g.exec)); g.exec = nullptr; }
    hipGraph_t graph = nullptr;
    HIPCHECK_L(L, hipStreamBeginCapture(lc.stream, hipStreamCaptureModeThreadLocal));
    (void)launch_ply(e, lc, use_split, nnets, net);     // no events: nothing in it can fail
    HIPCHECK_L(L, hipStreamEndCapture(lc.stream, &graph));
    hipError_t rc = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (rc != hipSuccess) { g.exec = nullptr; return lane_fail(L, AZ_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(rc)); }
    memcpy(&g.key, &lc, sizeof(LaunchCtx));
    *out = g.exec;
    return AZ_OK;
}

// few pending boards: the latency path, the tile-split trunk (the emulated trunk has one kernel, so that its results never
// depend on the slot count)
static bool use_split(const az_engine *e, const Lane &L, int pending_boards)
{
    return e->split_max > 0 && L.scratch.p && pending_boards <= e->split_max && e->trunk_mode == AZ_TRUNK_F32;
}

// The tapes of the ply a lane is about to play on stream s must be on the device (streamed a wave ahead of the games).  A wave
// whose upload is still in flight would stall the play stream by the same amount: it is waited for here so that the stall
// is counted (az_counters.tape_wait_seconds); normally the wave landed a ply or two ago.
static hipError_t await_tapes(az_engine *e, Lane &L, hipStream_t s)
{
    if (!e->tapes) return hipSuccess;
    hipEvent_t ev = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t rc = e->tapes->need(L.plies_played + e->tapes->ahead, &ev);
    if (rc == hipSuccess && ev && hipEventQuery(ev) != hipSuccess) rc = hipEventSynchronize(ev);
    L.tape_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc == hipSuccess && ev) rc = hipStreamWaitEvent(s, ev, 0);
    return rc;
}

// one lane plays up to max_steps plies of its active slots in lock step (one "step" = MCTS.run for each active game);
// runs on the lane's own host thread
static int lane_plies(az_engine *e, Lane &L, int max_steps)
{
    const az_engine::Run &r = e->run;
    const int S = L.d.S;
    const bool net = e->cfg.eval_kind == AZ_EVAL_NET;
    const bool prof = net && r.profile && e->profile;
    const int nbat = ply_batches(e);
    const size_t need_ev = prof ? (size_t)4 * nbat : 0;
    while (L.ev.size() < need_ev) {
        hipEvent_t ev;
        HIPCHECK_L(L, hipEventCreate(&ev));
        L.ev.push_back(ev);
    }
    const int nnets = r.arena ? 2 : 1;
    const LaunchCtx lc_full = ctx_of_impl(e, L);
    for (int step = 0; step < max_steps && L.active > 0; step++) {
        // this ply runs over the first L.cur slots: all of them, or -- after a compacting refill -- exactly the active ones
        LaunchCtx lc = lc_full;
        lc.d.B = L.cur;
        lc.dv.B = L.cur * L.d.L;
        const DevState &d = lc.d;
        const bool full = L.cur == L.d.B;          // the captured graph holds the full grid; a shrunken ply is launched kernel by kernel
        const bool split = use_split(e, L, L.active * e->vl);
        const hipError_t trc = await_tapes(e, L, L.stream);
        if (trc != hipSuccess) return lane_fail(L, AZ_ERR_HIP, "tape producer: %s", hipGetErrorString(trc));
        // a deep search (S > DEFAULT_MAX_S) is launched kernel by kernel instead of as one graph of ~3 (S + 1) nodes per ply
        // (measured, DESIGN 7b: 5x5 / 1024 slots / S = 1000 runs as fast eagerly as from the graph; a 15x15 search costs 2.5 %)
        // a capped ply (az_set_playout_cap) is launched kernel by kernel as well: the width of its second phase changes from
        // ply to ply, and a graph would have to be captured for every width (DESIGN 7g has the cost of the eager launch)
        CapPly cap;
        if (r.cap_fast) {
            cap.nb_a = sims_batches(e, r.cap_fast);
            cap.slots_b = L.n_full == 0 ? 0 : (e->compact ? L.n_full : L.cur);
            cap.split_b = use_split(e, L, L.n_full * e->vl);
        }
        const int nrun = cap_batches(e, r.cap_fast ? &cap : nullptr);      // evaluation batches this ply launches
        if (e->use_graph && !prof && full && S <= DEFAULT_MAX_S && !r.cap_fast) {
            hipGraphExec_t exec = nullptr;
            int rcg = ply_graph(e, L, lc, split, nnets, net, &exec);
            if (rcg) return rcg;
            HIPCHECK_L(L, hipGraphLaunch(exec, L.stream));
        } else {
            HIPCHECK_L(L, launch_ply(e, lc, split, nnets, net, prof ? L.ev.data() : nullptr, r.cap_fast ? &cap : nullptr));
        }
        if (net) L.trunk_launches += e->persist_gp ? 1 : (int64_t)nnets * nrun;
        L.steps += nrun;
        L.plies += L.active;
        if (r.preset) {
            L.active = 0;
        } else {
            hipLaunchKernelGGL(k_refill, dim3(1), dim3(1024), 0, L.stream, d, 1 << 30, e->compact ? 1 : 0);
            HIPCHECK_L(L, hipMemcpyAsync(L.refill_out, L.active_dev.p, 8, hipMemcpyDeviceToHost, L.stream));
        }
        if (e->tapes)         // finished games need no further tape (g_nply only ever goes from 0 to the game's length, so
                              // a snapshot that lands late can only cost the producer some extra work)
            HIPCHECK_L(L, hipMemcpyAsync(e->tapes->h_done, e->g_nply.p, (size_t)r.num_games * 4, hipMemcpyDeviceToHost, L.stream));
        HIPCHECK_L(L, hipStreamSynchronize(L.stream));
        HIPCHECK_L(L, hipGetLastError());
        if (!r.preset) { L.active = L.refill_out[0]; L.n_full = L.refill_out[1]; }
        if (!r.preset && e->compact && !e->reuse && L.active > 0) L.cur = L.active;
        L.plies_played++;
        if (prof) {
            for (int i = 0; i < (e->persist_gp ? 1 : nrun); i++) {
                float a = 0.f, b = 0.f, c = 0.f;
                HIPCHECK_L(L, hipEventElapsedTime(&a, L.ev[4 * i], L.ev[4 * i + 1]));
                HIPCHECK_L(L, hipEventElapsedTime(&b, L.ev[4 * i + 1], L.ev[4 * i + 2]));
                HIPCHECK_L(L, hipEventElapsedTime(&c, L.ev[4 * i + 2], L.ev[4 * i + 3]));
                L.trunk_ms += a;
                L.nn_ms += a + b;
                L.step_ms += c;
            }
        }
    }
    return AZ_OK;
}


// ------------------------------------------------------------------------------------------------
// external evaluator (az_set_external_evaluator): the plies of an episode whose evaluations leave the engine
// ------------------------------------------------------------------------------------------------
// Whatever an external episode put into the lanes' states goes back on EVERY way out of it (episode end, a failed call, an
// evaluator that gave up): with ext_eval left set, a later native episode would feed raw logits to the tree step as priors.
static int active_slots(const az_engine *e);
static void ext_restore(az_engine *e)
{
    each_state(e, [&](DevState &d) { d.ext_eval = 0; d.cache = (float *)e->cache.p; });
}

// an episode that failed is closed too: the engine stays usable
static void abandon_episode(az_engine *e)
{
    e->run.open = false;
    stop_tapes(e);
    ext_restore(e);
}

// The first K lanes as a finished episode leaves them, for the code that fills slots by hand: every slot and evaluation item
// idle, no pending leaf, the boards empty, no preset positions.  Enqueued on the engine's stream; IdleLanes also waits for it.
static void idle_lanes(az_engine *e, int K)
{
    for (int l = 0; l < K; l++) {
        Lane &L = e->lanes[l];
        (void)hipMemsetAsync(L.s_status.p, 0, L.s_status.bytes, e->stream);
        (void)hipMemsetAsync(L.leaf_kind.p, 0, L.leaf_kind.bytes, e->stream);
        if (L.it_status.p) (void)hipMemsetAsync(L.it_status.p, 0, L.it_status.bytes, e->stream);
        (void)hipMemsetAsync(L.board.p, 0, L.board.bytes, e->stream);
        L.active = L.preset_m = 0;
    }
}
struct IdleLanes {         // ... on every way out of the scope
    az_engine *e;
    int K;
    ~IdleLanes()
    {
        idle_lanes(e, K);
        (void)hipStreamSynchronize(e->stream);
    }
};

// the evaluator gave up (or a HIP call failed) in the middle of a ply: the episode is closed and every slot left idle
static void ext_abort(az_engine *e)
{
    (void)hipStreamSynchronize(e->stream);
    idle_lanes(e, (int)e->lanes.size());
    (void)hipStreamSynchronize(e->stream);
    e->have_episode = false;
    abandon_episode(e);
}

// All lanes play up to max_steps plies TOGETHER from the calling thread, kernel by kernel on the engine's stream: every
// evaluation step gathers the pending items of all lanes into one request per net, hands it to the caller's evaluator and
// scatters its answers before the lanes' tree steps run.  No lane threads (the evaluator is only ever called on the caller's
// thread), no captured graph (the host is in the loop at every step), no persistent search kernel.
static int ext_plies(az_engine *e, int max_steps)
{
    az_engine::Run &r = e->run;
    const az_ext_evaluator &ev = e->ext.ev;
    const int nnets = r.arena ? 2 : 1, nb = ply_batches(e);
    hipStream_t s = e->stream;
    struct Play { Lane *L; LaunchCtx lc; int item_base; };
    int rc = AZ_OK;
#define EXTCHECK(call)                                                                             \
    do {                                                                                           \
        hipError_t _r = (call);                                                                    \
        if (_r != hipSuccess) {                                                                    \
            rc = fail(e, AZ_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_r), __FILE__, __LINE__); \
            ext_abort(e);                                                                          \
            return rc;                                                                             \
        }                                                                                          \
    } while (0)
    for (int step = 0; step < max_steps && active_slots(e) > 0; step++) {
        std::vector<Play> play;
        int item_base = 0;
        for (Lane &L : e->lanes) {
            if (L.active > 0) {
                Play p{&L, ctx_of_impl(e, L), item_base};
                p.lc.stream = s;
                p.lc.synthetic = 0;                    // the tree step consumes rows, whatever az_config.eval_kind says
                p.lc.d.B = L.cur;                      // the first L.cur slots: all of them, or after a compacting refill the active ones
                p.lc.dv.B = L.cur * L.d.L;
                play.push_back(p);
            }
            item_base += L.d.B * L.d.L;
        }
        for (Play &p : play) {
            Lane &L = *p.L;
            EXTCHECK(await_tapes(e, L, s));
            hipLaunchKernelGGL(k_begin, dim3((p.lc.d.B + 255) / 256), dim3(256), 0, s, p.lc.d);
        }
        for (int idx = 0; idx < nb; idx++) {
            for (int net = 0; net < nnets; net++) {
                int first = 1, count = 0;
                for (Play &p : play) {
                    e->ops->ext_gather(p.lc, net, p.item_base, first, ev.capacity, ev.planes_dev, (int *)e->ext.map.p, (int *)e->ext.count.p);
                    first = 0;
                }
                EXTCHECK(hipMemcpyAsync(&count, e->ext.count.p, 4, hipMemcpyDeviceToHost, s));
                EXTCHECK(hipStreamSynchronize(s));
                EXTCHECK(hipGetLastError());
                if (count <= 0) continue;             // nothing waits for this net: no call
                e->ext.requests += 1;
                e->ext.items += count;
                const int cb = ev.fn(ev.user, r.ext_net >= 0 ? r.ext_net : net, count);
                if (cb) {
                    rc = fail(e, AZ_ERR_INVALID, "the evaluator returned %d", cb);
                    ext_abort(e);
                    return rc;
                }
                for (Play &p : play) e->ops->ext_scatter(p.lc, p.item_base, count, (const int *)e->ext.map.p, ev.policy_dev, ev.value_dev);
            }
            for (Play &p : play) launch_step(e, p.lc, idx);
        }
        for (Play &p : play) {
            Lane &L = *p.L;
            e->ops->move(p.lc);
            L.steps += nb;
            L.plies += L.active;
            if (r.preset) {
                L.active = 0;
            } else {
                hipLaunchKernelGGL(k_refill, dim3(1), dim3(1024), 0, s, p.lc.d, 1 << 30, e->compact ? 1 : 0);
                EXTCHECK(hipMemcpyAsync(&L.active, L.active_dev.p, 4, hipMemcpyDeviceToHost, s));
                EXTCHECK(hipStreamSynchronize(s));     // k_refill writes the lane's own counter cell, read back before the next lane's
            }
        }
        if (e->tapes) EXTCHECK(hipMemcpyAsync(e->tapes->h_done, e->g_nply.p, (size_t)r.num_games * 4, hipMemcpyDeviceToHost, s));
        EXTCHECK(hipStreamSynchronize(s));
        EXTCHECK(hipGetLastError());
        for (Play &p : play) {
            Lane &L = *p.L;
            if (!r.preset && e->compact && !e->reuse && L.active > 0) L.cur = L.active;
            L.plies_played++;
        }
    }
#undef EXTCHECK
    return AZ_OK;
}

// every lane plays up to max_steps plies, each on its own host thread (the caller's thread drives lane 0).  With
// profiling on the lanes play one after another instead, so that the HIP events time each kernel alone on the GPU.
static int episode_plies(az_engine *e, int max_steps)
{
    az_engine::Run &r = e->run;
    if (!r.open) return fail(e, AZ_ERR_STATE, "no episode is open");
    const int K = (int)e->lanes.size();
    const bool sequential = K == 1 || (e->profile && r.profile);
    auto t0 = std::chrono::steady_clock::now();
    if (max_steps == 0) {
        // nothing to play (callers read the counters this way): no threads
    } else if (r.ext) {
        const int rc = ext_plies(e, max_steps);
        r.c.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    } else if (sequential) {
        for (Lane &L : e->lanes)
            if (lane_plies(e, L, max_steps)) break;
    } else {
        // nothing may unwind through the C ABI: a thread that cannot be created (std::system_error at a thread limit,
        // bad_alloc) leaves its lane to the calling thread, which then plays it after its own
        std::vector<std::thread> th;
        std::vector<int> inline_lanes;
        const int dev = e->cfg.device;
        for (int i = 1; i < K; i++) {
            try {
                th.emplace_back([e, i, max_steps, dev]() {
                    Lane &L = e->lanes[i];
                    if (hipSetDevice(dev) != hipSuccess) { lane_fail(L, AZ_ERR_HIP, "hipSetDevice(%d) failed on a lane thread", dev); return; }
                    lane_plies(e, L, max_steps);
                });
            } catch (...) {
                inline_lanes.push_back(i);
            }
        }
        lane_plies(e, e->lanes[0], max_steps);
        for (int i : inline_lanes) lane_plies(e, e->lanes[i], max_steps);
        for (auto &t : th) t.join();
    }
    auto t1 = std::chrono::steady_clock::now();
    r.c.seconds += std::chrono::duration<double>(t1 - t0).count();
    for (Lane &L : e->lanes)
        if (L.rc) return fail(e, L.rc, "lane %d: %s", L.index, L.err.c_str());
    return AZ_OK;
}

static int active_slots(const az_engine *e)
{
    int a = 0;
    for (const Lane &L : e->lanes) a += L.active;
    return a;
}

// the column sums, over every slot of every lane, of a per-slot statistics buffer [B][K] of 64-bit counts
static int sum_slot_stats(az_engine *e, DevBuf Lane::*buf, int K, int64_t *sums)
{
    std::fill(sums, sums + K, (int64_t)0);
    std::vector<unsigned long long> h;
    for (Lane &L : e->lanes) {
        h.resize((size_t)L.d.B * K);
        HIPCHECK(e, az_memcpy(L.stream, h.data(), (L.*buf).p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h.size(); i++) sums[i % K] += (int64_t)h[i];
    }
    return AZ_OK;
}

static int read_counters(az_engine *e, az_counters &c)
{
    int64_t cnt[CNT_STRIDE];
    int rc = sum_slot_stats(e, &Lane::cnt, CNT_STRIDE, cnt);
    e->solver_stops = 0;
    if (!rc && e->episode_solver && e->lanes[0].proof_stops.p) rc = sum_slot_stats(e, &Lane::proof_stops, 1, &e->solver_stops);
    if (!rc && e->run.delta) rc = sum_slot_stats(e, &Lane::delta_cnt, DELTA_CNT, e->delta_stats);
    if (!rc && e->episode_threat) rc = sum_slot_stats(e, &Lane::threat_stat, THREAT_STATS, e->threat_stats);
    if (rc) return rc;
    c.expansions = cnt[0]; c.simulations = cnt[1]; c.terminal_hits = cnt[2]; c.depth_sum = cnt[3];
    const int64_t reused = cnt[4];
    c.duplicate_leaves = cnt[5]; c.cache_lookups = cnt[6]; c.cache_hits = cnt[7];
    c.steps = c.trunk_launches = c.plies = 0;
    double trunk_ms = 0.0, nn_ms = 0.0, step_ms = 0.0, tape_wait = 0.0;
    for (Lane &L : e->lanes) {
        c.steps += L.steps; c.trunk_launches += L.trunk_launches; c.plies += L.plies;
        trunk_ms += L.trunk_ms; nn_ms += L.nn_ms; step_ms += L.step_ms;
        if (L.tape_wait_s > tape_wait) tape_wait = L.tape_wait_s;
    }
    c.tape_wait_seconds = tape_wait;
    c.tape_threads = e->rng_mode != AZ_RNG_PHILOX && (e->tapes || e->stream_tapes) ? e->tape_threads : 0;
    c.host_cpus = e->host_cpus;
    e->run.reused_roots = reused;
    c.trunk_seconds = trunk_ms * 1e-3;
    c.nn_seconds = nn_ms * 1e-3;
    c.step_seconds = step_ms * 1e-3;
    c.root_evals = c.plies - reused;      // a retained root (subtree reuse) is not evaluated again
    c.records = c.plies;
    c.trunk_boards = e->run.ext ? 0 : c.expansions + c.root_evals - c.cache_hits;     // evaluations the net kernels actually ran
    c.games = e->run.num_games;
    return AZ_OK;
}

static int episode_end(az_engine *e, az_counters *out)
{
    az_engine::Run &r = e->run;
    if (!r.open) return fail(e, AZ_ERR_STATE, "no episode is open");
    int rc = read_counters(e, r.c);
    if (rc) return rc;
    e->h_nply.assign(r.num_games, 0);
    e->h_result.assign(r.num_games, 0);
    HIPCHECK(e, az_memcpy(e->stream, e->h_nply.data(), e->g_nply.p, (size_t)r.num_games * 4, hipMemcpyDeviceToHost));
    HIPCHECK(e, az_memcpy(e->stream, e->h_result.data(), e->g_result.p, (size_t)r.num_games * 4, hipMemcpyDeviceToHost));
    e->h_cross.assign(r.num_games, -1);
    HIPCHECK(e, az_memcpy(e->stream, e->h_cross.data(), e->g_cross.p, (size_t)r.num_games * 4, hipMemcpyDeviceToHost));
    e->h_key0 = r.game_key0;
    e->h_permille = r.arena || r.preset ? 0 : e->resign_permille;
    e->h_cap_fast = r.cap_fast; e->h_cap_permille = r.cap_permille; e->h_cap_export_full = r.cap_export_full;
    if (r.preset) {
        e->h_nply.assign(r.num_games, 1);   // a preset search plays exactly one ply; the game itself is not finished by it
    } else {
        // games still in flight when the caller stops early: report the plies played so far
        for (Lane &L : e->lanes) {
            const int B = L.d.B;
            std::vector<int> sg(B), sp(B), ss(B);
            HIPCHECK(e, az_memcpy(L.stream, sg.data(), L.s_game.p, sg.size() * 4, hipMemcpyDeviceToHost));
            HIPCHECK(e, az_memcpy(L.stream, sp.data(), L.s_ply.p, sp.size() * 4, hipMemcpyDeviceToHost));
            HIPCHECK(e, az_memcpy(L.stream, ss.data(), L.s_status.p, ss.size() * 4, hipMemcpyDeviceToHost));
            for (int b = 0; b < B; b++)
                if (ss[b] == SLOT_ACTIVE && sg[b] >= 0 && sg[b] < r.num_games) e->h_nply[sg[b]] = sp[b];
        }
    }
    // the device counts plies from the empty board; from here on h_nply is the plies searched (a game not begun stays 0)
    e->h_start.assign(r.num_games, 0);
    for (int g = 0; g < (int)r.start.size(); g++) {
        e->h_start[g] = r.start[g];
        e->h_nply[g] = std::max(0, e->h_nply[g] - r.start[g]);
    }
    int64_t plies = 0;
    for (int g = 0; g < r.num_games; g++) plies += e->h_nply[g];
    r.c.plies = r.c.records = plies;
    r.c.root_evals = plies - r.reused_roots;
    r.c.trunk_boards = r.ext ? 0 : r.c.expansions + r.c.root_evals - r.c.cache_hits;
    if (r.ext) ext_restore(e);
    e->last = r.c;
    e->episode_games = r.num_games;
    e->have_episode = true;
    r.open = false;
    stop_tapes(e);
    if (out) *out = r.c;
    return AZ_OK;
}

// every ply of the episode that `begun` (the result of its begin call) opened, and its end
static int play_episode(az_engine *e, int begun, az_counters *out)
{
    int rc = begun;
    if (!rc) rc = episode_plies(e, 1 << 30);
    if (!rc) rc = episode_end(e, out);
    if (rc) abandon_episode(e);
    return rc;
}
static int run_episode(az_engine *e, const EpisodeSpec &sp, az_counters *out) { return play_episode(e, episode_begin(e, sp), out); }

static int upload_T(az_engine *e, const double *table, bool arena)
{
    const int nn = e->nn;
    std::vector<double> T(nn + 4);
    for (int m = 0; m < nn + 4; m++) {
        if (table && m <= nn) T[m] = table[m];
        else T[m] = arena ? 0.3 * std::exp(-(double)m / 4.0) : (std::exp(-(double)m / 100.0) + 0.01) / 1.01;
    }
    HIPCHECK(e, hipMemcpyAsync(e->T_table.p, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    return AZ_OK;
}

extern "C" int az_selfplay_begin(az_engine *e, const az_selfplay_args *a)
{
    if (!e || !a || a->num_games < 1) return fail(e, AZ_ERR_INVALID, "az_selfplay: bad argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_selfplay_begin: an episode is already open (az_selfplay_end first)");
    DEVICE_GUARD(e);
    const int nn = e->nn, G = a->num_games;
    if (e->start_count > 0 && a->max_plies > 0 && e->start_max_ply >= a->max_plies)
        return fail(e, AZ_ERR_INVALID, "az_selfplay: a start position already holds %d stones, max_plies is %d", e->start_max_ply, a->max_plies);
    int rc = ensure_episode_buffers(e, G, true);
    if (rc) return rc;
    if ((rc = upload_T(e, a->temperature_table, false))) return rc;
    // tapes: explicit, or numpy-compatible RandomState(seed0 + g) streams generated on the host cores
    const int plies = a->max_plies > 0 && a->max_plies < nn ? a->max_plies : nn;
    if (a->noise_tape && a->u_tape) {
        // the explicit tape must cover every ply the games can reach: off(plies) = sum_{m < plies} (nn - m) doubles per game
        int64_t need = 0;
        for (int m = 0; m < plies; m++) need += nn - m;
        if (a->tape_stride < need) return fail(e, AZ_ERR_INVALID, "tape_stride %lld is shorter than the %lld doubles %d plies need", (long long)a->tape_stride, (long long)need, plies);
        HIPCHECK(e, hipMemcpy2DAsync(e->noise.p, (size_t)e->tape_len * 8, a->noise_tape, (size_t)a->tape_stride * 8,
                                     (size_t)std::min<int64_t>(a->tape_stride, e->tape_len) * 8, G, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(e->u.p, a->u_tape, (size_t)G * nn * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
    } else if (e->rng_mode == AZ_RNG_PHILOX) {
        // every ply of every game in one launch ahead of the first ply: no staging, no copy stream, no host thread
        HIPCHECK(e, az_tape_launch(e->stream, a->seed0, G, nn, 0, plies, e->cfg.dirichlet_alpha, e->gumbel_m > 0 ? AZ_TAPE_GUMBEL : AZ_TAPE_DIRICHLET,
                                   nullptr, (double *)e->noise.p, e->tape_len, (double *)e->u.p));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
    } else if (e->stream_tapes) {
        e->tapes = new TapeProducer();
        e->tapes->ahead = e->start_count > 0 ? e->start_max_ply : 0;      // a game's ply runs this far ahead of the episode's
        e->tapes->kind = e->gumbel_m > 0 ? 1 : 0;                          // az_set_gumbel: the legal-cell draws are Gumbel(0, 1)
        hipError_t trc = e->tapes->start(e->cfg.device, a->seed0, G, nn, plies, e->cfg.dirichlet_alpha, e->tape_len,
                                         (double *)e->noise.p, (double *)e->u.p, e->tape_threads);
        if (trc != hipSuccess) { stop_tapes(e); return fail(e, AZ_ERR_HIP, "tape producer: %s", hipGetErrorString(trc)); }
    } else {
        const int chunk = 256;
        std::vector<double> hn((size_t)chunk * e->tape_len), hu((size_t)chunk * nn);
        for (int g0 = 0; g0 < G; g0 += chunk) {
            int cnt = std::min(chunk, G - g0);
            azrng::selfplay_tapes_parallel(a->seed0, g0, cnt, nn, e->cfg.dirichlet_alpha, plies, hn.data(), e->tape_len,
                                           hu.data(), host_threads(), e->gumbel_m > 0 ? 1 : 0);
            HIPCHECK(e, az_memcpy(e->stream, (double *)e->noise.p + (size_t)g0 * e->tape_len, hn.data(), (size_t)cnt * e->tape_len * 8,
                                  hipMemcpyHostToDevice));
            HIPCHECK(e, az_memcpy(e->stream, (double *)e->u.p + (size_t)g0 * nn, hu.data(), (size_t)cnt * nn * 8, hipMemcpyHostToDevice));
        }
    }
    EpisodeSpec sp;
    sp.num_games = G; sp.max_plies = a->max_plies; sp.add_noise = true; sp.arena = false;
    sp.game_key0 = (unsigned)a->seed0;
    return episode_begin(e, sp);
}

extern "C" int az_selfplay_step(az_engine *e, int max_steps, int32_t *active_out, az_counters *progress)
{
    if (!e || max_steps < 0) return fail(e, AZ_ERR_INVALID, "az_selfplay_step: bad argument");
    DEVICE_GUARD(e);
    int rc = episode_plies(e, max_steps);
    if (rc) return rc;
    if (active_out) *active_out = active_slots(e);
    if (progress) {
        az_counters c = e->run.c;
        if ((rc = read_counters(e, c))) return rc;
        *progress = c;
    }
    return AZ_OK;
}

extern "C" int az_selfplay_end(az_engine *e, az_counters *out)
{
    if (!e) return AZ_ERR_INVALID;
    DEVICE_GUARD(e);
    const int rc = episode_end(e, out);
    if (rc) abandon_episode(e);
    return rc;
}

extern "C" int az_selfplay(az_engine *e, const az_selfplay_args *a, az_counters *out)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_selfplay: an episode is already open (az_selfplay_end first)");
    DEVICE_GUARD(e);
    return play_episode(e, az_selfplay_begin(e, a), out);
}

extern "C" int az_selfplay_games(az_engine *e, int32_t *nply, int32_t *result)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    for (int g = 0; g < e->episode_games; g++) {
        if (nply) nply[g] = e->h_nply[g];
        if (result) result[g] = e->h_result[g];
    }
    return AZ_OK;
}

// Every record of the last episode, game-major then ply: f(g, ply, src_index, r) with the game, the absolute ply (the device
// counts plies from the empty board), the record's place g * nn + ply in the device's [G][nn] arrays and its running number.
template <class F>
static void for_each_record(const az_engine *e, F f)
{
    size_t r = 0;
    for (int g = 0; g < e->episode_games; g++)
        for (int m = 0; m < e->h_nply[g]; m++, r++) {
            const int ply = e->h_start[g] + m;
            f(g, ply, (size_t)g * e->nn + ply, r);
        }
}

// one value per record, out of a device array [G][nn] of T
template <class T>
static int read_record_array(az_engine *e, const DevBuf &b, T *out)
{
    std::vector<T> h((size_t)e->episode_games * e->nn);
    HIPCHECK(e, az_memcpy(e->stream, h.data(), b.p, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    for_each_record(e, [&](int, int, size_t si, size_t r) { out[r] = h[si]; });
    return AZ_OK;
}

extern "C" int az_selfplay_records(az_engine *e, uint8_t *boards, uint8_t *movers, int16_t *lasts, int16_t *actions,
                                   float *pis, int32_t *visits, int8_t *z)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    DEVICE_GUARD(e);
    const int nn = e->nn, G = e->episode_games;
    const size_t tot = (size_t)G * nn;
    std::vector<u64> pl(tot * 8);
    std::vector<unsigned char> mv(tot);
    std::vector<float> pi(tot * nn);
    std::vector<unsigned short> vis(tot * nn);
    HIPCHECK(e, az_memcpy(e->stream, pl.data(), e->rec_planes.p, pl.size() * 8, hipMemcpyDeviceToHost));
    HIPCHECK(e, az_memcpy(e->stream, mv.data(), e->rec_mover.p, mv.size(), hipMemcpyDeviceToHost));
    HIPCHECK(e, az_memcpy(e->stream, pi.data(), e->rec_pi.p, pi.size() * 4, hipMemcpyDeviceToHost));
    HIPCHECK(e, az_memcpy(e->stream, vis.data(), e->rec_visits.p, vis.size() * 2, hipMemcpyDeviceToHost));
    int rc = lasts ? read_record_array(e, e->rec_last, lasts) : AZ_OK;
    if (!rc && actions) rc = read_record_array(e, e->rec_action, actions);
    if (rc) return rc;
    for_each_record(e, [&](int g, int, size_t si, size_t r) {
        const int mover = mv[si];
        if (boards)
            for (int j = 0; j < nn; j++) {
                bool me = (pl[si * 8 + (j >> 6)] >> (j & 63)) & 1ull, op = (pl[si * 8 + 4 + (j >> 6)] >> (j & 63)) & 1ull;
                boards[r * nn + j] = (uint8_t)(me ? mover : (op ? 3 - mover : 0));
            }
        if (movers) movers[r] = (uint8_t)mover;
        if (pis) memcpy(pis + r * nn, pi.data() + si * nn, (size_t)nn * 4);
        if (visits) for (int j = 0; j < nn; j++) visits[r * nn + j] = vis[si * nn + j];
        const int res = e->h_result[g];
        if (z) z[r] = (int8_t)(res == 0 ? 99 : (res == 3 ? 0 : (mover == res ? 1 : -1)));
    });
    return AZ_OK;
}

extern "C" int az_selfplay_clear(az_engine *e)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_selfplay_clear: an episode is open (az_selfplay_end first)");
    e->have_episode = false;
    return AZ_OK;
}

// source index (game * nn + absolute ply) of every record of the last episode, game-major then ply, on the device
// ... of every record the export carries: with az_set_playout_cap(export_full_only = 1) the records of FULL plies only
static bool exported(const az_engine *e, int g, int ply)
{
    return !(e->h_cap_fast && e->h_cap_export_full) || az_playout_cap_full(e->h_key0 + (uint32_t)g, ply, e->h_cap_permille);
}
static int upload_src_index(az_engine *e, int64_t *records)
{
    std::vector<int> src;
    for_each_record(e, [&](int g, int ply, size_t si, size_t) { if (exported(e, g, ply)) src.push_back((int)si); });
    *records = (int64_t)src.size();
    return src.empty() ? AZ_OK : upload(e, e->src_index, src.data(), src.size() * 4);
}
static int64_t export_records(const az_engine *e)
{
    int64_t n = 0;
    for_each_record(e, [&](int g, int ply, size_t, size_t) { n += exported(e, g, ply) ? 1 : 0; });
    return n;
}

extern "C" int64_t az_record_bytes(const az_engine *e) { return e ? record_bytes(e->nn) : 0; }

extern "C" int az_selfplay_pack(az_engine *e, void *packed_dev)
{
    if (!e || !e->have_episode || !packed_dev) return fail(e, AZ_ERR_STATE, "az_selfplay_pack: no episode / null buffer");
    DEVICE_GUARD(e);
    const int nn = e->nn;
    int64_t records = 0;
    int rc = upload_src_index(e, &records);
    if (rc || records == 0) return rc;
    hipLaunchKernelGGL(k_pack, dim3((unsigned)records), dim3(64), 0, e->stream, e->lanes[0].d, (const int *)e->src_index.p,
                       records, nn, record_bytes(nn), (unsigned char *)packed_dev);
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    HIPCHECK(e, hipGetLastError());
    return AZ_OK;
}

// ---- the search value per record, and resignation ----
extern "C" int az_selfplay_values(az_engine *e, float *values)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    if (!values) return fail(e, AZ_ERR_INVALID, "az_selfplay_values: null buffer");
    DEVICE_GUARD(e);
    return read_record_array(e, e->rec_value, values);
}

extern "C" int az_selfplay_pack_values(az_engine *e, float *values_dev)
{
    if (!e || !e->have_episode || !values_dev) return fail(e, AZ_ERR_STATE, "az_selfplay_pack_values: no episode / null buffer");
    DEVICE_GUARD(e);
    int64_t records = 0;
    int rc = upload_src_index(e, &records);
    if (rc || records == 0) return rc;
    hipLaunchKernelGGL(k_pack_values, dim3((unsigned)((records + 255) / 256)), dim3(256), 0, e->stream, (const float *)e->rec_value.p,
                       (const int *)e->src_index.p, records, values_dev);
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    HIPCHECK(e, hipGetLastError());
    return AZ_OK;
}

extern "C" uint32_t az_resign_mix(uint32_t x)     // the host's az_fmix32 (az_device.h), which k_move names the exempt games by
{
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

extern "C" int az_resign_exempt(uint32_t key, int playout_permille)
{
    return (int)(az_resign_mix(key) % 1000u) < playout_permille ? 1 : 0;
}

extern "C" int az_set_resign(az_engine *e, double threshold, int min_ply, int playout_permille)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_resign: an episode is open (az_selfplay_end first)");
    if (!(threshold >= 0.0 && threshold <= 1.0) || min_ply < 0 || playout_permille < 0 || playout_permille > 1000)
        return fail(e, AZ_ERR_INVALID, "az_set_resign: threshold %g (0 = off, else in (0, 1]), min_ply %d (>= 0), playout_permille %d (0..1000)",
                    threshold, min_ply, playout_permille);
    e->resign_thr = threshold; e->resign_min_ply = min_ply; e->resign_permille = playout_permille;
    return AZ_OK;
}

extern "C" int az_get_resign(const az_engine *e, double *threshold, int *min_ply, int *playout_permille)
{
    if (!e) return AZ_ERR_INVALID;
    if (threshold) *threshold = e->resign_thr;
    if (min_ply) *min_ply = e->resign_min_ply;
    if (playout_permille) *playout_permille = e->resign_permille;
    return AZ_OK;
}

// ---- playout cap randomisation ----
extern "C" int az_playout_cap_full(uint32_t key, int ply, int full_permille)
{
    return (int)(az_resign_mix(key ^ az_resign_mix((uint32_t)ply + 0x9E3779B9u)) % 1000u) < full_permille ? 1 : 0;
}

extern "C" int az_set_playout_cap(az_engine *e, int fast_sims, int full_permille, int export_full_only)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_playout_cap: an episode is open (az_selfplay_end first)");
    if (fast_sims == 0) {
        e->cap_fast = e->cap_permille = e->cap_export_full = 0;
        return AZ_OK;
    }
    if (fast_sims < 1 || fast_sims > e->cfg.num_simulations || full_permille < 0 || full_permille > 1000 ||
        (export_full_only != 0 && export_full_only != 1))
        return fail(e, AZ_ERR_INVALID, "az_set_playout_cap: fast_sims %d (0 = off, else 1..%d), full_permille %d (0..1000), export_full_only %d (0 / 1)",
                    fast_sims, e->cfg.num_simulations, full_permille, export_full_only);
    if (refuse_conflicts(e, SET_CAP)) return AZ_ERR_INVALID;
    e->cap_fast = fast_sims; e->cap_permille = full_permille; e->cap_export_full = export_full_only;
    return AZ_OK;
}

extern "C" int az_get_playout_cap(const az_engine *e, int *fast_sims, int *full_permille, int *export_full_only)
{
    if (!e) return AZ_ERR_INVALID;
    if (fast_sims) *fast_sims = e->cap_fast;
    if (full_permille) *full_permille = e->cap_permille;
    if (export_full_only) *export_full_only = e->cap_export_full;
    return AZ_OK;
}

// ---- forced playouts and policy target pruning ----
extern "C" int az_set_forced_playouts(az_engine *e, double k, int prune)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_forced_playouts: an episode is open (az_selfplay_end first)");
    if (k == 0.0) {
        e->forced_k = 0.0; e->forced_prune = 0;
        return AZ_OK;
    }
    if (!(k > 0.0 && k <= 16.0) || (prune != 0 && prune != 1))
        return fail(e, AZ_ERR_INVALID, "az_set_forced_playouts: k %g (0 = off, else in (0, 16]), prune %d (0 / 1)", k, prune);
    if (refuse_conflicts(e, SET_FORCED)) return AZ_ERR_INVALID;
    e->forced_k = k; e->forced_prune = prune;
    return AZ_OK;
}

extern "C" int az_get_forced_playouts(const az_engine *e, double *k, int *prune)
{
    if (!e) return AZ_ERR_INVALID;
    if (k) *k = e->forced_k;
    if (prune) *prune = e->forced_prune;
    return AZ_OK;
}

// k_move's pruning pass on one root row of `count` legal children, with the functions the kernel uses (az_tree.h)
extern "C" int64_t az_forced_prune(double k, double c_puct, int count, const int32_t *visits, const double *W, const float *prior, int32_t *out)
{
    if (!(k > 0.0 && k <= 16.0) || count < 1 || !visits || !W || !prior || !out) return -1;
    int64_t total = 0;
    int star = 0;
    for (int c = 0; c < count; c++) {
        if (visits[c] < 0 || visits[c] > 0xFFFF) return -1;
        total += visits[c];
        if (visits[c] > visits[star]) star = c;            // the most visited child, the lowest on ties
    }
    if (total < 1 || total > 0xFFFF) return -1;
    const double sq = sqrt((double)total + 1e-8);           // the engine's table: np.sqrt(total + 1e-8)
    const double target = forced_score(W[star] / (double)visits[star], c_puct, prior[star], sq, visits[star]);
    int64_t removed = 0;
    for (int c = 0; c < count; c++) {
        out[c] = visits[c];
        if (c != star && visits[c] > 0)
            out[c] = forced_pruned(k, c_puct, W[c] / (double)visits[c], prior[c], visits[c], (int)total, sq, target);
        removed += visits[c] - out[c];
    }
    return removed;
}

// ---- selection rule: first-play urgency and visit-dependent c_puct ----
// the two tables as the engine uploads them: cpuct[i] = c(i) for i = 0..S+1, mass[i] = sqrt(i / 4096) for i = 0..4096
static void selection_tables(double c_puct, double base, double factor, int count, double *cpuct, double *mass)
{
    // factor = 0 gives c_puct exactly: 0 * log(x) is +0 for every finite log
    for (int i = 0; i < count; i++) cpuct[i] = c_puct + factor * std::log(((double)i + base + 1.0) / base);
    for (int i = 0; i <= SEL_MASS_STEPS; i++) mass[i] = std::sqrt((double)i / (double)SEL_MASS_STEPS);
}

static bool selection_args_ok(double fpu, double fpu_root, double base, double factor)
{
    return std::isfinite(fpu) && fpu >= 0.0 && fpu <= 2.0 && std::isfinite(fpu_root) && fpu_root >= 0.0 && fpu_root <= 2.0 &&
           std::isfinite(factor) && factor >= 0.0 && factor <= 16.0 && std::isfinite(base) && base >= 1.0;
}

extern "C" int az_selection_tables(double c_puct, double cpuct_base, double cpuct_factor, int S, double *cpuct, double *mass)
{
    if (!std::isfinite(c_puct) || !selection_args_ok(0.0, 0.0, cpuct_base, cpuct_factor) || S < 1 || S > AZ_DEEP_MAX_SIMULATIONS ||
        !cpuct || !mass)
        return AZ_ERR_INVALID;
    selection_tables(c_puct, cpuct_base, cpuct_factor, S + 2, cpuct, mass);
    return AZ_OK;
}

extern "C" int az_set_selection(az_engine *e, int on, double fpu, double fpu_root, double cpuct_base, double cpuct_factor)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_selection: an episode is open (az_selfplay_end first)");
    if (!on) {
        e->sel_on = 0;
        return AZ_OK;
    }
    if (on != 1 || !selection_args_ok(fpu, fpu_root, cpuct_base, cpuct_factor))
        return fail(e, AZ_ERR_INVALID, "az_set_selection: on %d (0 / 1), fpu %g and fpu_root %g (in [0, 2]), cpuct_base %g (>= 1), cpuct_factor %g (in [0, 16])",
                    on, fpu, fpu_root, cpuct_base, cpuct_factor);
    if (refuse_conflicts(e, SET_SELECTION)) return AZ_ERR_INVALID;
    DEVICE_GUARD(e);
    // sized like sqrt_table (S + 3 entries, the last one never read) so that every index the sqrt takes is good for c(count) too
    const int S = e->cfg.num_simulations;
    std::vector<double> ct((size_t)S + 3), mt((size_t)SEL_MASS_STEPS + 1);
    selection_tables(e->cfg.c_puct, cpuct_base, cpuct_factor, S + 3, ct.data(), mt.data());
    int rc = upload(e, e->sel_cpuct, ct.data(), ct.size() * sizeof(double));
    if (!rc) rc = upload(e, e->sel_mass, mt.data(), mt.size() * sizeof(double));
    for (Lane &L : e->lanes)
        if (!rc) rc = dev_alloc(e, L.root_v, (size_t)L.d.B * sizeof(float));
    if (rc) return rc;
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    for (Lane &L : e->lanes) L.d.root_v = (float *)L.root_v.p;
    each_state(e, [&](DevState &d) { (void)d; });        // refresh the item views
    e->sel_on = 1; e->sel_fpu = fpu; e->sel_fpu_root = fpu_root; e->sel_base = cpuct_base; e->sel_factor = cpuct_factor;
    return AZ_OK;
}

extern "C" int az_get_selection(const az_engine *e, int *on, double *fpu, double *fpu_root, double *cpuct_base, double *cpuct_factor)
{
    if (!e) return AZ_ERR_INVALID;
    if (on) *on = e->sel_on;
    if (fpu) *fpu = e->sel_fpu;
    if (fpu_root) *fpu_root = e->sel_fpu_root;
    if (cpuct_base) *cpuct_base = e->sel_base;
    if (cpuct_factor) *cpuct_factor = e->sel_factor;
    return AZ_OK;
}

// ---- candidate moves: expansion, noise and selection over the empty cells near the stones ----
// the rule on the host: mask[j] = 1 for the cells of C(X); radius 0 = the option off, every empty cell
extern "C" int az_candidate_mask(int n, const uint8_t *board, int radius, uint8_t *mask)
{
    if (n < 3 || n > 15 || !board || !mask || radius < 0 || radius > n - 1) return AZ_ERR_INVALID;
    const int nn = n * n;
    int stones = 0;
    for (int j = 0; j < nn; j++) {
        if (board[j] > 2) return AZ_ERR_INVALID;
        stones += board[j] != 0;
    }
    for (int j = 0; j < nn; j++) {
        bool in = board[j] == 0 && (stones == 0 || radius == 0);
        if (board[j] == 0 && !in) {
            const int r = j / n, c = j % n;
            for (int rr = std::max(0, r - radius); rr <= std::min(n - 1, r + radius) && !in; rr++)
                for (int cc = std::max(0, c - radius); cc <= std::min(n - 1, c + radius) && !in; cc++) in = board[rr * n + cc] != 0;
        }
        mask[j] = in ? 1 : 0;
    }
    return AZ_OK;
}

extern "C" int az_set_candidates(az_engine *e, int radius)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_candidates: an episode is open (az_selfplay_end first)");
    if (radius < 0 || radius > e->n - 1) return fail(e, AZ_ERR_INVALID, "az_set_candidates: radius %d (0 = off, or 1 .. %d)", radius, e->n - 1);
    if (radius && refuse_conflicts(e, SET_CANDIDATES)) return AZ_ERR_INVALID;
    e->cand_radius = radius;
    return AZ_OK;
}

extern "C" int az_get_candidates(const az_engine *e, int *radius)
{
    if (!e) return AZ_ERR_INVALID;
    if (radius) *radius = e->cand_radius;
    return AZ_OK;
}

// ---- Gumbel root search: sequential halving and completed-Q policy targets ----
// seq[t] = the visit count a root child must have to be selectable at simulation t, for k candidates and S simulations
extern "C" int az_gumbel_schedule(int k, int S, int32_t *out)
{
    if (k < 0 || S < 1 || S > AZ_DEEP_MAX_SIMULATIONS || !out) return AZ_ERR_INVALID;
    if (k <= 1) {
        for (int t = 0; t < S; t++) out[t] = t;
        return AZ_OK;
    }
    int L = 0;
    while ((1 << L) < k) L++;                                   // ceil(log2 k)
    std::vector<int32_t> visits((size_t)k, 0);
    int c = k, n = 0;
    while (n < S) {
        const int extra = std::max(1, S / (L * c));
        for (int x = 0; x < extra && n < S; x++)
            for (int i = 0; i < c; i++) {
                if (n < S) out[n++] = visits[i];
                visits[i]++;
            }
        c = std::max(2, c / 2);
    }
    return AZ_OK;
}

extern "C" int az_set_gumbel(az_engine *e, int m, double c_visit, double c_scale)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_gumbel: an episode is open (az_selfplay_end first)");
    if (m == 0) {
        e->gumbel_m = 0;
        return AZ_OK;
    }
    if (m < 0 || m > std::min(e->nn, 64) || !(c_visit >= 0.0) || !std::isfinite(c_visit) || !(c_scale > 0.0) || !std::isfinite(c_scale))
        return fail(e, AZ_ERR_INVALID, "az_set_gumbel: m %d (0 = off, else 1..%d), c_visit %g (>= 0), c_scale %g (> 0)", m,
                    std::min(e->nn, 64), c_visit, c_scale);
    if (refuse_conflicts(e, SET_GUMBEL)) return AZ_ERR_INVALID;
    DEVICE_GUARD(e);
    // the schedules of k = 1 .. m candidates (a root has min(m, legal cells) of them), one row of S entries each
    const int S = e->cfg.num_simulations;
    std::vector<int32_t> row((size_t)S);
    std::vector<uint16_t> tab((size_t)m * S);
    for (int k = 1; k <= m; k++) {
        az_gumbel_schedule(k, S, row.data());
        for (int t = 0; t < S; t++) tab[(size_t)(k - 1) * S + t] = (uint16_t)row[t];
    }
    int rc = upload(e, e->gumbel_seq, tab.data(), tab.size() * sizeof(uint16_t));
    for (Lane &L : e->lanes) {
        if (!rc) rc = dev_alloc(e, L.root_logits, (size_t)L.d.B * e->RW * sizeof(float));
        if (!rc) rc = dev_alloc(e, L.root_v, (size_t)L.d.B * sizeof(float));
    }
    if (rc) return rc;
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    for (Lane &L : e->lanes) {
        L.d.gumbel_seq = (const unsigned short *)e->gumbel_seq.p;
        L.d.root_logits = (float *)L.root_logits.p;
        L.d.root_v = (float *)L.root_v.p;
    }
    each_state(e, [&](DevState &d) { (void)d; });        // refresh the item views
    e->gumbel_m = m; e->gumbel_cv = c_visit; e->gumbel_cs = c_scale;
    return AZ_OK;
}

extern "C" int az_get_gumbel(const az_engine *e, int *m, double *c_visit, double *c_scale)
{
    if (!e) return AZ_ERR_INVALID;
    if (m) *m = e->gumbel_m;
    if (c_visit) *c_visit = e->gumbel_cv;
    if (c_scale) *c_scale = e->gumbel_cs;
    return AZ_OK;
}

extern "C" int az_set_rng(az_engine *e, int mode)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_rng: an episode is open (az_selfplay_end first)");
    if (mode != AZ_RNG_NUMPY && mode != AZ_RNG_PHILOX) return fail(e, AZ_ERR_INVALID, "az_set_rng: mode %d (AZ_RNG_NUMPY = 0, AZ_RNG_PHILOX = 1)", mode);
    e->rng_mode = mode;
    return AZ_OK;
}

extern "C" int az_get_rng(const az_engine *e) { return e ? e->rng_mode : AZ_ERR_INVALID; }

// k_tape on its own: buffers of the call's own, the engine's stream, the result copied back
extern "C" int az_rng_philox_tape_device(az_engine *e, uint64_t seed0, int games, double alpha, int max_plies, int kind, double *noise_out,
                                         double *u_out)
{
    if (!e || games < 0) return fail(e, AZ_ERR_INVALID, "az_rng_philox_tape_device: bad argument");
    if (kind != AZ_TAPE_DIRICHLET && kind != AZ_TAPE_GUMBEL) return fail(e, AZ_ERR_INVALID, "az_rng_philox_tape_device: kind %d (0 = Dirichlet, 1 = Gumbel)", kind);
    if (noise_out && kind == AZ_TAPE_DIRICHLET && !(alpha > 0.0 && std::isfinite(alpha)))
        return fail(e, AZ_ERR_INVALID, "az_rng_philox_tape_device: alpha %g (> 0)", alpha);
    if (games == 0) return AZ_OK;
    if (!u_out) return fail(e, AZ_ERR_INVALID, "az_rng_philox_tape_device: null argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_rng_philox_tape_device: a self-play episode is open on this engine");
    DEVICE_GUARD(e);
    const int nn = e->nn, plies = max_plies > 0 && max_plies < nn ? max_plies : nn;
    int64_t len = 0;
    for (int m = 0; m < plies; m++) len += nn - m;
    DevBuf dn, du;
    int rc = dev_alloc(e, du, (size_t)games * nn * sizeof(double), true);
    if (!rc && noise_out) rc = dev_alloc(e, dn, (size_t)games * len * sizeof(double), false);
    if (!rc) {
        hipError_t h = az_tape_launch(e->stream, seed0, games, nn, 0, plies, noise_out ? alpha : 1.0, kind, nullptr, (double *)dn.p, len, (double *)du.p);
        if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
        if (h == hipSuccess && noise_out) h = az_memcpy(e->stream, noise_out, dn.p, (size_t)games * len * sizeof(double), hipMemcpyDeviceToHost);
        if (h == hipSuccess) h = az_memcpy(e->stream, u_out, du.p, (size_t)games * nn * sizeof(double), hipMemcpyDeviceToHost);
        if (h != hipSuccess) rc = fail(e, AZ_ERR_HIP, "az_rng_philox_tape_device: %s", hipGetErrorString(h));
    }
    dev_free(dn); dev_free(du);
    return rc;
}

// v_mix of one root row, as az_gumbel_target and k_move form it (NaN for a bad argument): the piece of the target whose
// summation order a test wants to see on its own
extern "C" double az_gumbel_vmix(int count, const int32_t *visits, const double *W, const float *prior, float root_value)
{
    if (count < 1 || count > 225 || !visits || !W || !prior) return NAN;
    std::vector<double> a((size_t)count), b((size_t)count);
    int64_t total = 0;
    for (int c = 0; c < count; c++) {
        if (visits[c] < 0 || visits[c] > 0xFFFF) return NAN;
        total += visits[c];
        a[c] = visits[c] ? (double)prior[c] : 0.0;
        b[c] = a[c] * (visits[c] ? W[c] / (double)visits[c] : 0.0);
    }
    if (total < 1) return NAN;
    return gumbel_vmix(root_value, (double)total, pw_sum(a.data(), count), pw_sum(b.data(), count));
}

// k_move's Gumbel pass on one root row of `count` legal children, with the functions the kernel uses (az_tree.h, az_device.h)
extern "C" int az_gumbel_target(int count, const float *logits, const double *g, const int32_t *visits, const double *W,
                                const float *prior, float root_value, double c_visit, double c_scale, float *pi, int32_t *action)
{
    if (count < 1 || count > 225 || !logits || !g || !visits || !W || !prior || !pi || !action) return AZ_ERR_INVALID;
    if (!(c_visit >= 0.0) || !std::isfinite(c_visit) || !(c_scale > 0.0) || !std::isfinite(c_scale)) return AZ_ERR_INVALID;
    int max_n = 0;
    int64_t total = 0;
    for (int c = 0; c < count; c++) {
        if (visits[c] < 0 || visits[c] > 0xFFFF) return AZ_ERR_INVALID;
        max_n = std::max(max_n, (int)visits[c]);
        total += visits[c];
    }
    if (total < 1) return AZ_ERR_INVALID;
    const double sig = gumbel_sigma(c_visit, c_scale, max_n);
    std::vector<double> q((size_t)count), a((size_t)count), b((size_t)count), y((size_t)count);
    int best = -1;
    double bs = 0.0;
    for (int c = 0; c < count; c++) {
        q[c] = visits[c] ? W[c] / (double)visits[c] : 0.0;
        a[c] = visits[c] ? (double)prior[c] : 0.0;
        b[c] = a[c] * q[c];
        if (visits[c] == max_n) {
            const double s = gumbel_score(g[c] + (double)logits[c], sig, q[c]);
            if (best < 0 || s > bs) { bs = s; best = c; }      // the first maximum
        }
    }
    const double vmix = gumbel_vmix(root_value, (double)total, pw_sum(a.data(), count), pw_sum(b.data(), count));
    double m = -INFINITY;
    for (int c = 0; c < count; c++) {
        y[c] = gumbel_score((double)logits[c], sig, visits[c] ? q[c] : vmix);
        m = y[c] > m ? y[c] : m;
    }
    for (int c = 0; c < count; c++) y[c] = az_exp(y[c] - m);
    const double s = pw_sum(y.data(), count);
    const bool uniform = (s < 1e-8) || (s != s);
    for (int c = 0; c < count; c++) pi[c] = (float)(uniform ? 1.0 / (double)count : y[c] / s);
    *action = best;
    return AZ_OK;
}

extern "C" int az_selfplay_sims(az_engine *e, int32_t *sims)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    if (!sims) return fail(e, AZ_ERR_INVALID, "az_selfplay_sims: null buffer");
    for_each_record(e, [&](int g, int ply, size_t, size_t r) {
        sims[r] = e->h_cap_fast && !az_playout_cap_full(e->h_key0 + (uint32_t)g, ply, e->h_cap_permille) ? e->h_cap_fast : e->cfg.num_simulations;
    });
    return AZ_OK;
}

extern "C" int az_selfplay_export_count(az_engine *e, int64_t *records)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    if (!records) return fail(e, AZ_ERR_INVALID, "az_selfplay_export_count: null buffer");
    *records = export_records(e);
    return AZ_OK;
}

extern "C" int az_selfplay_resign_info(az_engine *e, int32_t *cross_ply, uint8_t *exempt)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    for (int g = 0; g < e->episode_games; g++) {
        if (cross_ply) cross_ply[g] = e->h_cross[g];
        if (exempt) exempt[g] = (uint8_t)az_resign_exempt(e->h_key0 + (uint32_t)g, e->h_permille);
    }
    return AZ_OK;
}

extern "C" int az_examples_from_packed(az_engine *e, const void *packed_dev, int64_t records, int aug, float *states_dev,
                                       float *pis_dev, float *z_dev)
{
    if (!e || records < 0) return fail(e, AZ_ERR_INVALID, "az_examples_from_packed: bad argument");
    if (aug != AZ_AUG_NONE && aug != AZ_AUG_REFERENCE4 && aug != AZ_AUG_DIHEDRAL8) return fail(e, AZ_ERR_INVALID, "aug must be 1, 4 or 8");
    if (records == 0) return AZ_OK;         // nothing to read or write: the buffers of an empty batch may be null
    if (!packed_dev || !states_dev || !pis_dev || !z_dev) return fail(e, AZ_ERR_INVALID, "az_examples_from_packed: bad argument");
    DEVICE_GUARD(e);
    hipLaunchKernelGGL(k_examples, dim3((unsigned)records), dim3(256), 0, e->stream, (const unsigned char *)packed_dev,
                       records, e->n, record_bytes(e->nn), aug, states_dev, pis_dev, z_dev);
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    HIPCHECK(e, hipGetLastError());
    return AZ_OK;
}

// ------------------------------------------------------------------------------------------------
// single-position entry points
// ------------------------------------------------------------------------------------------------
static void planes_from_cells(const uint8_t *cells, int nn, u64 *x, u64 *o)
{
    for (int q = 0; q < 4; q++) x[q] = o[q] = 0;
    for (int j = 0; j < nn; j++) {
        if (cells[j] == 1) x[j >> 6] |= 1ull << (j & 63);
        else if (cells[j] == 2) o[j >> 6] |= 1ull << (j & 63);
    }
}

// az_net_eval_delta's part of eval_positions: the root every position is evaluated as a delta of, and where the path taken goes
struct DeltaRoot {
    const uint8_t *cells;
    int player;
    int32_t *path;
};

// The evaluation of `count` given positions on lane 0 (single-position and batch evaluation calls use lane 0), a pass at a time:
// the planes as the mover sees them into the first items of the lane, launch(lc, cnt) for the trunk, then the FC layers and
// the policy / value tail, and the rows copied back.  root: the delta call's extras, nullptr for the full evaluation.  The
// lane is left idle and empty on every way out.
template <class Launch>
static int eval_positions(az_engine *e, const char *who, int slot, int count, const uint8_t *boards, const uint8_t *players,
                          const int16_t *lasts, float *logits, float *policy, float *value, const DeltaRoot *root, Launch launch)
{
    Lane &L = e->lanes[0];
    const int nn = e->nn;
    // What the two calls differ in beyond their trunk kernels.  The full evaluation fills the lane's evaluation ITEMS, slots x
    // leaves per batch (az_set_virtual_loss), and launches over all of them: a pass is an evaluation batch of the search.  A
    // delta evaluation is of one leaf per SLOT, as the search's is (delta_eligible: no virtual-loss batching): base activations,
    // root board and mover are per slot, so a pass holds the lane's slots, the kernels see the slots as their items
    // (lc.dv = lc.d below) and run over the positions of the pass only.
    const DevState &v = root ? L.d : L.dv;
    const int B = v.B;
    int *const d_status = v.s_status, *const d_net = v.s_net;
    IdleLanes idle{e, 1};
    DevBuf dpol, dval;
    int rc = dev_alloc(e, dpol, (size_t)B * nn * 4);
    if (!rc) rc = dev_alloc(e, dval, (size_t)B * 4);
    u64 rx[4] = {}, ro[4] = {};
    if (root) planes_from_cells(root->cells, nn, rx, ro);
    for (int c0 = 0; !rc && c0 < count; c0 += B) {
        const int cnt = std::min(B, count - c0);
        std::vector<u64> lf((size_t)B * 8, 0), bd(root ? (size_t)B * 8 : 0, 0);
        std::vector<int> kind(B, LEAF_NONE), st(B, SLOT_IDLE), nets(B, slot), ll(B, -1), pl(B, root ? root->player : 0);
        for (int i = 0; i < cnt; i++) {
            u64 x[4], o[4];
            planes_from_cells(boards + (size_t)(c0 + i) * nn, nn, x, o);
            const bool xm = players[c0 + i] == 1;
            for (int q = 0; q < 4; q++) { lf[(size_t)i * 8 + q] = xm ? x[q] : o[q]; lf[(size_t)i * 8 + 4 + q] = xm ? o[q] : x[q]; }
            for (int q = 0; root && q < 4; q++) { bd[(size_t)i * 8 + q] = rx[q]; bd[(size_t)i * 8 + 4 + q] = ro[q]; }
            kind[i] = LEAF_ROOT; st[i] = SLOT_ACTIVE; ll[i] = lasts[c0 + i];
        }
        hipError_t hr = az_memcpy(e->stream, L.leaf.p, lf.data(), lf.size() * 8, hipMemcpyHostToDevice);
        if (hr == hipSuccess && root) hr = az_memcpy(e->stream, L.board.p, bd.data(), bd.size() * 8, hipMemcpyHostToDevice);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, L.leaf_kind.p, kind.data(), (size_t)B * 4, hipMemcpyHostToDevice);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, d_status, st.data(), (size_t)B * 4, hipMemcpyHostToDevice);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, d_net, nets.data(), (size_t)B * 4, hipMemcpyHostToDevice);
        if (hr == hipSuccess && root) hr = az_memcpy(e->stream, L.s_player.p, pl.data(), (size_t)B * 4, hipMemcpyHostToDevice);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, L.leaf_last.p, ll.data(), (size_t)B * 4, hipMemcpyHostToDevice);
        if (hr != hipSuccess) { rc = fail(e, AZ_ERR_HIP, "%s upload: %s", who, hipGetErrorString(hr)); break; }
        LaunchCtx lc = ctx_of_impl(e, L);
        lc.d.leaf_sym = lc.dv.leaf_sym = nullptr;       // controller.py:39-53 evaluates the position as it is
        if (root) { lc.d.B = cnt; lc.dv = lc.d; }
        launch(lc, cnt);
        e->ops->fc(lc, slot);
        e->ops->eval_tail(lc, cnt, (float *)dpol.p, (float *)dval.p);
        hr = hipStreamSynchronize(e->stream);
        if (hr == hipSuccess) hr = hipGetLastError();
        if (hr == hipSuccess && logits)
            hr = az_memcpy2d(e->stream, logits + (size_t)c0 * nn, (size_t)nn * 4, L.logits.p, (size_t)e->RW * 4, (size_t)nn * 4, cnt, hipMemcpyDeviceToHost);
        if (hr == hipSuccess && policy) hr = az_memcpy(e->stream, policy + (size_t)c0 * nn, dpol.p, (size_t)cnt * nn * 4, hipMemcpyDeviceToHost);
        if (hr == hipSuccess && value) hr = az_memcpy(e->stream, value + c0, dval.p, (size_t)cnt * 4, hipMemcpyDeviceToHost);
        if (hr == hipSuccess && root && root->path) {
            std::vector<unsigned char> done(cnt, 0);
            hr = az_memcpy(e->stream, done.data(), L.delta_done.p, (size_t)cnt, hipMemcpyDeviceToHost);
            for (int i = 0; i < cnt; i++) root->path[c0 + i] = (int)done[i] - 1;      // conv3 tiles of a delta evaluation, -1 = evaluated in full
        }
        if (hr != hipSuccess) { rc = fail(e, AZ_ERR_HIP, "%s: %s", who, hipGetErrorString(hr)); break; }
    }
    dev_free(dpol);
    dev_free(dval);
    return rc;
}

extern "C" int az_net_eval(az_engine *e, int slot, int count, const uint8_t *boards, const uint8_t *players,
                           const int16_t *lasts, float *logits, float *policy, float *value)
{
    if (!e || slot < 0 || slot > 1 || count < 0 || !boards || !players || !lasts) return fail(e, AZ_ERR_INVALID, "az_net_eval: bad argument");
    if (!e->net[slot].loaded) return fail(e, AZ_ERR_NO_WEIGHTS, "weights slot %d not loaded", slot);
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_net_eval: a self-play episode is open on this engine");
    DEVICE_GUARD(e);
    return eval_positions(e, "az_net_eval", slot, count, boards, players, lasts, logits, policy, value, nullptr, [&](LaunchCtx &lc, int cnt) {
        if (use_split(e, e->lanes[0], cnt)) e->ops->trunk_split(lc, slot); else e->ops->trunk(lc, slot);
    });
}

// ---- MCTS-Solver: proven wins, losses and draws in the search tree ----
// the root rows and root statuses of the first m slots of a lane, after a preset search, into e->proof_edges / proof_roots
// from position `at` on; boards = those positions' cells (an occupied cell reports 0)
static int fetch_proofs(az_engine *e, Lane &L, int m, const uint8_t *boards, size_t at)
{
    const size_t nn = (size_t)e->nn, pitch = (size_t)e->R * e->RW;
    if (e->proof_edges.size() < (at + m) * nn) { e->proof_edges.resize((at + m) * nn); e->proof_roots.resize(at + m); }
    HIPCHECK(e, az_memcpy2d(e->stream, e->proof_edges.data() + at * nn, nn, L.proof.p, pitch, nn, (size_t)m, hipMemcpyDeviceToHost));
    HIPCHECK(e, az_memcpy(e->stream, e->proof_roots.data() + at, L.root_proof.p, (size_t)m, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)m * nn; i++)
        if (boards[i]) e->proof_edges[at * nn + i] = 0;
    return AZ_OK;
}

extern "C" int az_set_solver(az_engine *e, int on)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_solver: an episode is open (az_selfplay_end first)");
    if (on != 0 && on != 1) return fail(e, AZ_ERR_INVALID, "az_set_solver: on %d (0 / 1)", on);
    if (!on) {
        if (e->threat_depth) return fail(e, AZ_ERR_INVALID, "az_set_solver: the threat search is on and needs the solver (az_set_threat_search(e, 0, 0) first)");
        e->solver = 0;
        e->proof_edges.clear(); e->proof_roots.clear();
        return AZ_OK;
    }
    if (refuse_conflicts(e, SET_SOLVER)) return AZ_ERR_INVALID;
    DEVICE_GUARD(e);
    // one status byte per edge beside every slot's tree
    size_t need = 0;
    for (Lane &L : e->lanes)
        if (!L.proof.p) need += (size_t)L.d.B * (size_t)e->R * (size_t)e->RW;
    if (need && e->deep) {
        int rc = deep_memory_guard("the edge statuses of the solver", need, e);
        if (rc) return rc;
    }
    const int rc = ensure_lane_buffers(e, {{&Lane::proof, (size_t)e->R * (size_t)e->RW, false}, {&Lane::root_proof, 1, false},
                                           {&Lane::proof_stops, sizeof(unsigned long long), false}});
    if (rc) return rc;
    for (Lane &L : e->lanes) {
        L.d.proof_buf = (unsigned char *)L.proof.p;
        L.d.root_proof = (signed char *)L.root_proof.p;
        L.d.proof_stops = (unsigned long long *)L.proof_stops.p;
    }
    each_state(e, [&](DevState &d) { (void)d; });        // refresh the item views
    e->solver = 1;
    return AZ_OK;
}

extern "C" int az_get_solver(const az_engine *e) { return e ? e->solver : AZ_ERR_INVALID; }

extern "C" int az_last_proof(az_engine *e, int capacity, int8_t *edges, int8_t *roots, int32_t *count)
{
    if (!e) return AZ_ERR_INVALID;
    if (!e->solver || e->proof_roots.empty()) return fail(e, AZ_ERR_STATE, "az_last_proof: no az_search / az_search_batch has run with the solver on");
    const int have = (int)e->proof_roots.size();
    if (count) *count = have;
    if ((edges || roots) && capacity < have)
        return fail(e, AZ_ERR_INVALID, "az_last_proof: the buffers hold %d positions, the last search had %d", capacity, have);
    if (edges) memcpy(edges, e->proof_edges.data(), (size_t)have * e->nn);
    if (roots) memcpy(roots, e->proof_roots.data(), (size_t)have);
    return AZ_OK;
}

extern "C" int az_solver_stops(const az_engine *e, int64_t *stops)
{
    if (!e || !stops) return AZ_ERR_INVALID;
    *stops = e->solver_stops;
    return AZ_OK;
}

// ---- delta evaluation (az_delta.h) ----
extern "C" int az_set_delta_eval(az_engine *e, int on)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_delta_eval: an episode is open");
    e->delta_on = on != 0;
    return AZ_OK;
}

extern "C" int az_get_delta_eval(const az_engine *e) { return e ? (e->delta_on ? 1 : 0) : AZ_ERR_INVALID; }

extern "C" int az_delta_max_tiles(az_engine *e, int tiles)
{
    if (!e) return AZ_ERR_INVALID;
    if (tiles == 0) return e->delta_tiles;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_delta_max_tiles: an episode is open");
    if (tiles < 1 || tiles > 15) return fail(e, AZ_ERR_INVALID, "az_delta_max_tiles: 1 .. 15 conv3 tiles, 0 asks");
    e->delta_tiles = tiles;
    return tiles;
}

extern "C" int az_delta_stats(const az_engine *e, int64_t *delta, int64_t *full, int64_t *tiles, int64_t *base, int64_t *by_tiles)
{
    if (!e) return AZ_ERR_INVALID;
    if (delta) *delta = e->delta_stats[0];
    if (full) *full = e->delta_stats[1];
    if (tiles) *tiles = e->delta_stats[2];
    if (base) *base = e->delta_stats[3];
    if (by_tiles) for (int t = 0; t < 16; t++) by_tiles[t] = e->delta_stats[4 + t];
    return AZ_OK;
}

// the tile lists of a set of changed cells at n = 15, with the functions the kernel uses (az_delta.h; no GPU needed)
extern "C" int az_delta_lists(int n, int count, const uint8_t *changed, uint16_t *wpos, uint16_t *cell, uint16_t *halo, int32_t *cnt)
{
    if (n != 15 || count < 0 || count > DELTA_MAX_CHANGED || (count && !changed) || !wpos || !cell || !halo || !cnt) return AZ_ERR_INVALID;
    for (int i = 0; i < count; i++) if (changed[i] >= 15 * 15) return AZ_ERR_INVALID;
    static DeltaLists<15> L;
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    memset(&L, 0xEE, sizeof L);          // whatever the function does not write reads as 0xEEEE
    delta_lists_serial<15>(changed, count, L);
    memcpy(wpos, L.wpos, sizeof L.wpos);
    memcpy(cell, L.cell, sizeof L.cell);
    memcpy(halo, L.halo, sizeof L.halo);
    for (int l = 0; l < 5; l++) cnt[l] = L.cnt[l];
    return AZ_OK;
}

// ... and of a position the delta kernel evaluates in full (delta_lists_full)
extern "C" int az_delta_lists_full(int n, uint16_t *wpos, uint16_t *cell, uint16_t *halo, int32_t *cnt)
{
    if (n != 15 || !wpos || !cell || !halo || !cnt) return AZ_ERR_INVALID;
    static DeltaLists<15> L;
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    memset(&L, 0xEE, sizeof L);
    delta_lists_full<15>(L);
    memcpy(wpos, L.wpos, sizeof L.wpos);
    memcpy(cell, L.cell, sizeof L.cell);
    memcpy(halo, L.halo, sizeof L.halo);
    for (int l = 0; l < 5; l++) cnt[l] = L.cnt[l];
    return AZ_OK;
}

// ... and the changed cells and the parity of a leaf against its root, with the function the kernel uses (delta_changed)
extern "C" int az_delta_changed(int n, const uint64_t *leaf, const uint64_t *board, int player, int last, uint8_t *changed,
                                int32_t *count, int32_t *parity)
{
    if (n != 15 || !leaf || !board || !changed || !count || !parity || (player != 1 && player != 2) || last < -1 || last >= 15 * 15)
        return AZ_ERR_INVALID;
    u64 lf[8], bd[8];
    for (int i = 0; i < 8; i++) { lf[i] = leaf[i]; bd[i] = board[i]; }
    int par = 0, cnt = 0;
    for (int k = 0; k < DELTA_MAX_CHANGED; k++) changed[k] = (uint8_t)delta_changed<15>(lf, bd, player, last, k, &cnt, &par);
    *count = cnt;
    *parity = par;
    return AZ_OK;
}

extern "C" int az_net_eval_delta(az_engine *e, int slot, const uint8_t *root, int root_player, int count, const uint8_t *boards,
                                 const uint8_t *players, const int16_t *lasts, float *logits, float *policy, float *value, int32_t *path)
{
    if (!e || slot < 0 || slot > 1 || count < 0 || !root || !boards || !players || !lasts || (root_player != 1 && root_player != 2))
        return fail(e, AZ_ERR_INVALID, "az_net_eval_delta: bad argument");
    if (!e->net[slot].loaded) return fail(e, AZ_ERR_NO_WEIGHTS, "weights slot %d not loaded", slot);
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_net_eval_delta: a self-play episode is open on this engine");
    if (!e->ops->trunk_delta || e->cfg.model != AZ_MODEL_PLAIN || e->cfg.eval_kind != AZ_EVAL_NET)
        return fail(e, AZ_ERR_INVALID, "az_net_eval_delta: no delta evaluation for this board size or net");
    DEVICE_GUARD(e);
    int rc = ensure_delta_buffers(e);
    if (rc) return rc;
    const Lane &L = e->lanes[0];
    const DeltaRoot dr{root, root_player, path};
    return eval_positions(e, "az_net_eval_delta", slot, count, boards, players, lasts, logits, policy, value, &dr, [&](LaunchCtx &lc, int) {
        lc.delta_base = (float *)L.delta_base.p;
        lc.delta_done = (unsigned char *)L.delta_done.p;
        lc.delta_cnt = (unsigned long long *)L.delta_cnt.p;
        lc.delta_tiles = e->delta_tiles;
        e->ops->trunk_base(lc, slot);
        e->ops->trunk_delta(lc, slot);
    });
}

extern "C" int az_selfplay_proofs(az_engine *e, int8_t *roots)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    if (!roots) return fail(e, AZ_ERR_INVALID, "az_selfplay_proofs: null buffer");
    if (!e->episode_solver || !e->rec_proof.p) return fail(e, AZ_ERR_STATE, "az_selfplay_proofs: the episode ran without the solver");
    DEVICE_GUARD(e);
    return read_record_array(e, e->rec_proof, roots);
}

// k_move's count vector N' of one root row of `count` legal children, with the function the kernel uses (az_tree.h)
extern "C" int az_solver_counts(int count, const int32_t *visits, const int8_t *status, int32_t *out)
{
    if (count < 1 || !visits || !status || !out) return AZ_ERR_INVALID;
    bool any_win = false, survivor = false;
    for (int c = 0; c < count; c++) {
        if (visits[c] < 0 || status[c] < 0 || status[c] > 3) return AZ_ERR_INVALID;
        any_win = any_win || status[c] == PROOF_WIN;
        survivor = survivor || (status[c] != PROOF_LOSS && visits[c] > 0);
    }
    for (int c = 0; c < count; c++) out[c] = solver_keeps(status[c], any_win, survivor) ? visits[c] : 0;
    return AZ_OK;
}

// ---- searches of given positions: MCTS.run for one position (az_search, az_search_callback) or every position of a list ----
// one given position, checked on the host; `who` names the entry point (and the position) in the error text
static int check_position(az_engine *e, const char *who, const uint8_t *bd, int player, int last, int *stones)
{
    const int nn = e->nn;
    if (player != 1 && player != 2) return fail(e, AZ_ERR_INVALID, "%s: player %d", who, player);
    int st = 0;
    for (int j = 0; j < nn; j++) {
        if (bd[j] > 2) return fail(e, AZ_ERR_INVALID, "%s: cell value %d", who, bd[j]);
        st += bd[j] != 0;
    }
    if (st >= nn) return fail(e, AZ_ERR_INVALID, "%s: no legal action", who);
    if (last >= nn || (last >= 0 && bd[last] == 0)) return fail(e, AZ_ERR_INVALID, "%s: bad last action", who);
    if (stones) *stones = st;
    return AZ_OK;
}

// Waves of at most `slots` positions; a wave is ONE ply of every lane (a one-ply episode whose game i is position i of the
// wave), so the searches of a wave share every evaluation batch.  Position i of the wave sits in slot i - first(l) of lane l.
static void add_counters(az_counters &t, const az_counters &c)
{
    t.games += c.games; t.plies += c.plies; t.records += c.records; t.simulations += c.simulations;
    t.expansions += c.expansions; t.root_evals += c.root_evals; t.terminal_hits += c.terminal_hits; t.depth_sum += c.depth_sum;
    t.steps += c.steps; t.seconds += c.seconds; t.nn_seconds += c.nn_seconds; t.trunk_seconds += c.trunk_seconds;
    t.trunk_launches += c.trunk_launches; t.trunk_boards += c.trunk_boards; t.step_seconds += c.step_seconds;
    t.duplicate_leaves += c.duplicate_leaves; t.cache_lookups += c.cache_lookups; t.cache_hits += c.cache_hits;
    t.tape_wait_seconds = std::max(t.tape_wait_seconds, c.tape_wait_seconds);
    t.tape_threads = c.tape_threads; t.host_cpus = c.host_cpus;
}

// A wave's m positions over the first K lanes: an even share each, what a lane cannot hold goes to the lanes with room.  Sets
// every Lane::preset_m; position i of the wave sits in slot i - first of its lane.
static BatchLanes spread_wave(az_engine *e, int K, int m)
{
    BatchLanes bl{};
    bl.K = K; bl.L = e->lanes[0].d.L;
    int left = m;
    for (int l = 0; l < K; l++) {
        Lane &L = e->lanes[l];
        L.preset_m = std::min(L.d.B, (left + (K - l) - 1) / (K - l));
        left -= L.preset_m;
    }
    for (int l = 0; l < K && left > 0; l++) {
        Lane &L = e->lanes[l];
        const int add = std::min(L.d.B - L.preset_m, left);
        L.preset_m += add; left -= add;
    }
    int first = 0;
    for (int l = 0; l < K; l++) {
        const Lane &L = e->lanes[l];
        BatchLane &b = bl.lane[l];
        b.board = L.d.board; b.s_game = L.d.s_game; b.s_ply = L.d.s_ply; b.s_player = L.d.s_player; b.s_last = L.d.s_last;
        b.s_status = L.d.s_status; b.leaf_kind = L.d.leaf_kind; b.carried = L.d.carried; b.edges = L.d.edges;
        b.B = L.d.B; b.first = first; b.m = L.preset_m;
        first += L.preset_m;
    }
    return bl;
}

// The search of `count` checked positions, arguments as az_search_batch.  batch: the positions go over every lane, the ply
// runs over the slots that hold one and the kernels are chosen for throughput, as in self-play (EpisodeSpec::batch); else
// they sit in the first slots of lane 0, whose ply runs over its whole grid (the captured graph) on the latency choices.
static int preset_search(az_engine *e, bool batch, int slot, int count, const uint8_t *boards, const uint8_t *players,
                         const int16_t *lasts, const double *temperatures, const double *noise, const double *u,
                         float *pi, int32_t *actions, int32_t *visits, double *W, float *prior)
{
    const int nn = e->nn, K = batch ? (int)e->lanes.size() : 1;
    if (!e->ext.on && e->cfg.eval_kind == AZ_EVAL_NET && !e->net[slot].loaded) return fail(e, AZ_ERR_NO_WEIGHTS, "weights slot %d not loaded", slot);
    if (K > BATCH_MAX_LANES) return fail(e, AZ_ERR_INVALID, "az_search_batch: more than %d lanes", BATCH_MAX_LANES);
    DEVICE_GUARD(e);
    e->proof_edges.clear(); e->proof_roots.clear();
    const int Wv = std::min(count, batch ? e->cfg.slots : e->lanes[0].d.B);     // positions per wave: everything below is sized by it, not by count
    int rc = ensure_episode_buffers(e, Wv, false);
    const size_t wn = (size_t)Wv * nn;
    if (!rc && noise) rc = dev_alloc(e, e->noise, wn * 8, false);
    if (!rc && !e->bt_zero_off.p) rc = dev_alloc(e, e->bt_zero_off, (size_t)(nn + 2) * sizeof(int), true);
    if (!rc) rc = dev_alloc(e, e->bt_cells, wn, false);
    if (!rc) rc = dev_alloc(e, e->bt_players, (size_t)Wv, false);
    if (!rc) rc = dev_alloc(e, e->bt_lasts, (size_t)Wv * 2, false);
    if (!rc) rc = dev_alloc(e, e->bt_T, (size_t)Wv * 8, false);
    if (!rc && visits) rc = dev_alloc(e, e->bt_visits, wn * 4, false);
    if (!rc && W) rc = dev_alloc(e, e->bt_W, wn * 8, false);
    if (!rc && prior) rc = dev_alloc(e, e->bt_prior, wn * 4, false);
    if (!rc && pi) rc = dev_alloc(e, e->bt_pi, wn * 4, false);
    if (!rc && actions) rc = dev_alloc(e, e->bt_action, (size_t)Wv * 4, false);
    if (rc) return rc;
    // The lanes' states for this call: per-position temperatures, key 0 for every position, and the compact noise rows.  The
    // baseline net (slot 1) searches as net 0 (the arena flag only selects the net through s_player) under its own cache
    // generation (the evaluation cache keys its entries by net id).  Everything is put back on every way out -- in the states
    // AND their item views, which az_net_eval goes by -- so that no other entry point ever sees these values.
    const PackedNet saved0 = e->net[0];
    const float *sv2w = e->lanes[0].d.v2w[0], *sv2b = e->lanes[0].d.v2b[0];
    struct Restore {
        az_engine *e; int slot; const PackedNet &saved0; const float *sv2w, *sv2b;
        ~Restore()
        {
            if (slot == 1) { e->net[0] = saved0; e->cache_gen ^= 0x80000000u; }
            each_state(e, [&](DevState &d) {
                d.T_game = nullptr; d.key_stride = 1; d.noise_off = (const int *)e->noise_off.p; d.noise_stride = e->tape_len;
                if (slot == 1) { d.v2w[0] = sv2w; d.v2b[0] = sv2b; d.cache_gen = e->cache_gen; }
            });
            for (Lane &L : e->lanes) L.preset_m = 0;
            e->have_episode = false;
        }
    } restore{e, slot, saved0, sv2w, sv2b};
    if (slot == 1) { e->net[0] = e->net[1]; e->cache_gen ^= 0x80000000u; }
    each_state(e, [&](DevState &d) {
        d.T_game = (const double *)e->bt_T.p; d.key_stride = 0; d.noise_off = (const int *)e->bt_zero_off.p;
        d.noise = (const double *)e->noise.p; d.noise_stride = nn;
        if (slot == 1) { d.v2w[0] = d.v2w[1]; d.v2b[0] = d.v2b[1]; }
    });
    EpisodeSpec sp;
    sp.max_plies = 0; sp.add_noise = noise != nullptr; sp.arena = false; sp.preset = true; sp.batch = batch; sp.profile = false;
    sp.ext_net = slot;
    az_counters total{};
    int64_t ext_requests = 0, ext_items = 0;       // az_ext_stats reports the whole call, like the counters
    int64_t batch_stops = 0;                       // ... and so does az_solver_stops
    int64_t batch_threat[THREAT_STATS] = {0, 0, 0, 0, 0};     // ... and az_threat_stats
    std::vector<double> hu(wn);
    for (int w0 = 0; w0 < count; w0 += Wv) {
        const int m = std::min(Wv, count - w0);
        const BatchLanes bl = spread_wave(e, K, m);
        // u is read at d.u[game * nn + ply]: scattered here, the other entries of the row are never read
        std::fill(hu.begin(), hu.begin() + (size_t)m * nn, 0.0);
        for (int i = 0; i < m; i++) {
            const uint8_t *bd = boards + (size_t)(w0 + i) * nn;
            int st = 0;
            for (int j = 0; j < nn; j++) st += bd[j] != 0;
            hu[(size_t)i * nn + st] = u[w0 + i];
        }
        HIPCHECK(e, hipMemcpyAsync(e->bt_cells.p, boards + (size_t)w0 * nn, (size_t)m * nn, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(e->bt_players.p, players + w0, (size_t)m, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(e->bt_lasts.p, lasts + w0, (size_t)m * 2, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(e->bt_T.p, temperatures + w0, (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(e->u.p, hu.data(), (size_t)m * nn * 8, hipMemcpyHostToDevice, e->stream));
        if (noise) HIPCHECK(e, hipMemcpyAsync(e->noise.p, noise + (size_t)w0 * nn, (size_t)m * nn * 8, hipMemcpyHostToDevice, e->stream));
        e->ops->set_positions(e->stream, bl, (const unsigned char *)e->bt_cells.p, (const unsigned char *)e->bt_players.p,
                              (const short *)e->bt_lasts.p);
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        HIPCHECK(e, hipGetLastError());
        sp.num_games = m;
        az_counters c{};
        if ((rc = run_episode(e, sp, &c))) return rc;
        add_counters(total, c);
        batch_stops += e->solver_stops;
        for (int i = 0; i < THREAT_STATS; i++) batch_threat[i] += e->threat_stats[i];
        ext_requests += e->ext.requests; ext_items += e->ext.items;
        // the lanes' streams are drained: every slot's root row and record into the compact staging, one copy per output
        e->ops->gather_roots(e->stream, bl, e->lanes[0].d, (const unsigned char *)e->bt_cells.p, visits ? (int *)e->bt_visits.p : nullptr, W ? (double *)e->bt_W.p : nullptr,
                             prior ? (float *)e->bt_prior.p : nullptr, pi ? (float *)e->bt_pi.p : nullptr,
                             actions ? (int *)e->bt_action.p : nullptr);
        if (e->solver) {
            int first = 0;
            for (Lane &L : e->lanes) {
                if (L.preset_m > 0 && (rc = fetch_proofs(e, L, L.preset_m, boards + (size_t)(w0 + first) * nn, (size_t)(w0 + first)))) return rc;
                first += L.preset_m;
            }
        }
        const size_t o = (size_t)w0 * nn, mn = (size_t)m * nn;
        if (visits) HIPCHECK(e, hipMemcpyAsync(visits + o, e->bt_visits.p, mn * 4, hipMemcpyDeviceToHost, e->stream));
        if (W) HIPCHECK(e, hipMemcpyAsync(W + o, e->bt_W.p, mn * 8, hipMemcpyDeviceToHost, e->stream));
        if (prior) HIPCHECK(e, hipMemcpyAsync(prior + o, e->bt_prior.p, mn * 4, hipMemcpyDeviceToHost, e->stream));
        if (pi) HIPCHECK(e, hipMemcpyAsync(pi + o, e->bt_pi.p, mn * 4, hipMemcpyDeviceToHost, e->stream));
        if (actions) HIPCHECK(e, hipMemcpyAsync(actions + w0, e->bt_action.p, (size_t)m * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        HIPCHECK(e, hipGetLastError());
    }
    e->last = total;
    e->solver_stops = batch_stops;
    for (int i = 0; i < THREAT_STATS; i++) e->threat_stats[i] = batch_threat[i];
    if (e->ext.on) { e->ext.requests = ext_requests; e->ext.items = ext_items; }
    return AZ_OK;
}

extern "C" int az_search_batch(az_engine *e, int slot, int count, const uint8_t *boards, const uint8_t *players,
                               const int16_t *lasts, const double *temperatures, const double *noise, const double *u,
                               float *pi, int32_t *actions, int32_t *visits, double *W, float *prior)
{
    if (!e || slot < 0 || slot > 1 || count < 0) return fail(e, AZ_ERR_INVALID, "az_search_batch: bad argument");
    if (count == 0) return AZ_OK;
    if (!boards || !players || !lasts || !temperatures || !u) return fail(e, AZ_ERR_INVALID, "az_search_batch: null argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_search_batch: a self-play episode is open on this engine");
    // every position is checked on the host before any GPU work: an error leaves every output untouched
    for (int i = 0; i < count; i++) {
        char who[48];
        snprintf(who, sizeof who, "az_search_batch: position %d", i);
        if (check_position(e, who, boards + (size_t)i * e->nn, players[i], lasts[i], nullptr)) return AZ_ERR_INVALID;
    }
    return preset_search(e, true, slot, count, boards, players, lasts, temperatures, noise, u, pi, actions, visits, W, prior);
}

// one position: a batch of one on lane 0.  The single noise row, temperature and u address the same values as the tapes of a
// one-game episode would, so the search is the one az_search_batch makes of the position, bit for bit.
static int search_one(az_engine *e, int slot, const uint8_t *board, int player, int last, int stones, double temperature,
                      const double *noise, double u, float *pi, int32_t *action, int32_t *visits, double *W, float *prior)
{
    const uint8_t pl = (uint8_t)player;
    const int16_t la = (int16_t)std::max(last, (int)INT16_MIN);     // the kernels tell negative values apart (the symmetry hash)
    std::vector<double> row;                                        // one entry per legal cell -> the [n*n] row of the batch
    if (noise) { row.assign(e->nn, 0.0); memcpy(row.data(), noise, (size_t)(e->nn - stones) * 8); }
    return preset_search(e, false, slot, 1, board, &pl, &la, &temperature, noise ? row.data() : nullptr, &u, pi, action, visits, W, prior);
}

extern "C" int az_search(az_engine *e, int slot, const uint8_t *board, int player, int last, double temperature,
                         const double *noise, double u, float *pi, int32_t *action, int32_t *visits, double *W,
                         float *prior)
{
    if (!e || !board || (player != 1 && player != 2) || slot < 0 || slot > 1) return fail(e, AZ_ERR_INVALID, "az_search: bad argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_search: a self-play episode is open on this engine");
    int stones = 0;
    if (check_position(e, "az_search", board, player, last, &stones)) return AZ_ERR_INVALID;
    return search_one(e, slot, board, player, last, stones, temperature, noise, u, pi, action, visits, W, prior);
}

// ---- the win rule: which game is played ----
static_assert(AZ_RULE_FREESTYLE == WIN_RULE_FREESTYLE && AZ_RULE_EXACT == WIN_RULE_EXACT, "the kernels' rule values are the C-ABI's");

// Full-board scan (no engine, no GPU): every maximal run of either colour in the four directions, counted from its first
// stone, is held against the rule (run_wins, the compare of the kernels' win test).
extern "C" int az_rules_winner(const uint8_t *board, int n, int k, int rule)
{
    if (!board || n < 1 || n > 15 || k < 1 || k > n || (rule != AZ_RULE_FREESTYLE && rule != AZ_RULE_EXACT)) return AZ_ERR_INVALID;
    static const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
    bool won[3] = {false, false, false};
    int stones = 0;
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) {
            const int v = board[r * n + c];
            if (v > 2) return AZ_ERR_INVALID;
            if (!v) continue;
            stones++;
            for (int t = 0; t < 4; t++) {
                const int pr = r - dr[t], pc = c - dc[t];
                if (pr >= 0 && pr < n && pc >= 0 && pc < n && board[pr * n + pc] == v) continue;     // not the first stone of its run
                int len = 1;
                for (int rr = r + dr[t], cc = c + dc[t]; rr >= 0 && rr < n && cc >= 0 && cc < n && board[rr * n + cc] == v; rr += dr[t], cc += dc[t]) len++;
                if (run_wins(len, k, rule)) won[v] = true;
            }
        }
    if (won[1] && won[2]) return AZ_ERR_INVALID;
    if (won[1]) return AZ_RES_X;
    if (won[2]) return AZ_RES_O;
    return stones == n * n ? AZ_RES_DRAW : AZ_RES_NONE;
}

static const char *win_rule_name(int rule) { return rule == AZ_RULE_EXACT ? "exact" : "freestyle"; }

extern "C" int az_set_win_rule(az_engine *e, int rule)
{
    if (!e) return AZ_ERR_INVALID;
    if (rule != AZ_RULE_FREESTYLE && rule != AZ_RULE_EXACT) return fail(e, AZ_ERR_INVALID, "az_set_win_rule: rule %d (0 = freestyle, 1 = exact)", rule);
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_win_rule: an episode is open (az_selfplay_end first)");
    if (e->start_count > 0 && rule != e->win_rule)
        return fail(e, AZ_ERR_STATE, "az_set_win_rule: %d start positions are set, validated under the %s rule (clear them, set the rule, set them again)",
                    e->start_count, win_rule_name(e->win_rule));
    e->win_rule = rule;
    each_state(e, [&](DevState &d) { d.rule = rule; });     // part of every launch's arguments: a captured ply graph is re-captured
    return AZ_OK;
}

extern "C" int az_get_win_rule(const az_engine *e) { return e ? e->win_rule : AZ_ERR_INVALID; }

// ---- start positions: later self-play and arena games continue these instead of beginning on the empty board ----
// A winning run of either colour anywhere on the board, under the engine's rule: the kernels test only lines through the last
// stone (wins_through) and the reference's winner is sticky (games.py:140-141), so such a position would be played on.
// Under AZ_RULE_EXACT a position that holds only overlines has no winner and is a legal start.
static bool has_line(const uint8_t *bd, int n, int k, int rule)
{
    const int w = az_rules_winner(bd, n, k, rule);
    return w == AZ_RES_X || w == AZ_RES_O || w == AZ_ERR_INVALID;
}

extern "C" int az_set_start_positions(az_engine *e, int count, const uint8_t *boards, const uint8_t *players,
                                      const int16_t *lasts, int64_t first)
{
    if (!e || count < 0 || count > (1 << 24) || first < 0) return fail(e, AZ_ERR_INVALID, "az_set_start_positions: bad argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_start_positions: an episode is open");
    if (count == 0) {
        e->start_count = e->start_first = e->start_max_ply = 0;
        e->start_ply.clear();
        return AZ_OK;
    }
    if (!boards || !players || !lasts) return fail(e, AZ_ERR_INVALID, "az_set_start_positions: null argument");
    const int nn = e->nn;
    // every position is checked on the host before anything is uploaded, by az_search_batch's rules and the line test
    std::vector<int> ply(count);
    int max_ply = 0;
    for (int i = 0; i < count; i++) {
        const uint8_t *bd = boards + (size_t)i * nn;
        if (players[i] != 1 && players[i] != 2) return fail(e, AZ_ERR_INVALID, "az_set_start_positions: position %d: player %d", i, players[i]);
        int st = 0;
        for (int j = 0; j < nn; j++) {
            if (bd[j] > 2) return fail(e, AZ_ERR_INVALID, "az_set_start_positions: position %d: cell value %d", i, bd[j]);
            st += bd[j] != 0;
        }
        if (st >= nn) return fail(e, AZ_ERR_INVALID, "az_set_start_positions: position %d: no legal action", i);
        if (lasts[i] >= nn || lasts[i] < -1 || (lasts[i] >= 0 && bd[lasts[i]] == 0)) return fail(e, AZ_ERR_INVALID, "az_set_start_positions: position %d: bad last action", i);
        if (has_line(bd, e->n, e->cfg.win_length, e->win_rule))
            return fail(e, AZ_ERR_INVALID, "az_set_start_positions: position %d: already won (a line of %s%d under the %s rule)", i,
                        e->win_rule == AZ_RULE_EXACT ? "exactly " : "", e->cfg.win_length, win_rule_name(e->win_rule));
        ply[i] = st;
        max_ply = std::max(max_ply, st);
    }
    DEVICE_GUARD(e);
    // a new table beside the one in force: any failure below keeps the previous setting
    DevBuf tab, cells, pl, la;
    int rc = dev_alloc(e, tab, (size_t)count * sizeof(StartPos), false);
    if (!rc) rc = dev_alloc(e, cells, (size_t)count * nn, false);
    if (!rc) rc = dev_alloc(e, pl, (size_t)count, false);
    if (!rc) rc = dev_alloc(e, la, (size_t)count * 2, false);
    if (!rc) {
        hipError_t hr = hipMemcpyAsync(cells.p, boards, (size_t)count * nn, hipMemcpyHostToDevice, e->stream);
        if (hr == hipSuccess) hr = hipMemcpyAsync(pl.p, players, (size_t)count, hipMemcpyHostToDevice, e->stream);
        if (hr == hipSuccess) hr = hipMemcpyAsync(la.p, lasts, (size_t)count * 2, hipMemcpyHostToDevice, e->stream);
        if (hr == hipSuccess) {
            e->ops->build_positions(e->stream, count, (const unsigned char *)cells.p, (const unsigned char *)pl.p, (const short *)la.p, (StartPos *)tab.p);
            hr = hipStreamSynchronize(e->stream);
        }
        if (hr == hipSuccess) hr = hipGetLastError();
        if (hr != hipSuccess) rc = fail(e, AZ_ERR_HIP, "az_set_start_positions: %s", hipGetErrorString(hr));
    }
    dev_free(cells); dev_free(pl); dev_free(la);
    if (rc) { dev_free(tab); return rc; }
    dev_free(e->start_tab);
    e->start_tab = tab;
    e->start_count = count;
    e->start_first = (int)(first % (2 * (int64_t)count));
    e->start_max_ply = max_ply;
    e->start_ply.swap(ply);
    return AZ_OK;
}

extern "C" int az_get_start_positions(const az_engine *e) { return e ? e->start_count : AZ_ERR_INVALID; }

// ---- root threat search: forced-four wins and forced blocks, proven exactly (csrc/az_threat.h) ----
static_assert(AZ_THREAT_MAX_DEPTH == THREAT_MAX_DEPTH, "the kernel's stack holds the C-ABI's depth");

extern "C" int az_set_threat_search(az_engine *e, int max_depth, int node_budget)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_threat_search: an episode is open (az_selfplay_end first)");
    if (max_depth == 0) {
        e->threat_depth = e->threat_budget = 0;
        return AZ_OK;
    }
    if (max_depth < 1 || max_depth > AZ_THREAT_MAX_DEPTH || node_budget < 1 || node_budget > 65535)
        return fail(e, AZ_ERR_INVALID, "az_set_threat_search: max_depth %d (0 = off, 1 .. %d), node_budget %d (1 .. 65535)", max_depth,
                    AZ_THREAT_MAX_DEPTH, node_budget);
    if (!e->solver) return fail(e, AZ_ERR_INVALID, "az_set_threat_search: the threat search hands its results to the solver (az_set_solver(e, 1) first)");
    DEVICE_GUARD(e);
    const int rc = ensure_threat_buffers(e);
    if (rc) return rc;
    e->threat_depth = max_depth;
    e->threat_budget = node_budget;
    return AZ_OK;
}

extern "C" int az_get_threat_search(const az_engine *e, int *max_depth, int *node_budget)
{
    if (!e) return AZ_ERR_INVALID;
    if (max_depth) *max_depth = e->threat_depth;
    if (node_budget) *node_budget = e->threat_budget;
    return AZ_OK;
}

extern "C" int az_threat_solve(const uint8_t *board, int n, int k, int rule, int player, int max_depth, int node_budget,
                               int32_t *move, int32_t *depth, int32_t *nodes, int8_t *edges)
{
    if (!board || n < 1 || n > 15 || k < 1 || k > n || (rule != AZ_RULE_FREESTYLE && rule != AZ_RULE_EXACT) || (player != 1 && player != 2) ||
        max_depth < 1 || max_depth > AZ_THREAT_MAX_DEPTH || node_budget < 1 || node_budget > 65535)
        return AZ_ERR_INVALID;
    int stones = 0;
    for (int j = 0; j < n * n; j++) {
        if (board[j] > 2) return AZ_ERR_INVALID;
        stones += board[j] != 0;
    }
    if (stones >= n * n || az_rules_winner(board, n, k, rule) != AZ_RES_NONE) return AZ_ERR_INVALID;     // no legal action, or already won
    int mv = -1, dp = 0, nd = 0;
    const int root = threat_solve_host(board, n, k, rule, player, max_depth, node_budget, &mv, &dp, &nd, (signed char *)edges);
    if (move) *move = mv;
    if (depth) *depth = dp;
    if (nodes) *nodes = nd;
    return root;
}

extern "C" int az_threat_batch(az_engine *e, int count, const uint8_t *boards, const uint8_t *players, int max_depth, int node_budget,
                               int8_t *status, int32_t *move, int32_t *depth, int32_t *nodes, int8_t *edges)
{
    if (!e || count < 0) return fail(e, AZ_ERR_INVALID, "az_threat_batch: bad argument");
    if (max_depth < 1 || max_depth > AZ_THREAT_MAX_DEPTH || node_budget < 1 || node_budget > 65535)
        return fail(e, AZ_ERR_INVALID, "az_threat_batch: max_depth %d (1 .. %d), node_budget %d (1 .. 65535)", max_depth, AZ_THREAT_MAX_DEPTH, node_budget);
    if (count == 0) return AZ_OK;
    if (!boards || !players) return fail(e, AZ_ERR_INVALID, "az_threat_batch: null argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_threat_batch: a self-play episode is open on this engine");
    const int nn = e->nn, K = (int)e->lanes.size();
    if (K > BATCH_MAX_LANES) return fail(e, AZ_ERR_INVALID, "az_threat_batch: more than %d lanes", BATCH_MAX_LANES);
    // every position is checked on the host before any GPU work: an error leaves every output untouched
    for (int i = 0; i < count; i++) {
        char who[48];
        snprintf(who, sizeof who, "az_threat_batch: position %d", i);
        const uint8_t *bd = boards + (size_t)i * nn;
        if (check_position(e, who, bd, players[i], -1, nullptr)) return AZ_ERR_INVALID;
        if (has_line(bd, e->n, e->cfg.win_length, e->win_rule))
            return fail(e, AZ_ERR_INVALID, "az_threat_batch: position %d: already won (a line of %s%d under the %s rule)", i,
                        e->win_rule == AZ_RULE_EXACT ? "exactly " : "", e->cfg.win_length, win_rule_name(e->win_rule));
    }
    DEVICE_GUARD(e);
    const int Wv = std::min(count, e->cfg.slots);
    int rc = ensure_threat_buffers(e);
    if (!rc) rc = dev_alloc(e, e->bt_cells, (size_t)Wv * nn, false);
    if (!rc) rc = dev_alloc(e, e->bt_players, (size_t)Wv, false);
    if (!rc) rc = dev_alloc(e, e->bt_lasts, (size_t)Wv * 2, false);
    if (rc) return rc;
    IdleLanes idle{e, K};
    const std::vector<int16_t> no_last((size_t)Wv, (int16_t)-1);
    HIPCHECK(e, hipMemcpyAsync(e->bt_lasts.p, no_last.data(), (size_t)Wv * 2, hipMemcpyHostToDevice, e->stream));
    std::vector<int8_t> h8;
    std::vector<int16_t> h16;
    for (int w0 = 0; w0 < count; w0 += Wv) {
        const int m = std::min(Wv, count - w0);
        const BatchLanes bl = spread_wave(e, K, m);
        HIPCHECK(e, hipMemcpyAsync(e->bt_cells.p, boards + (size_t)w0 * nn, (size_t)m * nn, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(e->bt_players.p, players + w0, (size_t)m, hipMemcpyHostToDevice, e->stream));
        e->ops->set_positions(e->stream, bl, (const unsigned char *)e->bt_cells.p, (const unsigned char *)e->bt_players.p,
                              (const short *)e->bt_lasts.p);
        for (Lane &L : e->lanes) {
            if (L.preset_m == 0) continue;
            LaunchCtx lc = ctx_of_impl(e, L);
            lc.stream = e->stream;
            set_threat_state(lc.d, &L, max_depth, node_budget);
            lc.d.rule = e->win_rule;
            lc.d.B = L.preset_m;
            e->ops->threat(lc);
        }
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        HIPCHECK(e, hipGetLastError());
        int first = 0;
        for (Lane &L : e->lanes) {
            const size_t pm = (size_t)L.preset_m, at = (size_t)(w0 + first);
            first += L.preset_m;
            if (pm == 0) continue;
            if (status) HIPCHECK(e, az_memcpy(e->stream, status + at, L.threat_root.p, pm, hipMemcpyDeviceToHost));
            if (depth) {
                h8.resize(pm);
                HIPCHECK(e, az_memcpy(e->stream, h8.data(), L.threat_depth.p, pm, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < pm; i++) depth[at + i] = h8[i];
            }
            if (move) {
                h16.resize(pm);
                HIPCHECK(e, az_memcpy(e->stream, h16.data(), L.threat_move.p, pm * 2, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < pm; i++) move[at + i] = h16[i];
            }
            if (nodes) HIPCHECK(e, az_memcpy(e->stream, nodes + at, L.threat_nodes.p, pm * 4, hipMemcpyDeviceToHost));
            if (edges) HIPCHECK(e, az_memcpy2d(e->stream, edges + at * nn, (size_t)nn, L.threat_edges.p, (size_t)e->RW, (size_t)nn, pm, hipMemcpyDeviceToHost));
        }
    }
    return AZ_OK;
}

extern "C" int az_selfplay_threats(az_engine *e, int8_t *depth)
{
    if (!e || !e->have_episode) return fail(e, AZ_ERR_STATE, "no episode has been run");
    if (!depth) return fail(e, AZ_ERR_INVALID, "az_selfplay_threats: null buffer");
    if (!e->episode_threat || !e->rec_threat.p) return fail(e, AZ_ERR_STATE, "az_selfplay_threats: the episode ran without the threat search");
    DEVICE_GUARD(e);
    return read_record_array(e, e->rec_threat, depth);
}

extern "C" int az_threat_stats(az_engine *e, int64_t *win_roots, int64_t *lost_roots, int64_t *block_roots, int64_t *exhausted, int64_t *nodes)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open && e->episode_threat) {       // the open episode so far
        DEVICE_GUARD(e);
        az_counters c = e->run.c;
        const int rc = read_counters(e, c);
        if (rc) return rc;
    }
    int64_t *out[THREAT_STATS] = {win_roots, lost_roots, block_roots, exhausted, nodes};
    for (int i = 0; i < THREAT_STATS; i++)
        if (out[i]) *out[i] = e->threat_stats[i];
    return AZ_OK;
}

extern "C" int az_arena(az_engine *e, const az_arena_args *a, az_arena_result *out, int32_t *results, int16_t *actions,
                        int32_t *nply)
{
    if (!e || !a || a->num_games < 1) return fail(e, AZ_ERR_INVALID, "az_arena: bad argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_arena: a self-play episode is open on this engine");
    DEVICE_GUARD(e);
    const int nn = e->nn, G = a->num_games;
    int rc = ensure_episode_buffers(e, G, false);
    if (rc) return rc;
    if ((rc = upload_T(e, a->temperature_table, true))) return rc;
    if (!a->u_tape && e->rng_mode == AZ_RNG_PHILOX) {
        // the move uniforms of the same stream as self-play's, and no noise
        HIPCHECK(e, az_tape_launch(e->stream, a->seed0, G, nn, 0, nn, 1.0, AZ_TAPE_DIRICHLET, nullptr, nullptr, 0, (double *)e->u.p));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
    } else {
        std::vector<double> hu((size_t)G * nn);
        if (a->u_tape) memcpy(hu.data(), a->u_tape, hu.size() * 8);
        else for (int g = 0; g < G; g++) azrng::uniforms(a->seed0 + (uint64_t)g, nn, hu.data() + (size_t)g * nn);
        HIPCHECK(e, az_memcpy(e->stream, e->u.p, hu.data(), hu.size() * 8, hipMemcpyHostToDevice));
    }
    EpisodeSpec sp;
    sp.num_games = G; sp.max_plies = 0; sp.add_noise = false; sp.arena = true;
    sp.game_key0 = (unsigned)a->seed0;
    az_counters c;
    if ((rc = run_episode(e, sp, &c))) return rc;
    int w = 0, l = 0, dr = 0;
    for (int g = 0; g < G; g++) {
        int r = e->h_result[g];
        w += r == AZ_RES_X; l += r == AZ_RES_O; dr += r == AZ_RES_DRAW;   // candidate = X, baseline = O (evaluator.py:64)
        if (results) results[g] = r;
        if (nply) nply[g] = e->h_nply[g];
    }
    if (actions) {
        std::vector<short> ac((size_t)G * nn);
        HIPCHECK(e, az_memcpy(e->stream, ac.data(), e->rec_action.p, ac.size() * 2, hipMemcpyDeviceToHost));
        std::fill(actions, actions + (size_t)G * nn, (int16_t)-1);     // a row per game, from the ply it started at
        for_each_record(e, [&](int g, int, size_t si, size_t) { actions[si - e->h_start[g]] = ac[si]; });
    }
    if (out) {
        out->wins = w; out->losses = l; out->draws = dr; out->total = w + l + dr;
        out->win_rate = out->total ? (w + 0.5 * dr) / out->total : 0.0;     // evaluator.py:106-109
    }
    return AZ_OK;
}

extern "C" int az_rules_replay(az_engine *e, int games, int max_len, const int16_t *actions, uint8_t *term_before,
                               uint8_t *boards, int32_t *players, int32_t *results, int32_t *first_illegal)
{
    if (!e || games < 0 || max_len < 0 || !actions || !boards || !players || !results || !first_illegal)
        return fail(e, AZ_ERR_INVALID, "az_rules_replay: bad argument");
    if (games == 0) return AZ_OK;
    DEVICE_GUARD(e);
    const size_t G = (size_t)games, L = (size_t)(max_len > 0 ? max_len : 1), nn = (size_t)e->nn;
    DevBuf da, dt, db, dp, dr, ds;
    int rc = dev_alloc(e, da, G * L * 2, true);
    if (!rc) rc = dev_alloc(e, dt, G * L, true);
    if (!rc) rc = dev_alloc(e, db, G * nn, false);
    if (!rc) rc = dev_alloc(e, dp, G * 4, false);
    if (!rc) rc = dev_alloc(e, dr, G * 4, false);
    if (!rc) rc = dev_alloc(e, ds, G * 4, false);
    hipError_t hr = hipSuccess;
    if (!rc) {
        if (max_len > 0) hr = az_memcpy(e->stream, da.p, actions, G * L * 2, hipMemcpyHostToDevice);
        else hr = hipMemsetAsync(da.p, 0xFF, G * L * 2, e->stream);
        if (hr == hipSuccess) {
            hipLaunchKernelGGL(k_rules_replay, dim3((games + 63) / 64), dim3(64), 0, e->stream, e->n, e->cfg.win_length, e->win_rule, games,
                               (int)L, (const short *)da.p, term_before ? (unsigned char *)dt.p : nullptr, (unsigned char *)db.p,
                               (int *)dp.p, (int *)dr.p, (int *)ds.p);
            hr = hipStreamSynchronize(e->stream);
        }
        if (hr == hipSuccess) hr = hipGetLastError();
        if (hr == hipSuccess && term_before && max_len > 0) hr = az_memcpy(e->stream, term_before, dt.p, G * L, hipMemcpyDeviceToHost);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, boards, db.p, G * nn, hipMemcpyDeviceToHost);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, players, dp.p, G * 4, hipMemcpyDeviceToHost);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, results, dr.p, G * 4, hipMemcpyDeviceToHost);
        if (hr == hipSuccess) hr = az_memcpy(e->stream, first_illegal, ds.p, G * 4, hipMemcpyDeviceToHost);
        if (hr != hipSuccess) rc = fail(e, AZ_ERR_HIP, "az_rules_replay: %s", hipGetErrorString(hr));
    }
    dev_free(da); dev_free(dt); dev_free(db); dev_free(dp); dev_free(dr); dev_free(ds);
    return rc;
}

// diagnostic builds (-DAZ_STAMPS): per-workgroup phase stamps of the last k_trunk or k_trunk_delta launch (az_delta.h, AZ_DSTAMP:
// other slots), 16 u64 per workgroup
extern "C" int az_debug_stamps(az_engine *e, unsigned long long *out, int max_groups)
{
    if (!e || !out || !e->lanes[0].dbg.p) return AZ_ERR_STATE;
    DevBuf &dbg = e->lanes[0].dbg;
    size_t n = std::min<size_t>((size_t)max_groups * 16, dbg.bytes / 8);
    if (max_groups < 0) n = dbg.bytes / 8;   // everything (trunk stamps, then k_fc stamps at offset B*16)
    HIPCHECK(e, az_memcpy(e->stream, out, dbg.p, n * 8, hipMemcpyDeviceToHost));
    return AZ_OK;
}

extern "C" int az_examples_gather(az_engine *e, const void *packed_dev, const int64_t *idx_dev, const int32_t *sym_dev,
                                  int count, int reference_pi, float *states_dev, float *pis_dev, float *z_dev)
{
    if (!e || count < 0) return fail(e, AZ_ERR_INVALID, "az_examples_gather: bad argument");
    if (count == 0) return AZ_OK;           // nothing to read or write: the buffers of an empty batch may be null
    if (!packed_dev || !idx_dev || !sym_dev || !states_dev || !pis_dev || !z_dev)
        return fail(e, AZ_ERR_INVALID, "az_examples_gather: bad argument");
    DEVICE_GUARD(e);
    hipLaunchKernelGGL(k_examples_gather, dim3((unsigned)count), dim3(256), 0, e->stream, (const unsigned char *)packed_dev,
                       (const long long *)idx_dev, (const int *)sym_dev, count, e->n, record_bytes(e->nn), reference_pi,
                       states_dev, pis_dev, z_dev);
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    HIPCHECK(e, hipGetLastError());
    return AZ_OK;
}

extern "C" int az_set_subtree_reuse(az_engine *e, int on)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_subtree_reuse: an episode is open");
    if (on && refuse_conflicts(e, SET_REUSE)) return AZ_ERR_INVALID;
    if (on && e->R > REUSE_MAX_ROWS)
        return fail(e, AZ_ERR_INVALID, "subtree reuse supports at most %d simulations per move", REUSE_MAX_ROWS - 1);
    e->reuse = on ? 1 : 0;
    return AZ_OK;
}

extern "C" int az_set_profiling(az_engine *e, int on)
{
    if (!e) return AZ_ERR_INVALID;
    e->profile = on != 0;
    return AZ_OK;
}

extern "C" int az_get_counters(const az_engine *e, az_counters *out)
{
    if (!e || !out) return AZ_ERR_INVALID;
    *out = e->last;
    return AZ_OK;
}

extern "C" int az_get_lanes(const az_engine *e) { return e ? (int)e->lanes.size() : AZ_ERR_INVALID; }

extern "C" int az_set_virtual_loss(az_engine *e, int leaves)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_virtual_loss: an episode is open");
    if (leaves < 1 || leaves > VL_MAX) return fail(e, AZ_ERR_INVALID, "virtual-loss batching supports 1..%d leaves per batch", VL_MAX);
    const char *f = getenv("AZ_VL_FORCE");       // AZ_VL_FORCE=1: the batched kernel also for batches of one (must equal k_step)
    const bool vl_kernel = leaves > 1 || (f && f[0] == '1');
    if (leaves > 1 && refuse_conflicts(e, SET_VL)) return AZ_ERR_INVALID;
    if (vl_kernel && refuse_conflicts(e, SET_VL_KERNEL)) return AZ_ERR_INVALID;
    DEVICE_GUARD(e);
    // deep search (S > DEFAULT_MAX_S) with batches: the in-flight counts live beside the tree, one byte per edge
    const bool need_inflight = e->deep && e->cfg.num_simulations > DEFAULT_MAX_S && leaves > 1;
    if (need_inflight) {
        size_t need = 0;
        for (Lane &L : e->lanes)
            if (!L.inflight.p) need += (size_t)L.d.B * (size_t)e->R * (size_t)e->RW;
        if (need) {
            int rc = deep_memory_guard("the in-flight counts of virtual-loss batching", need, e);
            if (rc) return rc;
        }
        for (Lane &L : e->lanes) {
            int rc = dev_alloc(e, L.inflight, (size_t)L.d.B * (size_t)e->R * (size_t)e->RW);
            if (rc) return rc;
        }
    } else {
        for (Lane &L : e->lanes) dev_free(L.inflight);
    }
    if (leaves != e->vl) {
        for (Lane &L : e->lanes) {
            int rc = alloc_items(e, L, leaves);
            if (rc) return rc;
            for (int i = 0; i < 4; i++)       // the captured plies bake the old buffers in
                if (L.graph[i >> 1][i & 1].exec) { (void)hipGraphExecDestroy(L.graph[i >> 1][i & 1].exec); L.graph[i >> 1][i & 1].exec = nullptr; }
        }
        HIPCHECK(e, hipStreamSynchronize(e->stream));
    }
    e->vl = leaves;
    e->vl_kernel = vl_kernel;
    each_state(e, [&](DevState &d) { (void)d; });        // refresh the item views
    return AZ_OK;
}

extern "C" int az_set_eval_cache(az_engine *e, int64_t entries)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_eval_cache: an episode is open");
    if (entries < 0 || entries > ((int64_t)1 << 26)) return fail(e, AZ_ERR_INVALID, "cache entries must be 0 (off) .. 2^26");
    DEVICE_GUARD(e);
    if (entries == 0) {
        dev_free(e->cache);
        e->cache_mask = 0;
    } else {
        int64_t n = 1024;
        while (n < entries) n <<= 1;
        const size_t ces = (size_t)(32 + e->RW + 64) * sizeof(float);       // CacheGeo<n>::CES floats per entry
        dev_free(e->cache);
        int rc = dev_alloc(e, e->cache, (size_t)n * ces, true);
        if (rc) return rc;
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        e->cache_mask = (unsigned)(n - 1);
    }
    e->cache_gen++;
    each_state(e, [&](DevState &d) { d.cache = (float *)e->cache.p; d.cache_mask = e->cache_mask; d.cache_gen = e->cache_gen; });
    return AZ_OK;
}

extern "C" int az_set_leaf_symmetry(az_engine *e, int on)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_leaf_symmetry: an episode is open");
    if (on && refuse_conflicts(e, SET_SYMMETRY)) return AZ_ERR_INVALID;
    e->leaf_symmetry = on ? 1 : 0;
    for (Lane &L : e->lanes) L.d.leaf_sym = on ? (int *)L.leaf_sym.p : nullptr;
    each_state(e, [&](DevState &d) { (void)d; });        // refresh the item views
    return AZ_OK;
}

extern "C" int az_set_trunk_mode(az_engine *e, int mode)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_trunk_mode: an episode is open");
    if (mode != AZ_TRUNK_F32 && mode != AZ_TRUNK_BF16X3 && mode != AZ_TRUNK_F16X2) return fail(e, AZ_ERR_INVALID, "az_set_trunk_mode: unknown mode %d", mode);
    if (mode == AZ_TRUNK_F16X2)
        for (int i = 0; i < 2; i++)
            if (e->net[i].loaded && !e->net[i].f16_ok)
                return fail(e, AZ_ERR_INVALID, "az_set_trunk_mode: weight slot %d holds a value outside float16's range (|w| >= 65504): use AZ_TRUNK_BF16X3", i);
    if (mode != AZ_TRUNK_F32) {
        DEVICE_GUARD(e);
        for (int i = 0; i < 2; i++) {
            const int rc = ensure_emul(e, i, mode);
            if (rc) return rc;
        }
    }
    if (mode != e->trunk_mode) {
        e->trunk_mode = mode;
        e->cache_gen++;           // cached evaluations of the other arithmetic never match again
        each_state(e, [&](DevState &d) { d.cache_gen = e->cache_gen; });
    }
    return AZ_OK;
}

extern "C" int az_get_trunk_mode(const az_engine *e) { return e ? e->trunk_mode : AZ_ERR_INVALID; }

extern "C" int az_emul_split(int mode, float x, uint16_t *parts)
{
    if (!parts || (mode != AZ_TRUNK_BF16X3 && mode != AZ_TRUNK_F16X2)) return AZ_ERR_INVALID;
    return emul_split(mode, x, parts) ? emul_parts(mode) : AZ_ERR_INVALID;
}

extern "C" int az_get_persistent(const az_engine *e) { return e ? e->persist_gp : AZ_ERR_INVALID; }

// ---- batched external evaluator ----
extern "C" int az_ext_capacity(const az_engine *e) { return e ? e->cfg.slots * e->vl : AZ_ERR_INVALID; }

extern "C" int az_get_external_evaluator(const az_engine *e) { return e ? (e->ext.on ? 1 : 0) : AZ_ERR_INVALID; }

extern "C" int az_set_external_evaluator(az_engine *e, const az_ext_evaluator *ev)
{
    if (!e) return AZ_ERR_INVALID;
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_set_external_evaluator: an episode is open");
    if (!ev) {
        e->ext.on = false;
        e->ext.ev = az_ext_evaluator{};
        return AZ_OK;
    }
    if (!ev->planes_dev || !ev->policy_dev || !ev->value_dev || !ev->fn)
        return fail(e, AZ_ERR_INVALID, "az_set_external_evaluator: null buffer or callback");
    if ((uintptr_t)ev->planes_dev & 15u) return fail(e, AZ_ERR_INVALID, "az_set_external_evaluator: planes_dev must be 16-byte aligned");
    if (refuse_conflicts(e, SET_EXT)) return AZ_ERR_INVALID;
    if (ev->capacity < e->cfg.slots * e->vl)
        return fail(e, AZ_ERR_INVALID, "az_set_external_evaluator: capacity %d is below az_ext_capacity = %d slots x %d leaves per batch",
                    ev->capacity, e->cfg.slots, e->vl);
    e->ext.ev = *ev;
    e->ext.on = true;
    return AZ_OK;
}

extern "C" int az_ext_stats(const az_engine *e, int64_t *requests, int64_t *items)
{
    if (!e) return AZ_ERR_INVALID;
    if (requests) *requests = e->ext.requests;
    if (items) *items = e->ext.items;
    return AZ_OK;
}

// MCTS.run with the evaluator outside the engine: the policy_value_fn seam of mcts.py:87-93 for evaluators that are not
// this engine's net (any callable in the reference).  The search is az_search's with an external evaluator of the engine's
// own (ext_plies): each of the num_simulations + 1 evaluations is a request of one entry, whose planes callback_eval reads
// back and decodes for the callback and whose priors and value it uploads, and the tree step consumes them as they are
// (no softmax, no value head).
struct CallbackEval {
    az_engine *e; az_eval_callback fn; void *user;
    int player, stones;            // of the searched position: the side to move at a leaf follows from the leaf's stone count
    int status = 0;                // what the callback returned, if not 0
    hipError_t hip = hipSuccess;   // ... or the copy that failed
    std::vector<float> planes, policy;
    std::vector<uint8_t> cells;
};
static int callback_eval(void *user, int /*net*/, int count)
{
    CallbackEval &c = *(CallbackEval *)user;
    az_engine *e = c.e;
    const int nn = e->nn;
    if (count != 1) return -1;     // one position, one leaf per batch
    std::vector<float> &planes = c.planes, &policy = c.policy;
    std::vector<uint8_t> &cells = c.cells;
    planes.resize((size_t)3 * nn); policy.assign((size_t)nn, 0.0f); cells.resize((size_t)nn);
    if ((c.hip = az_memcpy(e->stream, planes.data(), e->cb_planes.p, planes.size() * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return -1;
    int stones = 0, last = -1;
    for (int j = 0; j < nn; j++) stones += planes[j] != 0.0f || planes[nn + j] != 0.0f;
    const int mover = ((stones - c.stones) & 1) ? 3 - c.player : c.player;
    for (int j = 0; j < nn; j++) {
        cells[j] = (uint8_t)(planes[j] != 0.0f ? mover : (planes[nn + j] != 0.0f ? 3 - mover : 0));
        if (planes[2 * nn + j] != 0.0f) last = j;
    }
    float value = 0.0f;
    if ((c.status = c.fn(c.user, cells.data(), mover, last, policy.data(), &value))) return c.status;
    c.hip = az_memcpy(e->stream, e->cb_policy.p, policy.data(), policy.size() * sizeof(float), hipMemcpyHostToDevice);
    if (c.hip == hipSuccess) c.hip = az_memcpy(e->stream, e->cb_value.p, &value, sizeof value, hipMemcpyHostToDevice);
    return c.hip == hipSuccess ? 0 : -1;
}

extern "C" int az_search_callback(az_engine *e, const uint8_t *board, int player, int last, double temperature,
                                  const double *noise, double u, az_eval_callback fn, void *user, float *pi, int32_t *action,
                                  int32_t *visits, double *W, float *prior)
{
    if (!e || !board || !fn || (player != 1 && player != 2)) return fail(e, AZ_ERR_INVALID, "az_search_callback: bad argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_search_callback: a self-play episode is open on this engine");
    if (e->vl > 1 || e->reuse || e->leaf_symmetry)
        return fail(e, AZ_ERR_INVALID, "az_search_callback: not combinable with virtual-loss batching, subtree reuse or random-symmetry leaf evaluation");
    if (e->solver) return fail(e, AZ_ERR_INVALID, "az_search_callback: not combinable with the solver");
    if (e->cand_radius) return fail(e, AZ_ERR_INVALID, "az_search_callback: not combinable with candidate moves (the callback returns priors, not logits)");
    if (noise && e->gumbel_m > 0)
        return fail(e, AZ_ERR_INVALID, "az_search_callback: a noised search under the Gumbel root search needs logits, the callback returns priors");
    int stones = 0;
    if (check_position(e, "az_search_callback", board, player, last, &stones)) return AZ_ERR_INVALID;
    DEVICE_GUARD(e);
    const size_t cap = (size_t)e->cfg.slots * e->vl, nn = (size_t)e->nn;
    int rc = dev_alloc(e, e->cb_planes, cap * 4 * nn * sizeof(float), false);
    if (!rc) rc = dev_alloc(e, e->cb_policy, cap * nn * sizeof(float), false);
    if (!rc) rc = dev_alloc(e, e->cb_value, cap * sizeof(float), false);
    if (rc) return rc;
    // The engine's own evaluator stands in for the public one (written directly: az_set_external_evaluator's refusals are
    // about the public setting) while the position is searched like any other.  What a search call reports afterwards --
    // the public evaluator and its statistics, the counters, the solver's stops -- goes back as found on every way out.
    struct Restore {
        az_engine *e; bool on; az_ext_evaluator ev; int64_t requests, items, stops; az_counters last;
        ~Restore()
        {
            e->ext.on = on; e->ext.ev = ev; e->ext.requests = requests; e->ext.items = items;
            e->solver_stops = stops; e->last = last; e->have_episode = false;
        }
    } restore{e, e->ext.on, e->ext.ev, e->ext.requests, e->ext.items, e->solver_stops, e->last};
    CallbackEval ce{e, fn, user, player, stones};
    e->ext.ev = az_ext_evaluator{(float *)e->cb_planes.p, (float *)e->cb_policy.p, (float *)e->cb_value.p, (int32_t)cap, callback_eval, &ce};
    e->ext.on = true;
    rc = search_one(e, 0, board, player, last, stones, temperature, noise, u, pi, action, visits, W, prior);
    if (ce.status) return fail(e, AZ_ERR_INVALID, "az_search_callback: the evaluator returned %d", ce.status);
    if (ce.hip != hipSuccess) return fail(e, AZ_ERR_HIP, "az_search_callback: %s", hipGetErrorString(ce.hip));
    return rc;
}

// ------------------------------------------------------------------------------------------------
// multi-GPU: the episode-end exchange on RCCL, inside the library (include/az_engine.h az_dist_*).  librccl.so.1 is bound
// at run time -- the copy a host framework (PyTorch) has already mapped if there is one, so that the process holds ONE
// RCCL, else the system's -- and only the handful of entry points used here are resolved.
// ------------------------------------------------------------------------------------------------
namespace {
typedef int nccl_result;                     // ncclResult_t; ncclSuccess = 0
enum { NCCL_INT8 = 0, NCCL_UINT8 = 1, NCCL_INT64 = 4 };      // ncclDataType_t values used (rccl.h: ncclInt8 0, ncclUint8 1, ncclInt64 4)
enum { NCCL_SUM = 0 };
struct nccl_id { char internal[AZ_DIST_ID_BYTES]; };
struct Rccl {
    void *h = nullptr;
    nccl_result (*GetUniqueId)(nccl_id *) = nullptr;
    nccl_result (*CommInitRank)(void **, int, nccl_id, int) = nullptr;
    nccl_result (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(nccl_result) = nullptr;
    nccl_result (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    nccl_result (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    nccl_result (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    nccl_result (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    nccl_result (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    nccl_result (*GroupStart)() = nullptr;
    nccl_result (*GroupEnd)() = nullptr;
    std::string err;
};
Rccl g_rccl;
std::mutex g_rccl_mutex;

const Rccl *rccl_load(std::string *err)
{
    std::lock_guard<std::mutex> lk(g_rccl_mutex);
    Rccl &r = g_rccl;
    if (r.h) return &r;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);          // the copy already in the process (PyTorch's), if any
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { *err = std::string("cannot load librccl.so.1: ") + (dlerror() ? dlerror() : "?"); return nullptr; }
    bool ok = true;
    auto sym = [&](const char *name) { void *p = dlsym(h, name); if (!p) { ok = false; *err = std::string("librccl.so.1 lacks ") + name; } return p; };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
    r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
    r.Broadcast = (decltype(r.Broadcast))sym("ncclBroadcast");
    r.Send = (decltype(r.Send))sym("ncclSend");
    r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    if (!ok) return nullptr;
    r.h = h;
    return &r;
}
}  // namespace

#define NCCLCHECK(e, R, call)                                                                      \
    do {                                                                                           \
        nccl_result _r = (call);                                                                   \
        if (_r != 0) return fail(e, AZ_ERR_HIP, "%s failed: %s (%s:%d)", #call, (R)->GetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

static void dist_destroy(az_engine *e)
{
    if (e->comm && g_rccl.h) (void)g_rccl.CommDestroy(e->comm);
    e->comm = nullptr;
    e->dist_rank = 0;
    e->dist_world = 1;
    dev_free(e->dist_buf);
    dev_free(e->dist_pack);
}

extern "C" int az_dist_unique_id(void *id)
{
    if (!id) return fail(nullptr, AZ_ERR_INVALID, "az_dist_unique_id: null argument");
    std::string err;
    const Rccl *R = rccl_load(&err);
    if (!R) return fail(nullptr, AZ_ERR_HIP, "%s", err.c_str());
    nccl_id nid;
    nccl_result rc = R->GetUniqueId(&nid);
    if (rc != 0) return fail(nullptr, AZ_ERR_HIP, "ncclGetUniqueId failed: %s", R->GetErrorString(rc));
    memcpy(id, nid.internal, AZ_DIST_ID_BYTES);
    return AZ_OK;
}

extern "C" int az_dist_init(az_engine *e, const void *id, int rank, int world)
{
    if (!e || !id || world < 1 || rank < 0 || rank >= world) return fail(e, AZ_ERR_INVALID, "az_dist_init: bad argument");
    if (e->run.open) return fail(e, AZ_ERR_STATE, "az_dist_init: an episode is open");
    std::string err;
    const Rccl *R = rccl_load(&err);
    if (!R) return fail(e, AZ_ERR_HIP, "%s", err.c_str());
    DEVICE_GUARD(e);
    dist_destroy(e);
    nccl_id nid;
    memcpy(nid.internal, id, AZ_DIST_ID_BYTES);
    void *comm = nullptr;
    NCCLCHECK(e, R, R->CommInitRank(&comm, world, nid, rank));
    e->comm = comm;
    e->dist_rank = rank;
    e->dist_world = world;
    return dev_alloc(e, e->dist_buf, (size_t)(world + 1) * 64 * sizeof(int64_t));
}

extern "C" int az_dist_rank(const az_engine *e) { return e ? e->dist_rank : AZ_ERR_INVALID; }
extern "C" int az_dist_world(const az_engine *e) { return e ? e->dist_world : AZ_ERR_INVALID; }

// records this rank contributes: the last episode's, 0 without one
static int64_t dist_local_records(const az_engine *e)
{
    if (!e->have_episode) return 0;
    return export_records(e);      // what az_selfplay_pack writes
}

static int dist_counts(az_engine *e, const Rccl *R, std::vector<int64_t> &counts)
{
    const int W = e->dist_world;
    int64_t *dv = (int64_t *)e->dist_buf.p;          // [0] mine, [64 ..] everybody's
    const int64_t mine = dist_local_records(e);
    HIPCHECK(e, hipMemcpyAsync(dv, &mine, 8, hipMemcpyHostToDevice, e->stream));
    NCCLCHECK(e, R, R->AllGather(dv, dv + 64, 1, NCCL_INT64, e->comm, e->stream));
    counts.assign(W, 0);
    HIPCHECK(e, az_memcpy(e->stream, counts.data(), dv + 64, (size_t)W * 8, hipMemcpyDeviceToHost));
    return AZ_OK;
}

extern "C" int az_dist_counts(az_engine *e, int64_t *counts)
{
    if (!e || !counts) return fail(e, AZ_ERR_INVALID, "az_dist_counts: bad argument");
    if (!e->comm) return fail(e, AZ_ERR_STATE, "az_dist_counts: az_dist_init first");
    DEVICE_GUARD(e);
    std::vector<int64_t> c;
    const int rc = dist_counts(e, &g_rccl, c);
    if (rc) return rc;
    memcpy(counts, c.data(), c.size() * 8);
    return AZ_OK;
}

extern "C" int az_dist_gather_records(az_engine *e, int dst, void *packed_dev)
{
    if (!e || dst < -1) return fail(e, AZ_ERR_INVALID, "az_dist_gather_records: bad argument");
    if (!e->comm) return fail(e, AZ_ERR_STATE, "az_dist_gather_records: az_dist_init first");
    if (dst >= e->dist_world) return fail(e, AZ_ERR_INVALID, "az_dist_gather_records: rank %d of %d", dst, e->dist_world);
    const Rccl *R = &g_rccl;
    DEVICE_GUARD(e);
    const int W = e->dist_world, me = e->dist_rank;
    const bool receive = dst < 0 || dst == me;
    if (receive && !packed_dev) return fail(e, AZ_ERR_INVALID, "az_dist_gather_records: a receiving rank needs a destination buffer");
    std::vector<int64_t> counts;
    int rc = dist_counts(e, R, counts);
    if (rc) return rc;
    const int64_t rb = record_bytes(e->nn), mine = counts[me];
    std::vector<int64_t> off(W + 1, 0);
    for (int r = 0; r < W; r++) off[r + 1] = off[r] + counts[r] * rb;
    // this rank's records: straight into their place of the destination where this rank receives, else into a send buffer
    unsigned char *out = (unsigned char *)packed_dev;
    void *my_dev = nullptr;
    if (mine > 0) {
        if (receive) my_dev = out + off[me];
        else {
            if ((rc = dev_alloc(e, e->dist_pack, (size_t)(mine * rb), false))) return rc;
            my_dev = e->dist_pack.p;
        }
        if ((rc = az_selfplay_pack(e, my_dev))) return rc;
    }
    if (W == 1) return AZ_OK;
    NCCLCHECK(e, R, R->GroupStart());
    nccl_result gr = 0;
    if (mine > 0)
        for (int r = 0; r < W && gr == 0; r++)
            if (r != me && (dst < 0 || dst == r)) gr = R->Send(my_dev, (size_t)(mine * rb), NCCL_UINT8, r, e->comm, e->stream);
    if (receive)
        for (int r = 0; r < W && gr == 0; r++)
            if (r != me && counts[r] > 0) gr = R->Recv(out + off[r], (size_t)(counts[r] * rb), NCCL_UINT8, r, e->comm, e->stream);
    const nccl_result ge = R->GroupEnd();
    if (gr != 0 || ge != 0) return fail(e, AZ_ERR_HIP, "RCCL send/recv of the records failed: %s", R->GetErrorString(gr != 0 ? gr : ge));
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    return AZ_OK;
}

extern "C" int az_dist_allreduce_sum(az_engine *e, int64_t *values, int n)
{
    if (!e || !values || n < 1 || n > 64) return fail(e, AZ_ERR_INVALID, "az_dist_allreduce_sum: 1..64 values");
    if (!e->comm) return fail(e, AZ_ERR_STATE, "az_dist_allreduce_sum: az_dist_init first");
    const Rccl *R = &g_rccl;
    DEVICE_GUARD(e);
    int64_t *dv = (int64_t *)e->dist_buf.p;
    HIPCHECK(e, hipMemcpyAsync(dv, values, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    NCCLCHECK(e, R, R->AllReduce(dv, dv, (size_t)n, NCCL_INT64, NCCL_SUM, e->comm, e->stream));
    HIPCHECK(e, az_memcpy(e->stream, values, dv, (size_t)n * 8, hipMemcpyDeviceToHost));
    return AZ_OK;
}

extern "C" int az_dist_broadcast(az_engine *e, void *buf_dev, int64_t bytes, int root)
{
    if (!e || !buf_dev || bytes < 0) return fail(e, AZ_ERR_INVALID, "az_dist_broadcast: bad argument");
    if (!e->comm) return fail(e, AZ_ERR_STATE, "az_dist_broadcast: az_dist_init first");
    if (root < 0 || root >= e->dist_world) return fail(e, AZ_ERR_INVALID, "az_dist_broadcast: root %d of %d", root, e->dist_world);
    if (bytes == 0) return AZ_OK;
    const Rccl *R = &g_rccl;
    DEVICE_GUARD(e);
    NCCLCHECK(e, R, R->Broadcast(buf_dev, buf_dev, (size_t)bytes, NCCL_UINT8, root, e->comm, e->stream));
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    return AZ_OK;
}
