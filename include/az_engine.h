/*
 * az_engine.h -- C-ABI of the MI355X-native batched self-play engine.
 *
 * Drop-in boundary for the hot path of VojtaHavlicek/AlphaZero-Piskvorky
 * (alphazero/mcts.py + alphazero/self_play.py + alphazero/net.py, with games.py,
 * controller.make_policy_value_fn and evaluator.py).  The reference has no FFI of its
 * own: its seams are Python call signatures.  Each entry point below
 * names the reference interface it stands behind; the Python shims in
 * alphazero-piskvorky_amd/ keep those signatures and call this library via ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions: every call returns 0 on success or a negative az_status; nothing throws
 * or aborts across the boundary; the caller owns all input buffers; outputs are written
 * into caller-provided buffers; one engine per GPU; calls on one engine are serialised by
 * the caller (the engine runs its own host threads inside a call, one per lane, and joins them
 * before returning); engines on different GPUs are independent; the calling thread's current
 * HIP device is left as it was.  Pointers suffixed _dev are
 * device pointers (e.g. torch tensor.data_ptr()), all others are host pointers.
 *
 * The library contains NO CPU implementation of the path: az_create fails with
 * AZ_ERR_NO_DEVICE when no gfx950 device is present.
 */
#ifndef AZ_ENGINE_H
#define AZ_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct az_engine az_engine;

typedef enum {
    AZ_OK = 0,
    AZ_ERR_INVALID = -1,     /* bad argument / unsupported configuration            */
    AZ_ERR_NO_DEVICE = -2,   /* no HIP device (the engine has no CPU fallback)      */
    AZ_ERR_HIP = -3,         /* a HIP runtime call failed; see az_last_error        */
    AZ_ERR_ILLEGAL_MOVE = -4,/* games.py:76-77 ValueError("Invalid move")           */
    AZ_ERR_NO_WEIGHTS = -5,  /* net evaluator selected but slot not loaded          */
    AZ_ERR_STATE = -6        /* call sequence error (e.g. export before self-play)  */
} az_status;

enum { AZ_EVAL_NET = 0, AZ_EVAL_SYNTHETIC = 1 };   /* synthetic = deterministic hash evaluator (test hook, mcts.py:87-93 seam) */
enum { AZ_RES_NONE = 0, AZ_RES_X = 1, AZ_RES_O = 2, AZ_RES_DRAW = 3 }; /* constants.py:11-13 'X','O','D' */
enum { AZ_AUG_REFERENCE4 = 4, AZ_AUG_DIHEDRAL8 = 8, AZ_AUG_NONE = 1 };
enum { AZ_TRUNK_F32 = 0, AZ_TRUNK_BF16X3 = 1, AZ_TRUNK_F16X2 = 2 };   /* arithmetic of the conv trunk, az_set_trunk_mode */
enum { AZ_MODEL_PLAIN = 0, AZ_MODEL_RESNET = 1 };  /* net.py GomokuNet | ResidualBlock variant (README.md:72) */

/* Hyper-parameters the reference keeps in constants.py / MCTS.__init__ (mcts.py:87-97). */
typedef struct {
    int32_t board_size;        /* constants.py:2  BOARD_SIZE   (3 .. 15)                         */
    int32_t win_length;        /* constants.py:3  WIN_LENGTH                                     */
    int32_t num_simulations;   /* mcts.py:89      num_simulations (<= 1024; az_create_deep: <= 65534) */
    int32_t slots;             /* concurrent games resident on this GPU                          */
    double c_puct;             /* mcts.py:90                                                      */
    double dirichlet_alpha;    /* mcts.py:91 (0.3)                                                */
    double dirichlet_weight;   /* mcts.py:92 (0.25)                                               */
    int32_t eval_kind;         /* AZ_EVAL_NET | AZ_EVAL_SYNTHETIC                                 */
    int32_t device;            /* HIP device ordinal                                              */
    /* Optional tables so that the host layer can hand over the reference's own numpy values:
       log_table[N] = float32 log(N + 1e-8) for N = 0..num_simulations (mcts.py:161);
       NULL -> computed with libm logf.                                                          */
    const float *log_table;
    int32_t model;             /* AZ_MODEL_PLAIN (net.py:16-72) | AZ_MODEL_RESNET (config 5)                         */
    /* Lanes inside the engine: the slots are split over `engines` HIP streams, each driven by its own host thread inside
       the library, so that one lane's latency-bound tree / FC kernels run underneath another lane's conv trunk.  All lanes
       take their games from one shared queue (a freed slot of any lane gets the next waiting game) and write into the
       same per-game records, so the episode is the same whatever the number of lanes.  0 = the library chooses
       (1 for boards up to 5x5, else one lane per 128 slots up to 4).  Replaces the worker processes of
       self_play.py:29-45,122-136 (NUM_WORKERS, constants.py:6). */
    int32_t engines;
} az_config;

/* ---- lifecycle ---- */
int az_create(const az_config *cfg, az_engine **out);

/* Deep searches: the reference takes any num_simulations (mcts.py:18 DEFAULT_NUM_SIMULATIONS = 10_000).  az_create_deep is
 * az_create with num_simulations allowed in 1..AZ_DEEP_MAX_SIMULATIONS, a bound set by the 16-bit child row, path row and
 * visit-count fields of the tree.  It is a separate entry point because the tree memory grows with S: (S + 1) x
 * roundup(n*n, 64) x 16 B per slot (41 MB at 15x15 / S = 10 000), and a caller has to ask for that.  Before it allocates
 * anything it adds up the trees of all slots and the tables that grow with S and returns AZ_ERR_INVALID, with the byte
 * count in az_last_error, when that exceeds the device's free memory.
 * Up to 1024 simulations a deep engine IS the default engine (same kernels, same results, same persistent-kernel choice).
 * Above 1024 the tree step runs its deep instantiations (the sqrt table read from HBM instead of LDS; with virtual-loss
 * batching the in-flight counts in a byte per edge beside the tree, allocated by az_set_virtual_loss under the same memory
 * check), each ply is launched kernel by kernel instead of as one captured graph, and the persistent search kernel is never
 * chosen.  Results are bit-identical to the oracle at any S.  Everything else combines as below 1024: evaluation cache,
 * random-symmetry leaf evaluation, both nets, the emulated trunks, az_search, az_search_callback, az_arena and virtual-loss
 * batching.  Subtree reuse stays limited to 1023 simulations (az_set_subtree_reuse). */
#define AZ_DEEP_MAX_SIMULATIONS 65534
int az_create_deep(const az_config *cfg, az_engine **out);
void az_destroy(az_engine *e);
const char *az_last_error(const az_engine *e);   /* valid until the next call on e; e may be NULL */

/* ---- weights: replaces state_dict pickling into workers (self_play.py:121,127,36) ----
 * tensors[16] in net.py:37-53 state_dict order (conv1.weight, conv1.bias, conv2.*, conv3.*,
 * policy_conv.*, policy_fc.*, value_conv.*, value_fc1.*, value_fc2.*), fp32, torch layouts.
 * slot 0 = self-play / candidate, slot 1 = arena baseline (evaluator.py:53-62). */
int az_load_weights(az_engine *e, int slot, const float *const *tensors);

/* ResidualBlock variant (engines created with model = AZ_MODEL_RESNET).  The reference no longer ships a forward
 * for it; the topology is fixed by its historical checkpoints (alphazero/models/old/model_20250728_*.pt) and the
 * block by legacy/resnet/example.py:9-27: conv(4->64)+BN+ReLU, 3 x {conv+BN+ReLU, conv+BN, +skip, ReLU},
 * policy_conv(64->2)+BN+ReLU -> policy_fc(2n^2 -> n^2), value_conv(64->1)+BN+ReLU -> value_fc1(n^2 -> 64) -> ReLU ->
 * value_fc2 -> tanh.  tensors[24], fp32, eval-mode BatchNorm already FOLDED into conv weight/bias by the caller:
 *   0,1 stem w[64,4,3,3], b[64];  2+2i, 3+2i (i = 0..5) res{1,2,3}.conv{1,2} w[64,64,3,3], b[64];
 *   14,15 policy_conv w[2,64], b[2];  16,17 value_conv w[1,64], b[1];  18,19 policy_fc w[n^2,2n^2], b[n^2];
 *   20,21 value_fc1 w[64,n^2], b[64];  22,23 value_fc2 w[64], b[1]. */
int az_load_weights_resnet(az_engine *e, int slot, const float *const *tensors);

/* ---- batched net evaluation: controller.make_policy_value_fn (controller.py:33-55) ----
 * boards[count][n*n] absolute cells (0 empty, 1 X, 2 O), players[count] side to move,
 * lasts[count] last action (r*n+c, -1 none).  Outputs: logits/policy [count][n*n], value[count].
 * Any output pointer may be NULL. */
int az_net_eval(az_engine *e, int slot, int count, const uint8_t *boards, const uint8_t *players,
                const int16_t *lasts, float *logits, float *policy, float *value);

/* ---- single-position search: MCTS.run (mcts.py:101-183) ----
 * noise: Dirichlet sample over the legal cells in row-major order, or NULL for add_root_noise=False;
 * u: the uniform np.random.choice draws (mcts.py:177).  temperature as float64 (np.float64 schedules).
 * Outputs (any may be NULL): pi[n*n] float32, action, visits[n*n], W[n*n] float64, prior[n*n]. */
int az_search(az_engine *e, int slot, const uint8_t *board, int player, int last, double temperature,
              const double *noise, double u, float *pi, int32_t *action, int32_t *visits, double *W,
              float *prior);

/* ---- many positions at once: MCTS.run (mcts.py:101-183) for every position of a list ----
 * The throughput form of az_search: the positions are searched in waves of at most `slots`, every wave as one ply of every
 * lane, so the searches share their evaluation batches instead of each being a latency-bound chain over one board.  The
 * outputs of position i are exactly what az_search(e, slot, boards[i], players[i], lasts[i], temperatures[i],
 * noise ? row i : NULL, u[i], ...) returns on the same engine, whatever count, slots and lanes are, and with every search
 * option (virtual-loss batching, evaluation cache, random-symmetry leaf evaluation with key 0 for every position as in
 * az_search, both nets, the synthetic evaluator, the emulated trunks, deep engines; boards up to 7x7 run on the persistent
 * search kernel).  Every search starts from a fresh root.  Noise is all or nothing per call.
 * Every position is checked on the host first, by az_search's rules (cell values, at least one legal action, last in range
 * and on an occupied cell, player 1 or 2): AZ_ERR_INVALID, with the index of the first offending position in az_last_error
 * and no output written.  count = 0 returns AZ_OK and touches nothing.  AZ_ERR_STATE while an episode is open;
 * AZ_ERR_NO_WEIGHTS as az_search.  Like az_search the call forgets the last self-play episode (az_selfplay_games /
 * az_selfplay_records then fail with AZ_ERR_STATE).  Afterwards az_get_counters reports the sums over the whole batch
 * (simulations = count * num_simulations, root_evals = plies = count).  Device and host memory of the call are bounded by
 * the engine's slots, not by count. */
int az_search_batch(az_engine *e, int slot, int count,
                    const uint8_t *boards,        /* [count][n*n] absolute cells 0 / 1 X / 2 O          */
                    const uint8_t *players,       /* [count] side to move, 1 / 2                        */
                    const int16_t *lasts,         /* [count] last action r*n+c, -1 none                 */
                    const double *temperatures,   /* [count], one per position (np.float64 schedules)  */
                    const double *noise,          /* NULL = add_root_noise False for all; else [count][n*n]: row i holds the Dirichlet
                                                     sample of position i over its legal cells in row-major order in its first
                                                     (n*n - stones_i) entries, the rest is ignored */
                    const double *u,              /* [count] the np.random.choice draw of each search  */
                    float *pi, int32_t *actions, int32_t *visits, double *W, float *prior);
                    /* outputs [count][n*n] (actions: [count]); any may be NULL */

/* ---- the same search with the evaluator outside the engine: the policy_value_fn plugin seam (mcts.py:87-93) ----
 * The reference's MCTS takes ANY callable state -> (policy float32[n,n], value float) (controller.py:39-53 is just the
 * one the training loop uses).  az_search_callback keeps that seam: select / expand / backup / pi extraction run on the
 * GPU as in az_search, and each of the num_simulations + 1 evaluations (mcts.py:109,137) is handed to `fn` on the host:
 * board[n*n] absolute cells (0 empty, 1 X, 2 O), player = side to move there, last = last action (-1 none); fn writes
 * policy[n*n] (used as priors exactly as given: mcts.py:63 float(policy[r, c]), no masking, no renormalisation) and
 * *value (from the point of view of `player`), and returns 0 (anything else aborts the search with AZ_ERR_INVALID).
 * One host round trip per simulation: a compatibility path, not a fast one.  Needs no weights; not combinable with
 * virtual-loss batching or subtree reuse.  Other arguments and outputs as az_search. */
typedef int (*az_eval_callback)(void *user, const uint8_t *board, int player, int last, float *policy, float *value);
int az_search_callback(az_engine *e, const uint8_t *board, int player, int last, double temperature, const double *noise,
                       double u, az_eval_callback fn, void *user, float *pi, int32_t *action, int32_t *visits, double *W,
                       float *prior);

/* Opt-in: batched external evaluator -- the same seam (mcts.py:87-93: ANY callable evaluates) for every game at once and on
 * device buffers, so that self-play, the arena and batched search run at the tree kernels' speed with any net that lives on
 * the same GPU (a torch module the engine has no kernels for).  While one is set, every net evaluation of az_selfplay*
 * (begin / step / end included), az_arena, az_search and az_search_batch -- the root evaluations and the expanded leaves --
 * goes through it; az_search_callback, az_net_eval and az_rules_replay ignore the setting.  No weights are needed
 * (AZ_ERR_NO_WEIGHTS is not raised on this path) and az_config.eval_kind is overridden.
 *
 * One evaluation step (per ply 1 root step, then num_simulations steps, ceil(num_simulations / L) with virtual-loss
 * batching): a gather kernel collects the pending items of ALL lanes that need net `net` into one compact request, in
 * ascending (lane, slot, leaf-of-batch) order -- their encoded planes into planes_dev, an item -> slot map and the count stay
 * on the device; the engine synchronises its stream; it calls fn(user, net, count) ON THE CALLING THREAD (no library host
 * thread ever calls fn); a scatter kernel puts policy_dev / value_dev of the `count` entries back; the tree step runs.  A step
 * with no pending item makes no call.  A duplicate pending leaf of a virtual-loss batch is handed out once.  There are no
 * cache hits: the evaluation cache is bypassed, as for az_search_callback.  net: 0 in self-play; in the arena at most two
 * requests per step, 0 (candidate) then 1 (baseline), each homogeneous; in az_search / az_search_batch the `slot` argument.
 *
 * Synchronisation is the evaluator's side of the contract: when fn is called the planes are complete in device memory (the
 * engine has synchronised its stream); when fn RETURNS, policy_dev and value_dev of entries 0 .. count-1 must be complete in
 * device memory -- an evaluator that works on a stream of its own (torch) synchronises that stream before it returns.  The
 * engine does no cross-stream ordering of its own.  fn returns 0; anything else aborts the call with AZ_ERR_INVALID ("the
 * evaluator returned %d"), the episode is closed, the slots are left idle and the engine stays usable.
 *
 * On this path all lanes of the engine advance together from the calling thread, kernel by kernel on one stream: no
 * captured graph, no lane threads, and the persistent search kernel is never chosen (az_get_persistent == 0).  Slot refill
 * and compaction between plies work as always.  Combines with virtual-loss batching (1..32: L leaves per game cut the round
 * trips by L), start positions, resignation and the search value per record, deep engines, both step APIs, every board size
 * and max_plies.  NOT with subtree reuse or random-symmetry leaf evaluation (out of scope here): AZ_ERR_INVALID, whichever
 * is set first.  The emulated trunk mode and the evaluation cache setting are irrelevant while the evaluator is external and
 * back in force once it is cleared (ev = NULL: the engine's own evaluator again).
 *
 * Errors: AZ_ERR_STATE while an episode is open; AZ_ERR_INVALID for a NULL buffer or fn, a planes_dev that is not 16-byte
 * aligned, or capacity < az_ext_capacity(e) = slots x leaves per batch -- checked again when an episode begins, because
 * az_set_virtual_loss may have changed L since.  Counters: the tree counters as always; trunk_launches, trunk_boards,
 * nn_seconds and trunk_seconds are 0; az_ext_stats gives the requests made (calls of fn) and the items handed out in the
 * last (or open) episode / call: items == expansions + root_evals, every evaluation is handed out exactly once. */
typedef int (*az_eval_batch_fn)(void *user, int net, int count);   /* 0 = ok; anything else aborts the call */
typedef struct {
    float *planes_dev;   /* [capacity][4][n][n]  written by the engine: games.py:86-129 encode, plane 0 the side to move,
                            1 the opponent, 2 the last move one-hot (all zero when there is none), 3 zeros; every float of
                            entries 0 .. count-1, nothing behind them                                                */
    float *policy_dev;   /* [capacity][n*n]      written by the evaluator: priors, used exactly as given (mcts.py:63;
                            no mask, no renormalisation), as az_search_callback                                      */
    float *value_dev;    /* [capacity]           written by the evaluator: value for the side to move of that item   */
    int32_t capacity;    /* >= az_ext_capacity(e) = slots x leaves per batch (az_set_virtual_loss)                   */
    az_eval_batch_fn fn; void *user;
} az_ext_evaluator;
int az_set_external_evaluator(az_engine *e, const az_ext_evaluator *ev);   /* NULL: the engine's own evaluator again */
int az_get_external_evaluator(const az_engine *e);                        /* 1 / 0 */
int az_ext_capacity(const az_engine *e);
int az_ext_stats(const az_engine *e, int64_t *requests, int64_t *items);   /* of the last (or open) episode / call */

/* ---- self-play episode: SelfPlayManager.generate_self_play + _worker (self_play.py:29-77,110-159) ----
 * Plays games with ids [0, num_games); game g draws its randomness from numpy-compatible
 * RandomState(seed0 + g) (dirichlet then one uniform per ply) unless a tape is given.
 * temperature_table[m], m = 0..n*n : temperature_schedule(m) evaluated by the host layer
 * (self_play.py:24-26,53); NULL -> the reference default (exp(-m/100)+0.01)/1.01 via libm.
 * max_plies > 0 cuts every game after that many plies (fixtures / benchmarking), 0 = play to the end.
 * Results stay resident on the device until the next az_selfplay / az_destroy. */
typedef struct {
    uint64_t seed0;
    int32_t num_games;
    int32_t max_plies;
    const double *temperature_table;
    /* optional explicit tapes (tests): noise_tape[g] concatenated per game with stride tape_stride doubles,
       u_tape[g][n*n]; NULL -> generated from seed0 + g */
    const double *noise_tape;
    const double *u_tape;
    int64_t tape_stride;
} az_selfplay_args;

typedef struct {
    int64_t games, plies, records;      /* records = plies (one per position, before augmentation)      */
    int64_t simulations;                /* MCTS simulations run (mcts.py:123)                            */
    int64_t expansions;                 /* non-terminal leaf evaluations (mcts.py:136-138)               */
    int64_t root_evals;                 /* root evaluations (mcts.py:109), one per ply                   */
    int64_t terminal_hits;              /* simulations ending in a terminal leaf (mcts.py:132-134)       */
    int64_t depth_sum;                  /* sum of selection depths (mean depth = depth_sum/simulations)  */
    int64_t steps;                      /* lock-step evaluation batches launched                         */
    double seconds;                     /* device wall time of the episode                               */
    double nn_seconds;                  /* HIP-event time inside the net kernels                         */
    double trunk_seconds;               /* ... of which the fused conv trunk (dominant kernel)           */
    int64_t trunk_launches;
    int64_t trunk_boards;               /* boards evaluated by the trunk kernel (all launches)           */
    double step_seconds;                /* HIP-event time inside the tree kernel k_step (select/expand/backup) */
    int64_t duplicate_leaves;           /* virtual-loss batching: simulations that met a leaf already pending in their batch */
    int64_t cache_lookups, cache_hits;  /* evaluation cache: positions looked up / found (a hit skips the net kernels)  */
    /* Host side of the RNG tapes (mcts.py:114,177 draws, produced on the host ahead of the games): the longest time any
       lane's driver thread was blocked because the tape wave of its next ply was not yet produced or uploaded -- 0 when the
       producer keeps ahead of the games; a tape-bound run (many ranks on few cores) shows up here instead of looking like
       a slow GPU.  tape_threads = producer threads of this engine, host_cpus = CPUs the process may use (affinity mask
       and cgroup quota) that the count was sized from. */
    double tape_wait_seconds;
    int64_t tape_threads, host_cpus;
} az_counters;

int az_selfplay(az_engine *e, const az_selfplay_args *args, az_counters *out);

/* The same episode in pieces (benchmarks, pipelined callers): begin uploads tapes and fills the slots;
 * step plays up to max_steps plies of every active game in lock step (one step = MCTS.run for each
 * active game = 1 + num_simulations evaluation batches) and reports the number of still-active slots and,
 * optionally, the counters so far; end finalises the per-game results. */
int az_selfplay_begin(az_engine *e, const az_selfplay_args *args);
int az_selfplay_step(az_engine *e, int max_steps, int32_t *active_out, az_counters *progress);
int az_selfplay_end(az_engine *e, az_counters *out);

/* Per-game summary of the last episode: nply[g], result[g] (AZ_RES_*). */
int az_selfplay_games(az_engine *e, int32_t *nply, int32_t *result);

/* Raw per-ply records of the last episode, game-major then ply (tests/diagnostics):
 * boards[records][n*n] absolute cells before the move, movers, lasts, actions, pis[records][n*n],
 * visits[records][n*n], z[records] (self_play.py:71; 99 when the game was cut by max_plies). */
int az_selfplay_records(az_engine *e, uint8_t *boards, uint8_t *movers, int16_t *lasts, int16_t *actions,
                        float *pis, int32_t *visits, int8_t *z);

/* Forgets the last episode: afterwards the engine is in the state of one that has not played (az_selfplay_games,
 * az_selfplay_records and az_selfplay_pack fail with AZ_ERR_STATE, az_dist_counts / az_dist_gather_records contribute 0
 * records).  For a rank that got no games in the current episode: without it the rank would send its previous episode again.
 * AZ_ERR_STATE while an episode is open. */
int az_selfplay_clear(az_engine *e);

/* Packed records for the episode-end exchange (RCCL gather over xGMI), game-major then ply like
 * az_selfplay_records.  One record = az_record_bytes() bytes, little-endian:
 *   [0, 64)              8 x uint64 bit-planes, cell c = bit (c & 63) of word (c >> 6): words 0..3 the MOVER's stones,
 *                        words 4..7 the opponent's (n <= 15: cells 0..224);
 *   [64, 64 + 4 n*n)     pi float32[n*n];
 *   then int16 last move (-1 at the first ply), uint8 mover (1 / 2), int8 z;
 *   padded to a multiple of 8 bytes (4 padding bytes when n is even, none when n is odd; their content is unspecified).
 * z is self_play.py:71's label: +1 the mover won, -1 the mover lost, 0 draw.  A game cut by max_plies has no outcome: its
 * records carry z = 99, here exactly as in az_selfplay_records.
 * az_selfplay_pack writes records*az_record_bytes bytes to a DEVICE buffer. */
int64_t az_record_bytes(const az_engine *e);
int az_selfplay_pack(az_engine *e, void *packed_dev);

/* ---- multi-GPU: the episode-end exchange inside the library (replaces result_queue.put / get across workers,
 * self_play.py:73,140, and the tally of evaluator.py:106-109 across ranks) ----
 * One engine per rank = per GPU; ranks play disjoint game ids (the caller passes seed0 + first id and its share of the
 * games to az_selfplay / az_arena), so the only communication is at episode end.  The library calls RCCL directly on the
 * engine's own stream (librccl.so.1 is bound at run time: the copy a host framework has already loaded, else the
 * system's); nothing here needs torch.distributed.
 *   az_dist_unique_id   one rank creates the communicator id (ncclGetUniqueId) and hands its AZ_DIST_ID_BYTES bytes to the
 *                       other ranks over whatever channel the caller has (a file, MPI, a launcher's store);
 *   az_dist_init        collective: every rank joins with the same id (ncclCommInitRank on the engine's device);
 *   az_dist_counts      collective: counts[world] = records of every rank's last episode (ncclAllGather of one int64);
 *   az_dist_gather_records  collective: the packed records (az_record_bytes each, as az_selfplay_pack writes them) of all
 *                       ranks, in rank order, into packed_dev on rank dst -- grouped ncclSend / ncclRecv of the TRUE sizes, no
 *                       padding to the largest rank, nothing sent to ranks that do not train; dst = -1: every rank
 *                       receives everything.  packed_dev (DEVICE) needs room for sum(counts) records on a receiving rank
 *                       and may be NULL elsewhere.  A rank without an episode contributes 0 records.
 *   az_dist_allreduce_sum   collective: element-wise sum of n int64 values over the ranks (the arena's wins / losses / draws);
 *   az_dist_broadcast   collective: bytes of a DEVICE buffer from rank root to every rank (new weights after train_step).
 * az_dist_rank / az_dist_world: 0 / 1 before az_dist_init.  Errors: AZ_ERR_STATE without az_dist_init, AZ_ERR_HIP with the
 * RCCL message in az_last_error when RCCL cannot be loaded or a call fails. */
#define AZ_DIST_ID_BYTES 128
int az_dist_unique_id(void *id);
int az_dist_init(az_engine *e, const void *id, int rank, int world);
int az_dist_rank(const az_engine *e);
int az_dist_world(const az_engine *e);
int az_dist_counts(az_engine *e, int64_t *counts);
int az_dist_gather_records(az_engine *e, int dst, void *packed_dev);
int az_dist_allreduce_sum(az_engine *e, int64_t *values, int n);
int az_dist_broadcast(az_engine *e, void *buf_dev, int64_t bytes, int root);

/* Training examples: (state f32[4,n,n], pi f32[n,n], z) with the augmentation of
 * SelfPlayManager._augment_symmetries fused into the encode (self_play.py:94-108,146-148):
 * AZ_AUG_REFERENCE4 reproduces the reference (state rot k*90deg, pi rot 90deg once, Q16),
 * AZ_AUG_DIHEDRAL8 is the correct 8-fold group, AZ_AUG_NONE emits each position once.
 * Reads `records` packed records from packed_dev (this rank's or gathered ones) and writes
 * records*aug examples to DEVICE buffers, order (record, k).  Every cell of every example is written (plane 3 with
 * zeros), nothing behind the last example.  z is handed on as it is packed: cut games carry z = 99.0f as the value target;
 * callers that train must not cut (the Python seams never pass max_plies).  records = 0 returns AZ_OK without touching
 * any buffer (the pointers may then be NULL). */
int az_examples_from_packed(az_engine *e, const void *packed_dev, int64_t records, int aug,
                            float *states_dev, float *pis_dev, float *z_dev);

/* Training batch from a device-resident replay ring of packed records (replay_buffer.py:26-39 sample_batch +
 * controller.py:23-31 collate, with no host round trip): example i = symmetry sym_dev[i] (0..7, dihedral group;
 * 0..3 are the rotations) of record idx_dev[i].  reference_pi != 0 rotates pi once whatever the symmetry, like
 * self_play.py:105 does.  All pointers are DEVICE pointers.  idx_dev may repeat and need not be ordered; the caller keeps
 * it inside the ring and sym_dev inside 0..7 (neither is checked).  z as in az_examples_from_packed: cut games carry
 * z = 99.0f; callers that train must not cut.  count = 0 returns AZ_OK without touching any buffer (the pointers may
 * then be NULL: the batch of an empty ring). */
int az_examples_gather(az_engine *e, const void *packed_dev, const int64_t *idx_dev, const int32_t *sym_dev,
                       int count, int reference_pi, float *states_dev, float *pis_dev, float *z_dev);

/* ---- arena: ModelEvaluator.evaluate (evaluator.py:38-122) ----
 * candidate = slot 0 plays X, baseline = slot 1 plays O, odd game index => O moves first;
 * per-game RandomState(seed0 + g), one uniform per ply; temperature_table[step] =
 * evaluator.temperature_schedule(step) (NULL -> 0.3*exp(-step/4) via libm). */
typedef struct {
    uint64_t seed0;
    int32_t num_games;
    const double *temperature_table;
    const double *u_tape;               /* optional [num_games][n*n] */
} az_arena_args;
typedef struct { int32_t wins, losses, draws, total; double win_rate; } az_arena_result;
int az_arena(az_engine *e, const az_arena_args *args, az_arena_result *out, int32_t *results, int16_t *actions,
             int32_t *nply);

/* ---- rules only: Gomoku.apply_action / is_terminal / get_game_result (games.py:64-82,133-179) ----
 * Replays `games` action lists (actions[g][max_len], r*n+c, -1 = end of list) from the empty board with X to move, on the
 * device, with the same bit-plane win test the search kernels use (under the engine's win rule, az_set_win_rule).  Like the reference, apply_action does not look at
 * the terminal flag (a list may continue past the end of the game; the winner stays the first one, games.py:140-141).
 * Outputs (term_before may be NULL): term_before[g][i] = is_terminal() before move i; boards[g][n*n] final cells
 * (0 empty, 1 X, 2 O); players[g] = side to move afterwards; results[g] = AZ_RES_*; first_illegal[g] = index of the
 * first illegal action of the list (occupied cell or out of range: games.py:76-77 ValueError), -1 if none -- the replay
 * of that game stops there. */
int az_rules_replay(az_engine *e, int games, int max_len, const int16_t *actions, uint8_t *term_before, uint8_t *boards,
                    int32_t *players, int32_t *results, int32_t *first_illegal);

/* ---- host-side numpy-compatible RNG (legacy MT19937 RandomState; mcts.py:114,177) ---- */
int az_rng_selfplay_tape(uint64_t seed, int board_size, double alpha, int max_plies, double *noise, double *u);
int az_rng_uniforms(uint64_t seed, int count, double *u);
/* az_set_gumbel's tape: per ply p, n * n - p draws of RandomState(seed).gumbel() (-log(-log(1 - U)), one random_sample each) and
 * then one uniform, in az_rng_selfplay_tape's layout */
int az_rng_selfplay_tape_gumbel(uint64_t seed, int board_size, int max_plies, double *noise, double *u);

/* ---- device RNG: counter-based Philox tapes made on the GPU (opt-in; throughput runs) ----
 * az_set_rng(e, AZ_RNG_PHILOX) replaces the host tape producer above: az_selfplay_begin fills noise[G][tape_len] and
 * u[G][n*n] with one launch of k_tape before the first ply, az_arena its u alone; no pinned staging is allocated, no host
 * tape thread runs (az_counters.tape_threads and tape_wait_seconds read 0).  AZ_RNG_NUMPY (0), the default, is the numpy
 * stream of az_rng_selfplay_tape, and with it the engine equals the reference.  An explicit noise_tape / u_tape is taken
 * as given in either mode; az_search* with a caller's noise are untouched; every consumer kernel reads the same buffers in
 * the same layout, so the mode combines with every option.  az_set_rng returns AZ_ERR_STATE while an episode is open and
 * AZ_ERR_INVALID for another mode; az_get_rng returns the mode.
 *
 * The stream.  Every draw is a pure function of (game seed, ply m, legal rank j, attempt t, purpose): nothing depends on
 * max_plies, on the order of generation or on which other games are generated.
 *   Generator.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): ten rounds of
 *       (c0, c1, c2, c3) <- (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0)),
 *   M0 = 0xD2511F53, M1 = 0xCD9E8D57, hi / lo the halves of the 64-bit product; after each round k0 += 0x9E3779B9,
 *   k1 += 0xBB67AE85 (mod 2^32).  az_rng_philox4x32 is this function.
 *   Key.  seed = seed0 + g (mod 2^64), the per-game seed of the numpy tapes: key = (seed & 0xffffffff, seed >> 32).
 *   Counter.  (c0, c1, c2, c3) = (attempt t, rank j, ply m, purpose).
 *   Words to doubles.  One call's words (w0, w1, w2, w3) give Ua = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 and
 *   Ub = ((w2 >> 5) * 2^26 + (w3 >> 6)) / 2^53, both in [0, 1) and exact.
 *   Purposes.  0 move uniform: u[m] = Ua of (t 0, j 0, m, 0).  1 normal pair: (Ua, Ub) of (t, j, m, 1).  2 acceptance
 *   uniform: Ua of (t, j, m, 2).  3 boost uniform: Ua of (0, j, m, 3).  4 Gumbel: Ua of (0, j, m, 4).
 *   log and exp.  log is az_rng_log, a software float64 logarithm (argument reduction to [sqrt(1/2), sqrt(2)) and one fma
 *   polynomial; log(0) = -inf), exp is az_rng_exp, the float64 exp the engine's softmax uses, which gives 0 below -708.  Everything else is a separately
 *   rounded float64 + - * / sqrt in the order written here, left to right.
 *   Gamma(alpha) of (m, j).  Marsaglia and Tsang with shape a = alpha if alpha >= 1, else alpha + 1: d = a - 1/3,
 *   c = 1 / sqrt(9 * d).  Attempt t = 0, 1, ..: x1 = 2 * Ua - 1, x2 = 2 * Ub - 1 of the normal pair, r2 = x1 * x1 + x2 * x2;
 *   the attempt fails if r2 >= 1 or r2 == 0; x = x1 * sqrt(-2 * log(r2) / r2) (the polar method; its second normal is not
 *   used); v = 1 + c * x; the attempt fails if v <= 0; v = v * v * v; U the attempt's acceptance uniform, xx = x * x; the
 *   attempt succeeds if U < 1 - 0.0331 * xx * xx, or else if log(U) < 0.5 * xx + d * (1 - v + log(v)); the draw is d * v.
 *   After AZ_RNG_PHILOX_ATTEMPTS (64) failed attempts the draw is d (v = 1, the value at x = 0; probability below 1e-38
 *   per draw), so no input keeps a lane in the loop.  For alpha < 1 the draw is then multiplied by exp(log(U) / alpha), U the
 *   boost uniform.
 *   Dirichlet.  Ply m holds k = n*n - m entries, entry j = gamma_j / sum, or 1 / k each if sum == 0.  The sum has one order:
 *   64 partial sums p[l] = 0 + gamma_l + gamma_(l+64) + ... by rising rank, then p[l] = p[l] + p[l + h] for every l < h, for
 *   h = 32, 16, 8, 4, 2, 1; sum = p[0].
 *   Gumbel kind (AZ_TAPE_GUMBEL; the engine's choice under az_set_gumbel).  Entry j = -log(-log(1 - U)).
 *   Layout.  az_rng_selfplay_tape's: per game, ply m holds its k doubles at offset sum_{i<m} (n*n - i); u[m] is the move
 *   uniform of ply m.
 *
 * az_rng_philox_tape (host, needs no GPU) writes one game's tape with that sampler compiled for the host: plies
 * 0 .. max_plies - 1 (all n*n for max_plies <= 0 or >= n*n); noise may be NULL (the uniforms alone).  AZ_ERR_INVALID for a
 * board size outside 1..15, a kind other than the two, a null u, or an alpha that is not positive and finite.
 * az_rng_philox_tape_device runs the kernel on its own for games seed0 + 0 .. games - 1 on the engine's board size and copies
 * the result back: noise_out[games][sum_{m<plies} (n*n - m)] (may be NULL), u_out[games][n*n] (entries from max_plies on
 * are 0).  AZ_ERR_STATE while an episode is open. */
enum { AZ_RNG_NUMPY = 0, AZ_RNG_PHILOX = 1 };
enum { AZ_TAPE_DIRICHLET = 0, AZ_TAPE_GUMBEL = 1 };
#define AZ_RNG_PHILOX_ATTEMPTS 64
int az_set_rng(az_engine *e, int mode);
int az_get_rng(const az_engine *e);
void az_rng_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
double az_rng_log(double x);
double az_rng_exp(double x);
int az_rng_philox_tape(uint64_t seed, int board_size, double alpha, int max_plies, int kind, double *noise, double *u);
int az_rng_philox_tape_device(az_engine *e, uint64_t seed0, int games, double alpha, int max_plies, int kind, double *noise_out,
                              double *u_out);

/* Opt-in search upgrade the reference lists as a TODO (mcts.py:17-22 "subtree reuse", mcts.py:106 builds a new root
 * every run): after a self-play move the chosen child's subtree becomes the next ply's tree.  The retained root keeps
 * its priors and visit statistics, receives the ply's fresh Dirichlet sample with the arithmetic of a new root
 * (mcts.py:113-116), is NOT evaluated again, and the search runs only the simulations that top its children's visits
 * up to num_simulations, so pi is still a distribution over num_simulations visits.  Off by default: with it the visit
 * counts differ from the reference's (parity is then against the oracle's restatement of this rule, "parity
 * unpinned" by the reference).  Self-play only; arena games and az_search always start from a fresh root.  Needs
 * num_simulations <= 1023.  Not allowed while an episode is open. */
int az_set_subtree_reuse(az_engine *e, int on);

/* Opt-in: virtual-loss batching within a search, the third item of the reference's TODO list (mcts.py:17-22); its
 * simulation loop (mcts.py:123-141) is strictly sequential: select one leaf, evaluate it, back it up.  With `leaves` = L > 1
 * the num_simulations simulations of a search run in batches of L: the leaves of a batch are selected one after another
 * from the same tree, each selection counting the earlier ones of its batch as one visit that lost on every edge of their
 * paths (N + 1, W - 1 in mcts.py:73's formula), then the L leaves are evaluated together, and the simulations are
 * finished in selection order exactly like mcts.py:136-141 (the virtual visit is taken back first).  A selection that
 * ends on a leaf an earlier one of its batch is waiting on does not evaluate again: it backs up that leaf's value
 * (az_counters.duplicate_leaves).  Every search still makes exactly num_simulations simulations, in
 * ceil(num_simulations / L) dependent evaluation batches instead of num_simulations -- the lever for the latency-bound
 * uses (az_search, az_arena, episode tails).  Visit counts differ from the reference's sequential search, so parity is
 * against the oracle's restatement of this rule ("parity unpinned" by the reference); L = 1 is the reference's loop.
 * 1 <= leaves <= 32.  Combines with random-symmetry leaf evaluation; not with subtree reuse.  Not allowed while an episode
 * is open. */
int az_set_virtual_loss(az_engine *e, int leaves);

/* Opt-in: evaluation cache, the first item of the reference's TODO list (mcts.py:17 DEFAULT_CACHE_SIZE = 500_000,
 * mcts.py:22 "TODO: add caching").  A table in HBM keyed on what the net sees -- mover planes, opponent planes, last
 * move (games.py:86-129), which weight slot -- holding the net's raw outputs (policy logits, value-head hidden row).
 * A leaf or root whose position is in the table skips the conv trunk and the FC layers; the values are the very floats
 * those kernels would produce again, so visit counts, pi and moves are bit-identical with the cache on or off.
 * Shared by all lanes of the engine and kept across plies, games and episodes; every az_load_weights* call invalidates
 * it.  entries = 0 switches it off (and frees it); otherwise rounded up to a power of two, (96 + roundup(n*n, 64)) * 4
 * bytes each.  Hits are reported in az_counters.cache_lookups / cache_hits.  Not allowed while an episode is open. */
int az_set_eval_cache(az_engine *e, int64_t entries);

/* Delta evaluation, ON by default: within one ply a game's root does not change, and a leaf is the root plus
 * `depth` stones, so the trunk evaluates the root's stones once per ply and side to move (two base evaluations per active
 * slot) and every root and leaf of the ply only where its 3x3 / 5x5 / 7x7 footprints in the three conv layers differ from
 * them.  Every output element is the same k-ordered fma chain as in the full trunk: results are bit-identical with the
 * switch on or off.  A leaf with more than 8 changed cells, or with more conv3 tiles than az_delta_max_tiles, is evaluated
 * in full.
 * Serves the lock-step pipeline of the plain float32 trunk at 15x15 with one net and one leaf per game and batch
 * (az_selfplay*, az_search, az_search_batch); every other configuration -- other sizes, the ResidualBlock net, the
 * emulated trunks, the arena, virtual-loss batching, leaf symmetry, subtree reuse, the playout cap, deep searches above
 * 1024 simulations, the external evaluator, az_net_eval -- evaluates in full whatever the switch says.  Costs
 * 2 x 122 KB of HBM per slot, allocated by the first eligible episode.
 * az_set_delta_eval: AZ_ERR_STATE while an episode is open.
 * az_delta_max_tiles(e, tiles): sets the threshold (1 .. 15 conv3 tiles of 16 cells) and returns it; tiles = 0 only asks.
 * az_delta_stats: of the last (or open) episode or search call: evaluations on the delta path, evaluations in full on
 * an eligible episode (fallbacks), conv3 tiles computed on the delta path, base evaluations, and by_tiles[16]: the delta
 * evaluations by their conv3 tile count 0 .. 15.  Any pointer may be NULL.
 * az_net_eval_delta (tests, measurements): `count` positions evaluated as deltas from ONE root position (root[n*n] cells,
 * root_player to move there): outputs as az_net_eval, plus path[count]: the conv3 tiles the delta path computed for the
 * position, -1 when it was evaluated in full.  The positions need not be reachable from the root: what differs is what
 * is recomputed.  AZ_ERR_INVALID where no delta kernels exist (board size, net). */
int az_set_delta_eval(az_engine *e, int on);
int az_get_delta_eval(const az_engine *e);
int az_delta_max_tiles(az_engine *e, int tiles);
int az_delta_stats(const az_engine *e, int64_t *delta, int64_t *full, int64_t *tiles, int64_t *base, int64_t *by_tiles);
/* The integer logic of the delta path on the host (no GPU needed), n = 15 and at most 8 changed cells (AZ_ERR_INVALID
 * otherwise): the three tile lists -- wpos / cell [3][240]: padded-image position (r + 1) * 17 + c + 1 and board cell of every
 * tile lane of the 3x3 / 5x5 / 7x7 regions, cell 0xFFFF = a junk lane -- the two position lists halo [2][289] and the five
 * counts; entries behind a list's last tile read 0xEEEE.  conv2 runs on list 1, conv3 and the heads on list 2; conv1 is
 * recomputed on list 2 as well, so list 0 is only reported.  halo[0] (list 3) = the region conv1 computes plus
 * the ring positions it zeroes (nothing is copied there any more), halo[1] (list 4) = the positions of the base conv2 image
 * that are copied. */
int az_delta_lists(int n, int count, const uint8_t *changed, uint16_t *wpos, uint16_t *cell, uint16_t *halo, int32_t *cnt);
/* ... and the lists of a position evaluated in full by the delta kernel (more changed cells, or more conv3 tiles than
 * az_delta_max_tiles): every board cell in ascending position at all three layers, no window positions.  Same arrays. */
int az_delta_lists_full(int n, uint16_t *wpos, uint16_t *cell, uint16_t *halo, int32_t *cnt);
/* The changed cells of a leaf against its root, as the kernel finds them from the 16 board words: leaf[8] = the leaf's planes
 * (words 0-3 side to move, 4-7 opponent, bit c of word c / 64 = cell c), board[8] = the root's (words 0-3 X, 4-7 O), player =
 * the root's side to move (1 / 2), last = the leaf's last move or -1.  *count = changed cells (more than 8: the position is
 * evaluated in full), changed[8] = the first 8 in ascending order, 0xFF behind them, *parity = 0 where the root's mover is
 * to move at the leaf.  AZ_ERR_INVALID for n != 15, a NULL pointer, another player or a last move off the board. */
int az_delta_changed(int n, const uint64_t *leaf, const uint64_t *board, int player, int last, uint8_t *changed,
                     int32_t *count, int32_t *parity);
int az_net_eval_delta(az_engine *e, int slot, const uint8_t *root, int root_player, int count, const uint8_t *boards,
                      const uint8_t *players, const int16_t *lasts, float *logits, float *policy, float *value, int32_t *path);

/* Opt-in: random-symmetry leaf evaluation, the optional half of SURVEY §8f-2 (the reference's README.md:61,82 names the 8-fold
 * symmetry of the board, its code only uses it to augment the examples and leaves Gomoku.rot90 / flip unused,
 * games.py:183-197).  With it every net evaluation of a search -- the root (mcts.py:109) and each expanded leaf
 * (mcts.py:137) -- shows the net one of the 8 dihedral symmetries of the position and maps the policy back: priors of a
 * board cell = softmax entry of the image cell it was moved to; the value is taken as is.  The symmetry of evaluation idx
 * (0 = root, s + 1 = simulation s) of game g at ply p is a fixed hash of (low 32 bits of seed0 + g, p, idx) -- the game is
 * named by its seed, which a rank playing the id block [lo, hi) of a larger episode passes as seed0 + lo -- so runs are
 * reproducible and independent of slots, lanes and ranks (az_search / az_search_callback: key 0).  Visit counts differ from the reference's (its net always sees the position
 * unrotated); parity is against the oracle's restatement of this rule (orc_cfg.leaf_sym, "parity unpinned" by the
 * reference).  Lock-step pipeline and persistent search kernel alike; combines with virtual-loss batching (simulation s of a batch is evaluation s + 1 like
 * in the sequential loop), with the evaluation cache (the symmetry is part of the key: a hit is the evaluation under that
 * symmetry, records are unchanged) and with subtree reuse (a retained root is not evaluated again; simulation s stays
 * evaluation s + 1); az_search_callback evaluates positions as they are.  Not allowed while an episode is open. */
int az_set_leaf_symmetry(az_engine *e, int on);

/* Opt-in: start positions.  The reference always starts `Gomoku()` (self_play.py:50, evaluator.py:64); with count > 0 later
 * az_selfplay*, az_arena start their games from these positions instead of the empty board; count = 0 (pointers may be
 * NULL): back to the empty board.  Same position format as az_search_batch.  The definition: a game started from the
 * position that game g reached at ply m, with game g's seed, continues game g bit for bit.
 *   Self-play: game g starts from position (first + g) mod count.  Its ply is the number of stones on the board, side to
 *     move and last move are as given.  Everything indexed by ply keeps the ABSOLUTE ply -- the temperature table, the
 *     noise tape offset, u[g][ply], the explicit noise_tape / u_tape arguments, the leaf-symmetry hash, and max_plies (a
 *     game is cut once max_plies stones are on the board): a game whose first moves were forced.
 *   Arena: game g starts from position ((first + g) >> 1) mod count, for odd g with the colours exchanged (stones 1 <-> 2,
 *     side to move 3 - player): games 2i and 2i+1 are the same position with the nets on opposite sides (first even).
 *     The empty board with X to move gives the default arena.  Temperature temperature_table[(ply + 1) >> 1] and u by
 *     absolute ply.
 *   Records carry only searched plies: az_selfplay_games' nply[g] counts the plies searched = the records of game g;
 *     az_selfplay_records, az_selfplay_pack, az_dist_counts and az_dist_gather_records likewise, the first record of a
 *     game showing the start position with its `last`; az_arena's actions[g][0 .. nply[g]) are the moves played after the
 *     start position.  Counters: plies = records = root_evals (less retained roots) count searched plies.
 *   Checked on the host before anything is uploaded, by az_search_batch's rules (cell values, a legal action exists, last
 *     in range and on an occupied cell or -1, player 1 or 2) and one more: no line of win_length or more stones of either
 *     colour anywhere on the board (an already won position would be played on; under AZ_RULE_EXACT: no run of exactly win_length).  AZ_ERR_INVALID with the index of the first
 *     offending position in az_last_error; the previous setting is kept.  first >= 0.  AZ_ERR_STATE while an episode is
 *     open.  az_selfplay_begin / az_selfplay return AZ_ERR_INVALID when max_plies > 0 and some position already holds
 *     max_plies or more stones.
 * az_search, az_search_batch, az_search_callback, az_net_eval and az_rules_replay ignore the setting.  Combines with every
 * search option; with subtree reuse the first ply of a game has a fresh root. */
int az_set_start_positions(az_engine *e, int count, const uint8_t *boards /* [count][n*n] 0 / 1 X / 2 O */,
                           const uint8_t *players, const int16_t *lasts, int64_t first);
int az_get_start_positions(const az_engine *e);   /* count in force, 0 = none */

/* Opt-in: the win rule, i.e. which game is played.  AZ_RULE_FREESTYLE is the default and the reference's game (games.py:212-227):
 * a run of win_length OR MORE stones wins.  AZ_RULE_EXACT is standard Gomoku: the stone just placed wins when, in at least one
 * of the four directions, the maximal run of the mover's stones through it is EXACTLY win_length long; board edges end a run like
 * an empty cell.  A stone that makes an overline in one direction and an exact run in another wins; a stone that makes only
 * overlines does not, and the game goes on; a full board without a winner is a draw; the winner stays sticky.  A new exact run
 * must contain the new stone, so the kernels' test of the lines through the last stone stays sufficient under both rules.
 * The rule holds wherever the win test runs: every descent of the tree kernels, the game's own terminal test, az_selfplay*,
 * az_arena, az_search, az_search_batch, az_search_callback, az_rules_replay, the external evaluator path and deep engines; the
 * solver proves what the descent's win test finds, so it proves the game that is played.  It combines with every option:
 * there is no refused pair.  An engine whose rule is never set plays the reference's game bit for bit.
 * az_set_win_rule: AZ_ERR_INVALID for a rule other than 0 / 1; AZ_ERR_STATE while an episode is open, and when start positions
 * are set and the rule would change -- they were validated under the other rule: clear them (count = 0), set the rule, set them
 * again.  az_set_start_positions checks "already won" under the rule in force: under AZ_RULE_EXACT a position that holds only
 * overlines is a legal start, one that holds an exact run is refused.
 * az_rules_winner(board, n, k, rule) is a host-side helper (no engine, no GPU): a scan of the whole board[n*n] (0 empty, 1 X,
 * 2 O; 1 <= n <= 15, 1 <= k <= n) that returns AZ_RES_X / AZ_RES_O when that colour holds a winning run under `rule`, AZ_RES_DRAW
 * for a full board without one, AZ_RES_NONE otherwise, and AZ_ERR_INVALID for a bad argument or when both colours hold one. */
enum { AZ_RULE_FREESTYLE = 0, AZ_RULE_EXACT = 1 };
int az_set_win_rule(az_engine *e, int rule);
int az_get_win_rule(const az_engine *e);
int az_rules_winner(const uint8_t *board, int n, int k, int rule);

/* The search value per record, and opt-in resignation (AlphaGo Zero resigned below a value threshold and let a share of its
 * games play out to measure the false positives; the reference plays every game to the end, self_play.py:52-58).
 *
 * Search value of a ply.  After the search of a ply let a* be the legal cell with the largest root visit count N, the lowest
 * cell index on ties (the N that pi is made from, mcts.py:144-160).  v = W[a*] / (double)N[a*]: one IEEE float64 division of
 * the root row's own fields (az_search's `W` and `visits`), from the mover's point of view.  N[a*] >= 1: every ply ends with
 * num_simulations >= 1 visits under the root, retained roots of subtree reuse included.  (float)v is recorded for every
 * record of every episode, resignation on or off: az_selfplay_values returns it game-major then ply, in exactly the order
 * and count of az_selfplay_records; az_selfplay_pack_values writes the same floats to a DEVICE buffer in the order
 * az_selfplay_pack packs.  AZ_ERR_STATE without an episode.  The packed record format is unchanged, and the values of other
 * ranks are not exchanged: az_dist_gather_records carries the packed records only.
 *
 * Rule.  az_set_resign(threshold in (0, 1], min_ply >= 0, playout_permille in 0..1000); threshold = 0 switches resignation
 * off, which is the default.  A ply of game g CROSSES when ply >= min_ply (the absolute ply = stones on the board, as
 * everywhere) and v < -threshold, strictly, in float64.  Game g is EXEMPT when
 *     az_resign_mix(key(g)) % 1000 < playout_permille,
 * key(g) = the low 32 bits of seed0 + g, the global name of the game that the leaf-symmetry hash uses, so exemption does not
 * depend on slots, lanes or ranks (a rank playing the id block [lo, hi) passes seed0 + lo).  The move of a crossing ply is
 * made like any other: pi, the sampled action, the record, the move applied, the terminal test.  Then, if that move did not
 * end the game and the game is not exempt, the game ends with the opponent of the mover as winner: result = 3 - mover,
 * nply = ply + 1.  A natural end (win or full board) by that very move takes precedence; a cut by max_plies stays a cut
 * unless the ply crossed -- on a crossing ply the resignation is the result.
 *   Prefix property: a game played with resignation on is the same-seed game played with it off, truncated after its first
 *   crossing ply m: the records of plies 0..m are byte-identical, nply = m + 1, result = the other colour (z follows from the
 *   result as always).  An exempt game is the whole game, unchanged.
 * For every game the first crossing ply is kept, exempt games included: az_selfplay_resign_info gives cross_ply[g] (absolute
 * ply, -1 = none; all -1 while resignation is off) and exempt[g] (0 / 1) per game of the last episode; either may be NULL;
 * AZ_ERR_STATE without an episode, like az_selfplay_games.  The false-positive rate of a threshold is read from the exempt
 * games that crossed: those whose crossing side did not lose.
 * Applies to az_selfplay* and az_arena.  A resigned arena game shows in results[g] / nply[g] and in the tally like any other
 * decided game; NO arena game is exempt (playout_permille is ignored there; az_selfplay_resign_info after an arena reports
 * exempt = 0).  az_search, az_search_batch, az_search_callback, az_net_eval and az_rules_replay ignore the setting.  Combines
 * with every search option (evaluation cache, subtree reuse -- the slot of a resigned game starts its next game from a fresh
 * root --, virtual-loss batching, leaf symmetry, both nets, emulated trunks, deep engines, start positions) and with both
 * the lock-step pipeline and the persistent search kernel.  az_set_resign: AZ_ERR_INVALID for arguments out of range (the
 * previous setting is kept), AZ_ERR_STATE while an episode is open. */
/* mix, murmur3's 32-bit finaliser, in uint32_t arithmetic:
 *     x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16;
 * az_resign_mix and az_resign_exempt are host-side helpers (they need no GPU, like az_rng_*): the mix itself, and 1 / 0 for
 * whether the game named `key` is exempt under playout_permille. */
uint32_t az_resign_mix(uint32_t x);
int az_resign_exempt(uint32_t key, int playout_permille);
int az_set_resign(az_engine *e, double threshold, int min_ply, int playout_permille);
int az_get_resign(const az_engine *e, double *threshold, int *min_ply, int *playout_permille);
int az_selfplay_values(az_engine *e, float *values);
int az_selfplay_pack_values(az_engine *e, float *values_dev);
int az_selfplay_resign_info(az_engine *e, int32_t *cross_ply, uint8_t *exempt);

/* Opt-in playout cap randomisation (KataGo, Wu 2019: only a random share of the plies gets the full search and serves as a
 * policy target; the other plies are played with a small search that only moves the game along and feeds the outcome z).
 *
 * Rule.  az_set_playout_cap(fast_sims, full_permille, export_full_only).  fast_sims = 0 switches the cap off, which is the
 * default; the other arguments are then ignored.  Otherwise 1 <= fast_sims <= num_simulations, 0 <= full_permille <= 1000
 * and export_full_only in {0, 1}.  Ply p of game g is FULL when
 *     az_resign_mix(key(g) ^ az_resign_mix((uint32_t)p + 0x9E3779B9u)) % 1000 < full_permille,
 * p = the absolute ply (stones on the board, as everywhere), key(g) = the low 32 bits of seed0 + g, the global name of the
 * game that the leaf-symmetry hash and the resignation exemption use: fullness does not depend on slots, lanes, ranks,
 * compaction or refill order.  az_playout_cap_full(key, ply, full_permille) is the host-side helper (no GPU needed): 1 / 0.
 *   A FULL ply is the search as without the cap: num_simulations simulations and the ply's root noise from the tape.
 *   A FAST ply is the same search with fast_sims simulations and NO root noise: the priors are used as az_search(noise =
 *   NULL) and the arena use them.  The ply's noise on the tape is generated and skipped: everything indexed by ply stays
 *   where it is (the noise offsets, u[g][ply], the temperature table, explicit noise_tape / u_tape arguments).  pi, the
 *   sampled action, the record, the search value W[a*] / N[a*], the resignation test and the terminal test are made exactly
 *   as for any ply, from a root with fast_sims visits.
 * So full_permille = 1000 is the episode with the cap off, byte for byte, and fast_sims = num_simulations differs from it
 * only by the missing noise on the FAST plies.
 * Applies to az_selfplay and az_selfplay_begin / _step / _end only; az_arena, az_search, az_search_batch,
 * az_search_callback, az_net_eval and az_rules_replay ignore the setting.  Combines with virtual-loss batching (a slot
 * selects min(L, budget - done) leaves per batch and none once done >= budget: what a search with num_simulations = budget
 * does), the evaluation cache, leaf symmetry (evaluation index s + 1 is simulation s, as always), both nets, the synthetic
 * evaluator, the emulated trunks, deep engines, start positions, resignation and max_plies.  Refused with AZ_ERR_INVALID,
 * whichever is set first: subtree reuse (a retained root can already hold more than fast_sims visits) and the external
 * evaluator.  While the cap is on the persistent search kernel is never chosen (az_get_persistent == 0).
 * AZ_ERR_INVALID for arguments out of range (the previous setting is kept), AZ_ERR_STATE while an episode is open.
 *
 * Records.  Every ply, FAST or FULL, is a record as always and z is valid for all of them: az_selfplay_games, _records,
 * _values and _resign_info are unchanged in order and count.  az_selfplay_sims returns the simulations of every record,
 * game-major then ply, in exactly the order and count of az_selfplay_records (every entry num_simulations with the cap
 * off); AZ_ERR_STATE without an episode.  The device keeps no per-record array for it: the host restates the rule above
 * from the episode's seed0, each game's first ply and its length.
 * Export.  With export_full_only = 1, az_selfplay_pack, az_selfplay_pack_values, az_dist_counts and
 * az_dist_gather_records carry the records of FULL plies only, in their usual order; with 0 they carry every record and the
 * caller filters by az_selfplay_sims.  az_selfplay_export_count returns how many records az_selfplay_pack writes, cap on or
 * off.  The packed record format is unchanged.
 * Counters.  simulations is the sum of the budgets actually run; root_evals, plies and records are as always; steps counts
 * the evaluation batches actually launched per lane (a ply without a FULL slot launches only the FAST search's batches). */
int az_playout_cap_full(uint32_t key, int ply, int full_permille);
int az_set_playout_cap(az_engine *e, int fast_sims, int full_permille, int export_full_only);
int az_get_playout_cap(const az_engine *e, int *fast_sims, int *full_permille, int *export_full_only);
int az_selfplay_sims(az_engine *e, int32_t *sims);
int az_selfplay_export_count(az_engine *e, int64_t *records);

/* Opt-in forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2: every noised root child is guaranteed a
 * number of visits that grows with the square root of its prior and of the search so far, and the policy target afterwards
 * drops those visits again unless the search confirmed the move by its own PUCT logic).
 *
 * Rule.  az_set_forced_playouts(k, prune).  k = 0 switches the option off, which is the default; otherwise 0 < k <= 16
 * (KataGo: 2) and prune in {0, 1}.  It applies in every search whose root priors receive Dirichlet noise, and only at that
 * root: the self-play plies that are not FAST plies of the playout cap, and az_search / az_search_batch /
 * az_search_callback with noise != NULL.  az_arena, FAST plies and searches without noise are untouched, byte for byte;
 * below the root selection is unchanged.
 *   Forced selection.  At the root a legal child c is forced when
 *       (double)n * (double)n < (k * (double)P[c]) * (double)total,
 *   P[c] = the noised float32 prior of the root edge, n = the visit count its PUCT value uses (N, or N + in-flight visits
 *   under virtual-loss batching), total = the parent count the selection uses (the simulations finished so far; + j for item
 *   j of a virtual-loss batch).  A forced child scores +infinity instead of its PUCT value, and the usual order rule -- the
 *   first maximum in row-major order -- picks the lowest forced cell.  No square root is taken: the test is exact in float64.
 *   Pruning (prune = 1, after the search).  total = the sum of the root children's visits, sq = sqrt(total + 1e-8) as the
 *   selection uses it, c* = the most visited legal cell (the lowest on ties), score(c, m) = Q_c + ((c_puct * (double)P[c]) *
 *   sq) / (double)(1 + m) with Q_c = W_c / N_c held fixed, target = score(c*, N_c*).  For every other legal child with
 *   N_c > 0: F_c = the smallest integer m >= 0 with (double)m * m >= (k * (double)P[c]) * (double)total; lo = max(0, N_c -
 *   F_c); N'_c = the smallest m in [lo, N_c] with score(c, m) < target, or N_c when score(c, N_c) >= target; and N'_c = 1 <
 *   N_c becomes 0.  N'_c* = N_c*; children without visits keep 0.  pi and the sampled action are made from N' exactly as
 *   they are made from N without the option.  Everything else stays on the raw counts: the record's visits, the visits / W /
 *   prior outputs of the searches, the search value W[a*] / N[a*], the resignation test and the counters.
 *   With prune = 0 only the forced selection is active.
 * az_forced_prune(k, c_puct, count, visits, W, prior, out) restates the pruning on the host for one root row of `count` legal
 * children (no GPU needed): it writes N' to out[0 .. count) and returns the number of visits removed, or -1 for a bad
 * argument (k outside (0, 16], count < 1, a null pointer, a negative count, or no visit at all).
 * Combines with virtual-loss batching, the evaluation cache, leaf symmetry, both nets, the emulated trunks, the synthetic
 * evaluator, deep engines, the external evaluator, start positions, resignation, max_plies, the playout cap (FULL plies
 * only get the rule) and the persistent search kernel, which stays in use.  Refused with AZ_ERR_INVALID, whichever is set
 * first: subtree reuse (a retained root's carried visits were not made under the rule).
 * AZ_ERR_INVALID for arguments out of range (the previous setting is kept), AZ_ERR_STATE while an episode is open. */
int az_set_forced_playouts(az_engine *e, double k, int prune);
int az_get_forced_playouts(const az_engine *e, double *k, int *prune);
int64_t az_forced_prune(double k, double c_puct, int count, const int32_t *visits, const double *W, const float *prior, int32_t *out);

/* Opt-in selection rule: first-play urgency (Leela Zero, KataGo) and AlphaZero's visit-dependent c_puct.  The reference scores
 * a child Q + ((c_puct P) sqrt(Np + 1e-8)) / (1 + N) with Q = 0 while the child is unvisited and one constant c_puct; with
 * the option on an unvisited child is worth its parent's value less a reduction that grows with the prior mass already
 * visited, and c_puct grows with the parent's count.  Whether this trains a stronger net per GPU hour has not been measured.
 *
 * Rule.  az_set_selection(on, fpu, fpu_root, cpuct_base, cpuct_factor).  on = 0 switches the option off, which is the default
 * (the other arguments are then ignored and the stored ones kept); every search is then the reference's, executed by the
 * kernels that run it without this option.  With on = 1, at a node X whose children are scored:
 *   nv_c, wv_c = the child's count and total as the selection uses them: N and W, or N + in-flight and W - in-flight under
 *   virtual-loss batching.  A child is visited when nv_c > 0.
 *   mass = the sum over the visited legal children of (uint32) floor((double)P_c * 2^24), P_c the edge's float32 prior as stored
 *   (noised at a noised root): an integer, so the sum has no order.  idx = min(mass >> 12, 4096).
 *   red = r_X * mass_table[idx], mass_table[i] = sqrt(i / 4096.0) for i = 0..4096; r_X = fpu_root at the root, fpu elsewhere.
 *   V_X = the node's value for its side to move: at the root (double) of the float32 value the root's evaluation gave (the net,
 *   a cache hit, the synthetic or an external evaluator); elsewhere -Q_sel, Q_sel = the Q the level above computed for the
 *   edge it chose (always a visited one: a row exists only after a backup).
 *   Q_c = nv_c > 0 ? wv_c / nv_c : V_X - red       (the product and the difference are two float64 operations)
 *   score = Q_c + ((c(Np) * P_c) * sqrt(Np + 1e-8)) / (1 + nv_c), c(Np) = cpuct_table[Np] with the count the sqrt takes,
 *   cpuct_table[i] = c_puct + cpuct_factor * log((i + cpuct_base + 1.0) / cpuct_base) for i = 0..S+1 (std::log on the host);
 *   cpuct_factor = 0 gives c_puct exactly in every entry.
 *   Forced playouts: the pruning's score(c, m) and target take c(total) for c_puct, total the count its sqrt takes; the forced
 *   test n^2 < (k P) total, pi, the sampled move and the search value keep their definitions.
 * az_selection_tables(c_puct, cpuct_base, cpuct_factor, S, cpuct, mass) writes the two tables exactly as the engine uploads
 * them, cpuct[0 .. S+1] and mass[0 .. 4096] (host only, no engine needed); AZ_ERR_INVALID for a bad argument.
 * While the option is on every board size runs the lock-step kernels (az_get_persistent reports 0); switching it off brings
 * the persistent search kernel back.
 * Combines with virtual-loss batching, the evaluation cache, leaf symmetry, both nets, the synthetic evaluator, deep engines,
 * the external evaluator, start positions, resignation, the playout cap (a FAST ply's un-noised root uses fpu_root like any
 * root), forced playouts, the exact win rule and delta evaluation.  Refused with AZ_ERR_INVALID, whichever is set first:
 * subtree reuse (a retained root has no fresh value), the solver and with it the threat search (their kernels do not carry
 * the rule), the Gumbel root search.
 * AZ_ERR_INVALID unless fpu and fpu_root are finite and in [0, 2], cpuct_factor finite and in [0, 16], cpuct_base finite and
 * >= 1 (the previous setting is kept); AZ_ERR_STATE while an episode is open. */
int az_set_selection(az_engine *e, int on, double fpu, double fpu_root, double cpuct_base, double cpuct_factor);
int az_get_selection(const az_engine *e, int *on, double *fpu, double *fpu_root, double *cpuct_base, double *cpuct_factor);
int az_selection_tables(double c_puct, double cpuct_base, double cpuct_factor, int S, double *cpuct, double *mass);

/* Opt-in candidate moves: the search considers only the empty cells near the stones, and priors are normalised over them.
 * Every node of the reference's tree has one selectable edge per empty cell, up to 225 at 15x15, and its priors are a softmax
 * over all n^2 logits (controller.py:49), occupied cells included.  Whether this trains a stronger net per GPU hour has not
 * been measured.
 *
 * Rule.  az_set_candidates(e, radius) takes radius 0 (off, the default) or 1 .. n-1.  The candidate set C(X) of a node X with
 * position B (the stones of both colours, those placed along the descent included):
 *   B empty: C(X) = all n^2 cells.
 *   otherwise: C(X) = the empty cells whose Chebyshev distance to some stone of B is <= radius, max(|drow|, |dcol|) <= radius,
 *   with no wrap across row ends.  A board that is neither empty nor full always has a candidate (the 8-neighbour grid is
 *   connected), so radius = n-1 is "all legal cells": the legal-move-masked softmax on its own.
 * C(X) depends on the position alone; it is not stored with the row.
 * Expansion of X (root or leaf), x the logits in board order (after the leaf symmetry has been undone):
 *   m   = max over c in C of x_c
 *   e_c = expf_c (x_c - m)                     c in C; expf_c: the engine's canonical float32 exp (az_expf of csrc/az_device.h)
 *   s   = canonical wave sum of e_c             float32: lane l adds its cells j = l (mod 64), j in C, in ascending order;
 *                                               then v[l] = v[l] + v[l ^ msk] for msk = 32, 16, 8, 4, 2, 1
 *   P_c = e_c / s  (c in C),   P_c = 0.0f exactly  (c not in C)
 * i.e. the softmax of every expansion with "j < n^2" replaced by "j in C".  The value head is untouched.  The synthetic
 * evaluator has no logits and is not normalised: candidates keep their prior, every other cell gets 0.
 * Root noise, where the root is noised today; the tape and its offsets are unchanged.  nz_c = noise[legal_rank(c)], legal_rank
 * the index among the empty cells as today:
 *   t    = canonical wave sum over c in C of nz_c      float64, the same lane partials and butterfly
 *   P'_c = (float)((double)((float)(1-w) * P_c) + w * (nz_c / t))      c in C; nothing is fused
 * (a sub-vector of a Dirichlet(alpha) sample, renormalised, is Dirichlet(alpha) on the subset).  Non-candidates stay at 0.
 * Selection, at every level and with or without virtual-loss batching: the argmax runs over C(X) instead of over the empty
 * cells; the expression, the operation order and the tie-break (first maximum in cell order) do not change.  A non-candidate
 * edge is never selected and keeps N = 0; pi gives it what it gives any legal cell with no visit.
 * The terminal tests, backup, the move, the search value, resignation, the temperature schedule and the records' layout keep
 * their definitions.  Forced playouts: a child with P = 0 is never forced (n^2 < (k P) total is false), and the pruning only
 * touches children with a visit.
 * az_candidate_mask(n, board, radius, mask) is the rule on the host (no engine needed): board uint8[n*n] 0 empty / 1 / 2,
 * mask[j] = 1 for the cells of C; radius 0 gives the empty cells (the option off).  AZ_ERR_INVALID for n outside 3..15, radius
 * outside 0 .. n-1, a cell value above 2 or a null pointer.
 * Off -- never set, or set back to 0 -- the engine is the one without the option byte for byte, run by the kernels that run
 * it without.  While the option is on every board size runs the lock-step kernels (az_get_persistent reports 0).
 * Combines with the evaluation cache (entries hold logits: they serve both settings), leaf symmetry, virtual-loss batching,
 * deep engines, both nets, the synthetic evaluator, start positions, resignation, the exact win rule, the playout cap, forced
 * playouts, delta evaluation, az_search / az_search_batch and both step APIs.  Refused with AZ_ERR_INVALID, whichever is set
 * first: subtree reuse (a retained root's priors and noise were not made under the rule for this position), the Gumbel root
 * search (top-m and the completed-Q target are defined over the legal cells), the solver and with it the threat search
 * ("every move loses" is no proof when moves were left out), the selection rule (its kernels do not carry this one yet), the
 * external evaluator (it returns priors, not logits); az_search_callback refuses the option itself.
 * AZ_ERR_INVALID for a radius outside 0 .. n-1 (the previous setting is kept); AZ_ERR_STATE while an episode is open. */
int az_set_candidates(az_engine *e, int radius);
int az_get_candidates(const az_engine *e, int *radius);
int az_candidate_mask(int n, const uint8_t *board, int radius, uint8_t *mask);

/* Opt-in Gumbel root search ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022): instead of Dirichlet
 * noise, PUCT at the root and the visit-count target, the root samples Gumbel-top-m candidates without replacement, spends a
 * fixed sequential-halving schedule on them and trains on softmax(logits + sigma(completed Q)).  Made for 16 to 64 simulations
 * per move.  Values are in [-1, 1] from the mover's side; there is no min-max rescaling.
 *
 * Rule.  az_set_gumbel(m, c_visit, c_scale).  m = 0 switches the option off, which is the default; otherwise
 * 1 <= m <= min(n * n, 64), c_visit >= 0 and c_scale > 0, both finite (the paper: m = 16, c_visit = 50, c_scale = 1).  It
 * applies in every search whose root would receive Dirichlet noise, and only at that root: the self-play plies that are not
 * FAST plies of the playout cap, and az_search / az_search_batch with noise != NULL.  az_arena, FAST plies and searches without
 * noise are untouched, byte for byte; below the root the search stays PUCT exactly as it is.
 *   Noise.  At such a root the noise values are not mixed into the priors: the edge keeps the plain float32 softmax prior.  The
 *   noise values are read as Gumbel(0, 1) draws g over the legal cells in row-major order -- same place, stride and offsets as
 *   the Dirichlet sample.  An episode begun with the option on fills the tapes it generates itself with
 *   RandomState(seed0 + game).gumbel() draws (az_rng_selfplay_tape_gumbel: per ply p, n * n - p draws, then one uniform); an
 *   explicit noise_tape is taken as given.  The uniforms of a generated tape are therefore not those of the Dirichlet tape of
 *   the same seed (a Gumbel draw takes one random_sample, a Dirichlet sample a varying number): the FAST plies of a capped
 *   episode are searched as without the option, but on generated tapes they sample their moves with other uniforms.
 *   Schedule, a pure function of (k, S) (az_gumbel_schedule).  For k <= 1 it is 0, 1, .., S - 1.  Otherwise L = ceil(log2 k),
 *   visits[0 .. k) = 0, c = k; until S entries exist: extra = max(1, S / (L * c)) in integers; extra times: append
 *   visits[0 .. c), then increment those c entries; then c = max(2, c / 2).  Truncated to S entries.  seq_k[t] is the visit
 *   count a root child must have to be selectable at simulation t.  A root uses k = min(m, number of legal cells).
 *   Root selection at simulation t (t = the simulations finished so far).  maxN = the largest visit count among the legal root
 *   children before this simulation; sig = (c_visit + (double)maxN) * c_scale; h_c = (double)g[rank(c)] + (double)logit_c, one
 *   float64 add, logit_c the float32 logit the softmax consumes (read through the leaf symmetry where that option is on);
 *   q_c = W_c / N_c, or 0.0 when unvisited; score_c = h_c + sig * q_c with a separate multiply and add.  Among the legal cells
 *   with N_c == seq_k[t] the first maximum in row-major order is taken.  The candidates of one simulation have equal N, so
 *   every selection is exact in float64.
 *   Move.  After the last simulation: among the legal cells with N_c == maxN, the first maximum of score_c.  Temperature and u
 *   are not used on such a ply (the tape still carries u).
 *   Policy target.  v0 = the root's float32 value, widened.  Over the legal cells in row-major order, with float64 pairwise
 *   sums in np.add.reduce order: sumN = sum N_c; pv = sum (double)P_c over the visited cells (unvisited ones add 0.0);
 *   pq = sum (double)P_c * q_c likewise; v_mix = (v0 + (sumN / pv) * pq) / (1 + sumN); qh_c = q_c if visited, else v_mix;
 *   y_c = (double)logit_c + sig * qh_c with sig from the final maxN; pi_c = exp(y_c - max y) / sum, the exp and the pairwise
 *   sum being those of the temperature path, stored as float32.  The record's pi and the pi output of the searches is this.
 *   Everything else stays on the raw tree as without the option: visits, W, prior (the unmixed softmax), the search value
 *   W[a*] / N[a*] of the most visited cell, resignation, the counters.
 * az_gumbel_schedule(k, S, out) writes seq_k[0 .. S) (no GPU needed).  az_gumbel_target(count, logits, g, visits, W, prior,
 * root_value, c_visit, c_scale, pi, action) restates move and policy target on the host for one root row of `count` legal
 * children with the functions the kernel uses: pi[0 .. count) and the index of the chosen child.  Both return AZ_ERR_INVALID for
 * a bad argument (a null pointer, count outside 1 .. 225, a count outside 0 .. 65535, no visit at all, constants out of range).
 * Combines with the evaluation cache, leaf symmetry, both nets, the emulated trunks, deep engines, start positions,
 * resignation, max_plies, the playout cap (FULL plies only get the rule), both step APIs and the persistent search kernel,
 * which stays in use.  Refused with AZ_ERR_INVALID, whichever is set first: subtree reuse, virtual-loss batching (in-flight
 * counts under the equal-N gate need a definition of their own), forced playouts (both rules own the root selection), the
 * external evaluator (it returns priors, not logits) and engines created with AZ_EVAL_SYNTHETIC; az_search_callback with noise
 * and the option set returns AZ_ERR_INVALID as well.
 * AZ_ERR_INVALID for arguments out of range (the previous setting is kept), AZ_ERR_STATE while an episode is open. */
int az_set_gumbel(az_engine *e, int m, double c_visit, double c_scale);
int az_get_gumbel(const az_engine *e, int *m, double *c_visit, double *c_scale);
int az_gumbel_schedule(int k, int S, int32_t *out);
int az_gumbel_target(int count, const float *logits, const double *g, const int32_t *visits, const double *W, const float *prior,
                     float root_value, double c_visit, double c_scale, float *pi, int32_t *action);
/* v_mix alone, as az_gumbel_target forms it: NaN for a bad argument */
double az_gumbel_vmix(int count, const int32_t *visits, const double *W, const float *prior, float root_value);

/* Opt-in MCTS-Solver (Winands, Bjornsson, Saito 2008): proven wins, losses and draws in the search tree.  The reference's
 * mcts.py has nothing of the kind; off by default, and with the option off nothing below is read, written or executed.
 *
 * Rule.  Every edge has a status, seen from the side that makes the move: */
enum { AZ_PROOF_UNKNOWN = 0, AZ_PROOF_WIN = 1, AZ_PROOF_LOSS = 2, AZ_PROOF_DRAW = 3 };
/* A node's status, seen from its side to move, is computed over its legal cells (the empty cells at that node): WIN if any
 * edge is WIN; otherwise, if every legal edge is proven, DRAW if any edge is DRAW, else LOSS; otherwise UNKNOWN.
 * With az_set_solver(e, 1) every search applies the rule -- self-play, arena, az_search and az_search_batch, with or without
 * root noise, the FULL and the FAST plies of the playout cap alike.  In one simulation:
 *   Selection, at every level and at the root.  The scores are the PUCT scores.  A WIN edge then scores +infinity, and a LOSS
 *   edge -infinity provided the row has at least one legal edge that is not LOSS; if every legal edge is LOSS (the root only)
 *   the plain scores decide.  The first maximum in row-major order is taken, as without the option.
 *   After the move the real terminal tests come first (a line through the stone, a full board).  If neither holds and the
 *   edge's status is not UNKNOWN the simulation ends on that edge: no evaluation is made, no row is allocated, and it backs
 *   up -1 for a WIN edge, +1 for a LOSS edge and 0 for a DRAW edge as the value of the side to move below the edge; it counts
 *   as a terminal hit (az_counters.terminal_hits).  Otherwise the simulation expands or descends.
 *   Backup is unchanged.
 *   Marking, only when the simulation ended on a real terminal whose edge was UNKNOWN: that edge becomes WIN for the mover
 *   if the move made the line, DRAW if it filled the board.  Then, walking the path upwards: the status of the node that
 *   owns the edge is computed; if it is UNKNOWN the walk stops; otherwise the edge above it gets the negated status (WIN
 *   and LOSS swap, DRAW stays), and at the top the root's own status is kept.  A proven edge is never descended through,
 *   so the walk never meets an edge that is already proven.
 * At the end of the search, with st the root row's statuses, pi and the sampled move are made from the count vector N': if
 * any root edge is WIN, the counts of the WIN edges and 0 elsewhere (a WIN edge has at least one visit); otherwise, if some
 * legal edge that is not LOSS has a visit, 0 on the LOSS edges; otherwise the raw counts.  The temperature / cumsum /
 * searchsorted path is unchanged, and the record's visits stay the raw ones.  The record's value (az_selfplay_values) is
 * exactly +1, -1 or 0 when the root is proven WIN, LOSS or DRAW, else W[a*] / N[a*] as always; resignation reads it
 * unchanged, so a proven loss resigns by itself.  The number of simulations stays num_simulations (no early out), games are
 * played to their real end, z is unchanged.
 *
 * az_last_proof(e, capacity, edges, roots, count): after az_search, edges[n*n] and roots[1]; after az_search_batch,
 * edges[positions][n*n] and roots[positions] -- the root row's statuses (0 on occupied cells) and the root's status.  *count
 * receives the number of positions the engine holds (1 after az_search); capacity is the number of positions the caller's
 * buffers hold, and a call with a buffer and capacity < *count writes nothing but *count and returns AZ_ERR_INVALID.  Any
 * pointer may be NULL (edges = roots = NULL asks for the count).  AZ_ERR_STATE when the last search or episode on the engine
 * was not such a search with the solver on.
 * az_solver_stops(e, stops): the simulations of the last (or open) episode, az_search or az_search_batch call that ended on
 * a proven edge (they are terminal hits in az_counters as well); 0 with the option off.  az_selfplay_proofs(e, roots): the root status of every record of the last episode, indexed like
 * az_selfplay_values; AZ_ERR_STATE without an episode or when it ran without the solver.
 * az_solver_counts(count, visits, status, out) restates N' on the host for one root row of `count` legal children with the
 * function the kernel uses (no GPU needed); AZ_ERR_INVALID for a null pointer, count < 1, a negative visit count or a
 * status outside 0 .. 3.
 * Combines with both nets, the evaluation cache, leaf symmetry, the emulated trunks, deep engines, start positions,
 * resignation, max_plies, the playout cap, the arena, az_search_batch and the step API (az_selfplay_begin / _step / _end).  Refused with AZ_ERR_INVALID,
 * whichever is set first: subtree reuse, virtual-loss batching, forced playouts, the Gumbel root search, the batched external
 * evaluator (az_set_external_evaluator: refused, not supported) and engines created with AZ_EVAL_SYNTHETIC;
 * az_search_callback with the option set returns AZ_ERR_INVALID as well.  The persistent search kernel serves the solver
 * with one status byte per edge behind the edges in LDS; where the rows and the bytes of a configuration do not fit together
 * the searches run on the lock-step pipeline (az_get_persistent says which).
 * AZ_ERR_INVALID for on outside 0 / 1, AZ_ERR_STATE while an episode is open. */
int az_set_solver(az_engine *e, int on);
int az_get_solver(const az_engine *e);
int az_last_proof(az_engine *e, int capacity, int8_t *edges, int8_t *roots, int32_t *count);
int az_solver_stops(const az_engine *e, int64_t *stops);
int az_selfplay_proofs(az_engine *e, int8_t *roots);
int az_solver_counts(int count, const int32_t *visits, const int8_t *status, int32_t *out);

/* Opt-in root threat search: forced-four wins ("victory by continuous fours", VCF) and forced blocks, proven exactly over the
 * rules of the game by a kernel of its own (csrc/az_threat.h) on every root before the simulations, and handed to the solver as
 * premarked root statuses.  The solver alone proves only what the search happens to reach; this widens it at the root.  Off by
 * default, and with the option off nothing below is read, written or executed.
 *
 * Rule.  For a position P with side to move A and opponent D, win(P, c) is the set of empty cells where a stone of colour c
 * wins at once under the win rule in force (az_set_win_rule).  Cells are taken in ascending row-major order.  T(P, d) returns
 * (found, move, depth) and counts nodes in one counter shared by the whole search of a root:
 *   1. Wa = win(P, A).  If it is non-empty: found, move = the lowest cell of Wa, depth 1.
 *   2. If d <= 1: not found.
 *   3. Wd = win(P, D).  If |Wd| >= 2: not found.  The candidates are the single cell of Wd if |Wd| == 1, otherwise every empty
 *      cell.
 *   4. For each candidate x in ascending order: P' = P + A at x, W = win(P', A).  If W is empty x is not a four: it is skipped
 *      and counts no node.  Otherwise nodes += 1; if nodes > node_budget the whole search of this root ends "exhausted" and no
 *      win is reported.  If win(P', D) is non-empty x is skipped (D wins instead of blocking).  If |W| >= 2: found, move x,
 *      depth 2.  Otherwise let w be the single cell of W, P'' = P' + D at w and r = T(P'', d - 1); if r is found: found, move x,
 *      depth r.depth + 1.
 *   5. Not found.
 * The depth is that of the line found, not necessarily the shortest.  The root search is T(root, max_depth).
 * Root statuses, AZ_PROOF_* seen from the mover.  A win found at step 1: every cell of Wa is WIN and the root is WIN.  A win
 * found deeper: the edge `move` is WIN and the root is WIN.  Otherwise, exhausted searches included, if Wd of the root is
 * non-empty: every legal cell outside Wd is LOSS; with |Wd| >= 2 the cells of Wd are LOSS too and the root is LOSS; with
 * |Wd| == 1 that cell stays UNKNOWN.  Everything else is UNKNOWN.  The root's Wd is computed before any node is counted, so
 * these marks do not depend on the budget.
 * Soundness.  A WIN of depth d means A wins within 2d - 1 plies against any defence; a LOSS edge means D completes a line on
 * the next move.  Both hold under both win rules: a stone of the other colour on an empty cell never changes a maximal run
 * of one's own stones.
 *
 * az_set_threat_search(e, max_depth, node_budget): max_depth = 0 is off (the default); otherwise 1 <= max_depth <=
 * AZ_THREAT_MAX_DEPTH and 1 <= node_budget <= 65535.  It needs the solver: AZ_ERR_INVALID while az_get_solver(e) == 0, and
 * az_set_solver(e, 0) while it is on is refused with AZ_ERR_INVALID (switch the threat search off first).  It inherits the
 * solver's refused pairs and adds none.  With it on, every search the solver serves -- self-play, arena, az_search and
 * az_search_batch, FULL and FAST plies alike -- runs the kernel over the active slots after the roots are set up and before the
 * root expansion, and the root row and the root start from the premarked statuses instead of UNKNOWN.  From there on the
 * solver's rule as written does the rest: a WIN edge scores +infinity, a descent onto a premarked WIN edge that is not a real
 * terminal ends there (no evaluation, no row), pi is made from the WIN edges' counts, the record's value is exactly +1 / -1, a
 * proven loss resigns by itself.  The root is still evaluated once.  While the option is on the persistent search kernel is
 * never chosen (az_get_persistent == 0), as under the playout cap.  AZ_ERR_STATE while an episode is open; arguments out of range keep the
 * previous setting.
 * az_threat_batch(e, count, boards, players, max_depth, node_budget, status, move, depth, nodes, edges): the kernel on its
 * own, for analysis and tests; it searches any number of positions in waves of the engine's slots and ignores the setter.
 * status[count] = the root status, move[count] = the winning move or -1, depth[count] = the depth or 0, nodes[count] (the search
 * was exhausted iff nodes > node_budget), edges[count][n*n] (0 on occupied cells).  Any output may be NULL; count = 0 returns
 * AZ_OK.  Positions are checked on the host by az_search_batch's rules (without `last`) and must not already be won under the
 * rule in force (az_set_start_positions' check): AZ_ERR_INVALID with the index of the first offender in az_last_error.
 * AZ_ERR_STATE while an episode is open.
 * az_threat_solve(board, n, k, rule, player, max_depth, node_budget, move, depth, nodes, edges): the same on the host for one
 * position (no engine, no GPU, like az_rules_winner; 1 <= n <= 15, 1 <= k <= n).  Returns the root status, or AZ_ERR_INVALID
 * for a bad argument, a full board or a position already won.  move, depth, nodes, edges may be NULL.
 * az_selfplay_threats(e, depth): per record, in the order and count of az_selfplay_values, 0 = none, d = a win of depth d;
 * AZ_ERR_STATE without an episode or when it ran without the option.
 * az_threat_stats: over the last (or open) episode or the last az_search / az_search_batch call: roots proven WIN, roots proven
 * LOSS, roots with a single forced block and no win, exhausted searches, and nodes; any pointer may be NULL; 0 with the option
 * off. */
#define AZ_THREAT_MAX_DEPTH 16
int az_set_threat_search(az_engine *e, int max_depth, int node_budget);
int az_get_threat_search(const az_engine *e, int *max_depth, int *node_budget);
int az_threat_batch(az_engine *e, int count, const uint8_t *boards, const uint8_t *players, int max_depth, int node_budget,
                    int8_t *status, int32_t *move, int32_t *depth, int32_t *nodes, int8_t *edges);
int az_threat_solve(const uint8_t *board, int n, int k, int rule, int player, int max_depth, int node_budget,
                    int32_t *move, int32_t *depth, int32_t *nodes, int8_t *edges);
int az_selfplay_threats(az_engine *e, int8_t *depth);
int az_threat_stats(az_engine *e, int64_t *win_roots, int64_t *lost_roots, int64_t *block_roots, int64_t *exhausted, int64_t *nodes);

/* Opt-in: fp32-emulating conv trunks.  AZ_TRUNK_F32 (default) computes the net's forward (net.py:55-72) on the float32
 * matrix instruction in the build's canonical fp order: bit-identical to the oracle.  The other two run every conv but the
 * first (99 % of the net's arithmetic) and the 1x1 head convs on the 16 x faster 16-bit matrix instructions with split
 * operands and float32 accumulation:
 *   AZ_TRUNK_BF16X3  three bfloat16 parts per operand, the six largest cross products: float32's exponent range, 2.67 x
 *                    ceiling over the float32 instruction;
 *   AZ_TRUNK_F16X2   two float16 parts per operand (the low part scaled by 2^11), three cross products in two accumulators:
 *                    5.3 x ceiling; float16's range -- activations saturate at 65504 and a weight set with |w| >= 65504 is
 *                    refused (AZ_ERR_INVALID from this call or from the next az_load_weights*, which puts the engine back on
 *                    AZ_TRUNK_F32).  The saturation is silent: a net whose weights pass that check but whose activations
 *                    exceed 65504 gets clipped logits with no error.  At the low end the split resolves an operand to an
 *                    absolute ~2^-36 below |x| = 2^-14 (float16 subnormals) instead of the relative 2^-22 above it
 *                    (tests/numeric.py derives both terms of the bound).
 * Both give float32-like accuracy (|logit| 2e-5, |P| 1e-6, |value| 2e-6 against the oracle, the tolerances already granted
 * against the Python reference's torch numbers), NOT bit-identical results, so visit counts can differ from the reference's
 * on near-tied PUCT scores (measured: DESIGN.md section 4).  One kernel for every occupancy (no split / persistent variants),
 * so results do not depend on the slot count.  Both nets.  Invalidates the evaluation cache.  Not allowed while an episode
 * is open. */
int az_set_trunk_mode(az_engine *e, int mode);
int az_get_trunk_mode(const az_engine *e);
/* Host-side helper (needs no GPU, like az_rng_*): the 16-bit parts a weight is split into for `mode` -- bfloat16 hi, mid, lo
 * (x = hi + mid + lo) or float16 hi, lo (x = hi + lo / 2048) as raw bit patterns.  Returns the number of parts written, or
 * AZ_ERR_INVALID for an unknown mode or a value outside float16's range in AZ_TRUNK_F16X2. */
int az_emul_split(int mode, float x, uint16_t *parts);

/* HIP-event timing of every trunk / FC / tree-step launch (az_counters.trunk_seconds, nn_seconds, step_seconds);
 * off by default: four events per evaluation batch cost a few microseconds of stream time, which matters on small boards.
 * While it is on, the lanes of the engine play one after another instead of concurrently, so that every kernel is timed
 * alone on the GPU (roofline calibration). */
int az_set_profiling(az_engine *e, int on);

int az_get_counters(const az_engine *e, az_counters *out);

/* Number of lanes the engine runs (az_config.engines after the library's choice for 0). */
int az_get_lanes(const az_engine *e);

/* Which kernels ran the searches of the last (or the open) episode: 0 = the lock-step pipeline, one conv-trunk, FC and
 * tree launch per evaluation batch; g > 0 = the persistent search kernel (csrc/az_search.h), one launch per ply with g
 * games per workgroup and their trees resident in LDS.  The library picks the persistent kernel by itself whenever it
 * applies -- boards up to 7x7 whose (num_simulations + 1) tree rows fit into LDS, either net or the synthetic evaluator,
 * float32 trunk, no virtual-loss batching, at most 1024 simulations (the evaluation cache, subtree reuse and the leaf symmetry
 * it knows) -- because its results are bit-identical; AZ_PERSIST=0 in the environment keeps the lock-step pipeline. */
int az_get_persistent(const az_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* AZ_ENGINE_H */
