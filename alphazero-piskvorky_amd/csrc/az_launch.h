// az_launch.h -- per-board-size kernel launchers.  Every board size n = 3..15 is its own translation unit
// (az_kernels.hip compiled with -DAZ_N=n, in parallel); the engine dispatches through this table.
#pragma once
#include "az_net.h"
#include "az_net_emul.h"
#include "az_delta.h"
#include "az_search.h"
#include "az_batch.h"
#include "az_ext.h"
#include "az_threat.h"

struct LaunchCtx {
    hipStream_t stream;
    DevState d;         // the games' view: B = game slots
    DevState dv;        // the net kernels' view: B = evaluation items (slots x leaves per batch), s_status / s_net per item;
                        // identical to d unless virtual-loss batching is on
    NetWeights w[2];
    ResWeights rw[2];
    int model;          // AZ_MODEL_PLAIN | AZ_MODEL_RESNET
    int synthetic;      // AZ_EVAL_SYNTHETIC
    int persist_gp;     // games per workgroup of the persistent search kernel, 0 = lock-step pipeline (part of the graph key)
    int vl_kernel;      // the batched (virtual-loss) tree kernel is in use (part of the graph key)
    int emul;           // 0 | AZ_TRUNK_BF16X3 | AZ_TRUNK_F16X2: the convs on the 16-bit MFMA with split operands (az_net_emul.h)
    float *feat;
    unsigned long long *dbg;
    float *scratch;     // split-trunk images, SizeOps::split_floats_per_group floats per board group (or null)
    unsigned char *inflight;   // deep search (S > DEFAULT_MAX_S) with virtual-loss batching: in-flight count per edge [B][R][RW], else null
    // delta evaluation (az_delta.h, az_set_delta_eval; part of the graph key): null = off, every board through SizeOps::trunk
    float *delta_base;              // [slots][2] base images and feature rows of the running ply
    unsigned char *delta_done;      // [slots] the path of each board in the running batch: 0 in full, 1 + conv3 tiles as a delta
    unsigned long long *delta_cnt;  // [slots][DELTA_CNT] (az_delta.h)
    int delta_tiles;                // a board with more conv3 tiles than this is evaluated in full
};

struct SizeOps {
    void (*trunk)(const LaunchCtx &, int net_id);
    void (*trunk_split)(const LaunchCtx &, int net_id);     // same results as trunk, lower latency for few boards
    long long (*split_scratch_floats)(int slots, int model);
    void (*fc)(const LaunchCtx &, int net_id);
    void (*step)(const LaunchCtx &, int rootN, int do_select);
    void (*step_vl)(const LaunchCtx &, int sims_done, int nb_next);      // virtual-loss batching (DevState.L leaves per game)
    void (*root_cache)(const LaunchCtx &);                                // evaluation-cache lookup of the root positions
    // persistent search kernel (az_search.h): prepare returns 1 when `games` games per workgroup with S simulations fit
    // into LDS on the current device (and raises the kernel's dynamic-LDS limit), 0 when this size has no such kernel
    int (*search_prepare)(int S, int games, int synthetic, int model, int solver);
    void (*search)(const LaunchCtx &, int games);
    void (*move)(const LaunchCtx &);
    void (*eval_tail)(const LaunchCtx &, int count, float *policy, float *value);
    // az_search_batch (az_batch.h), one launch over the slots of every lane: the given positions into the slots, and after
    // the ply every slot's root row and record into compact [wave][n*n] staging (null outputs are skipped)
    void (*set_positions)(hipStream_t, const BatchLanes &, const unsigned char *cells, const unsigned char *players, const short *lasts);
    void (*gather_roots)(hipStream_t, const BatchLanes &, const DevState &, const unsigned char *cells, int *visits, double *W, float *prior, float *pi, int *action);
    // az_set_start_positions: `count` positions given as cells -> the table k_refill starts games from
    void (*build_positions)(hipStream_t, int count, const unsigned char *cells, const unsigned char *players, const short *lasts, StartPos *table);
    // az_set_external_evaluator (az_ext.h), over the items of one lane (LaunchCtx.dv): the items waiting for net `net` appended
    // to the request (first: a new request), and the evaluator's priors and values of `count` entries back into their rows
    void (*ext_gather)(const LaunchCtx &, int net, int item_base, int first, int capacity, float *planes, int *map, int *count);
    void (*ext_scatter)(const LaunchCtx &, int item_base, int count, const int *map, const float *policy, const float *value);
    // az_set_threat_search / az_threat_batch (az_threat.h): the root threat search of the first d.B slots, one wavefront each
    void (*threat)(const LaunchCtx &);
    // delta evaluation (az_delta.h), null where the size has none: the base evaluations of every active slot, once per ply; and
    // the trunk of one batch, bit-identical to trunk's
    void (*trunk_base)(const LaunchCtx &, int net_id);
    void (*trunk_delta)(const LaunchCtx &, int net_id);
    long long delta_floats_per_slot;
};

const SizeOps *az_size_ops(int n);     // nullptr for unsupported sizes
// weak: a development build may leave sizes out (make SIZES="5 9 15"); az_size_ops then returns nullptr for them
#define AZ_DECL_OPS(n) const SizeOps *az_size_ops_##n() __attribute__((weak));
AZ_DECL_OPS(3) AZ_DECL_OPS(4) AZ_DECL_OPS(5) AZ_DECL_OPS(6) AZ_DECL_OPS(7) AZ_DECL_OPS(8) AZ_DECL_OPS(9)
AZ_DECL_OPS(10) AZ_DECL_OPS(11) AZ_DECL_OPS(12) AZ_DECL_OPS(13) AZ_DECL_OPS(14) AZ_DECL_OPS(15)
