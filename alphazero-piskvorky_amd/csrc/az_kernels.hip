// az_kernels.hip -- the size-templated kernels instantiated for ONE board size (compile with -DAZ_N=n).
#include <hip/hip_runtime.h>
#include "az_launch.h"

#ifndef AZ_N
#error "compile with -DAZ_N=<board size>"
#endif
#define AZ_CAT2(a, b) a##b
#define AZ_CAT(a, b) AZ_CAT2(a, b)

namespace {
constexpr int N = AZ_N;

void trunk(const LaunchCtx &c, int net_id)
{
    if (c.model == 1) {
        typedef ResGeo<N> G;
        dim3 gt((c.dv.B + G::G - 1) / G::G), bt(G::NW * 64);
        if (c.emul == EMUL_BF16X3) hipLaunchKernelGGL((k_trunk_res_emul<N, EMUL_BF16X3>), gt, dim3(ResGeoEmul<N>::NW * 64), 0, c.stream, c.dv, c.rw[net_id], net_id, c.feat);
        else if (c.emul == EMUL_F16X2) hipLaunchKernelGGL((k_trunk_res_emul<N, EMUL_F16X2>), gt, dim3(ResGeoEmul<N>::NW * 64), 0, c.stream, c.dv, c.rw[net_id], net_id, c.feat);
        else hipLaunchKernelGGL(k_trunk_res<N>, gt, bt, 0, c.stream, c.dv, c.rw[net_id], net_id, c.feat);
    } else {
        typedef NetGeo<N> G;
        dim3 gt((c.dv.B + G::G - 1) / G::G), bt(G::NW * 64);      // one board group per workgroup
        if (c.emul == EMUL_BF16X3) hipLaunchKernelGGL((k_trunk_emul<N, EMUL_BF16X3>), gt, bt, 0, c.stream, c.dv, c.w[net_id], net_id, c.feat, c.dbg);
        else if (c.emul == EMUL_F16X2) hipLaunchKernelGGL((k_trunk_emul<N, EMUL_F16X2>), gt, bt, 0, c.stream, c.dv, c.w[net_id], net_id, c.feat, c.dbg);
        else hipLaunchKernelGGL(k_trunk<N>, gt, bt, 0, c.stream, c.dv, c.w[net_id], net_id, c.feat, c.dbg);
    }
}

// by cell tiles (az_net.h k_tile / k_tile_res): two launches of grid (groups, MT) for the plain net, six of 4-wave workgroups
// for the ResidualBlock net
void trunk_split(const LaunchCtx &c, int net_id)
{
    if (c.model == 1) {
        typedef ResGeo<N> G;
        const dim3 gt((c.dv.B + G::G - 1) / G::G, G::MT), b4(256);
        const ResWeights &w = c.rw[net_id];
        hipLaunchKernelGGL((k_tile_res<N, 0>), gt, b4, 0, c.stream, c.dv, w.stem, w.stemb, w.blk[0], w.blkb[0], net_id, c.scratch, c.feat);
        hipLaunchKernelGGL((k_tile_res<N, 1>), gt, b4, 0, c.stream, c.dv, w.blk[1], w.blkb[1], nullptr, nullptr, net_id, c.scratch, c.feat);
        hipLaunchKernelGGL((k_tile_res<N, 2>), gt, b4, 0, c.stream, c.dv, w.blk[2], w.blkb[2], nullptr, nullptr, net_id, c.scratch, c.feat);
        hipLaunchKernelGGL((k_tile_res<N, 1>), gt, b4, 0, c.stream, c.dv, w.blk[3], w.blkb[3], nullptr, nullptr, net_id, c.scratch, c.feat);
        hipLaunchKernelGGL((k_tile_res<N, 2>), gt, b4, 0, c.stream, c.dv, w.blk[4], w.blkb[4], nullptr, nullptr, net_id, c.scratch, c.feat);
        hipLaunchKernelGGL((k_tile_res<N, 3>), gt, b4, 0, c.stream, c.dv, w.blk[5], w.blkb[5], w.hd, w.hdb, net_id, c.scratch, c.feat);
        return;
    }
    typedef NetGeo<N> G;
    const dim3 gt((c.dv.B + G::G - 1) / G::G, G::MT), bt(G::NW * 64);
    hipLaunchKernelGGL((k_tile<N, 1>), gt, bt, 0, c.stream, c.dv, c.w[net_id], net_id, c.scratch, c.feat);
    hipLaunchKernelGGL((k_tile<N, 2>), gt, bt, 0, c.stream, c.dv, c.w[net_id], net_id, c.scratch, c.feat);
}

long long split_scratch_floats(int slots, int model)
{
    if (model == 1) return (long long)((slots + ResGeo<N>::G - 1) / ResGeo<N>::G) * ResTileGeo<N>::SCRATCH;
    return (long long)((slots + NetGeo<N>::G - 1) / NetGeo<N>::G) * TileGeo<N>::SCRATCH;
}

template <class G>
void fc_t(const LaunchCtx &c, int net_id, const NetWeights &w, unsigned long long *dbgfc)
{
    // few board rows: one tile per workgroup (the latency shape); many: eight per workgroup in four rounds of two (the
    // throughput shape: 3 workgroups per board row at n = 15)
    const int rows = (c.dv.B + 15) / 16;
    if (rows <= 4) {
        dim3 gf(rows, G::NTP + 4), bf(256);
        hipLaunchKernelGGL((k_fc<G, 1, 1>), gf, bf, 0, c.stream, c.dv, w, net_id, (const float *)c.feat, dbgfc);
    } else {
        dim3 gf(rows, (G::NTP + 7) / 8 + 1), bf(512);
        hipLaunchKernelGGL((k_fc<G, 2, 4>), gf, bf, 0, c.stream, c.dv, w, net_id, (const float *)c.feat, dbgfc);
    }
}

void fc(const LaunchCtx &c, int net_id)
{
    unsigned long long *dbgfc = c.dbg ? c.dbg + (size_t)c.dv.B * 16 : nullptr;
    if (c.model == 1) fc_t<ResGeo<N>>(c, net_id, c.w[net_id], dbgfc);
    else fc_t<NetGeo<N>>(c, net_id, c.w[net_id], dbgfc);
}

// S > DEFAULT_MAX_S (deep engines only): the DEEP tree kernels, no LDS sqrt table (az_tree.h)
void step(const LaunchCtx &c, int rootN, int do_select)
{
    dim3 g((c.d.B + STEP_WAVES - 1) / STEP_WAVES), b(STEP_WAVES * 64);
    if (c.d.proof) {                                           // az_set_solver (never with the synthetic evaluator): the SOLVER kernels
        if (c.d.S > DEFAULT_MAX_S) hipLaunchKernelGGL((k_step<N, false, true, true>), g, b, 0, c.stream, c.d, rootN, do_select);
        else hipLaunchKernelGGL((k_step<N, false, false, true>), g, b, (size_t)(c.d.S + 2) * sizeof(double), c.stream, c.d, rootN, do_select);
        return;
    }
    if (c.d.sel_cpuct) {                                       // az_set_selection (never with the solver): the SEL kernels
        const size_t lds = c.d.S > DEFAULT_MAX_S ? 0 : (size_t)(c.d.S + 2) * sizeof(double);
        if (c.d.S > DEFAULT_MAX_S) {
            if (c.synthetic) hipLaunchKernelGGL((k_step<N, true, true, false, true, false, SelLevel>), g, b, lds, c.stream, c.d, rootN, do_select, SelLevel{});
            else hipLaunchKernelGGL((k_step<N, false, true, false, true, false, SelLevel>), g, b, lds, c.stream, c.d, rootN, do_select, SelLevel{});
        } else {
            if (c.synthetic) hipLaunchKernelGGL((k_step<N, true, false, false, true, false, SelLevel>), g, b, lds, c.stream, c.d, rootN, do_select, SelLevel{});
            else hipLaunchKernelGGL((k_step<N, false, false, false, true, false, SelLevel>), g, b, lds, c.stream, c.d, rootN, do_select, SelLevel{});
        }
        return;
    }
    if (c.d.cand_radius) {                                     // az_set_candidates (never with the solver or the selection rule): the CAND kernels
        if (c.d.S > DEFAULT_MAX_S) {
            if (c.synthetic) hipLaunchKernelGGL((k_step<N, true, true, false, false, true, CandLevel>), g, b, 0, c.stream, c.d, rootN, do_select, CandLevel{});
            else hipLaunchKernelGGL((k_step<N, false, true, false, false, true, CandLevel>), g, b, 0, c.stream, c.d, rootN, do_select, CandLevel{});
            return;
        }
        const size_t lds = (size_t)(c.d.S + 2) * sizeof(double);
        if (c.synthetic) hipLaunchKernelGGL((k_step<N, true, false, false, false, true, CandLevel>), g, b, lds, c.stream, c.d, rootN, do_select, CandLevel{});
        else hipLaunchKernelGGL((k_step<N, false, false, false, false, true, CandLevel>), g, b, lds, c.stream, c.d, rootN, do_select, CandLevel{});
        return;
    }
    if (c.d.S > DEFAULT_MAX_S) {
        if (c.synthetic) hipLaunchKernelGGL((k_step<N, true, true>), g, b, 0, c.stream, c.d, rootN, do_select);
        else hipLaunchKernelGGL((k_step<N, false, true>), g, b, 0, c.stream, c.d, rootN, do_select);
        return;
    }
    const size_t lds = (size_t)(c.d.S + 2) * sizeof(double);   // sqrt table
    if (c.synthetic)
        hipLaunchKernelGGL((k_step<N, true>), g, b, lds, c.stream, c.d, rootN, do_select);
    else
        hipLaunchKernelGGL((k_step<N, false>), g, b, lds, c.stream, c.d, rootN, do_select);
}

void step_vl(const LaunchCtx &c, int sims_done, int nb_next)
{
    dim3 g((c.d.B + 3) / 4), b(256);
    if (c.d.sel_cpuct) {                                       // az_set_selection: the SEL kernels
        if (c.d.S > DEFAULT_MAX_S) {
            if (c.synthetic) hipLaunchKernelGGL((k_step_vl<N, true, true, true, false, SelLevel, unsigned char *>), g, b, 0, c.stream, c.d, sims_done, nb_next, SelLevel{}, c.inflight);
            else hipLaunchKernelGGL((k_step_vl<N, false, true, true, false, SelLevel, unsigned char *>), g, b, 0, c.stream, c.d, sims_done, nb_next, SelLevel{}, c.inflight);
            return;
        }
        const size_t lds = (size_t)(c.d.S + 2) * sizeof(double);
        if (c.synthetic) hipLaunchKernelGGL((k_step_vl<N, true, false, true, false, SelLevel>), g, b, lds, c.stream, c.d, sims_done, nb_next, SelLevel{});
        else hipLaunchKernelGGL((k_step_vl<N, false, false, true, false, SelLevel>), g, b, lds, c.stream, c.d, sims_done, nb_next, SelLevel{});
        return;
    }
    if (c.d.cand_radius) {                                     // az_set_candidates: the CAND kernels
        if (c.d.S > DEFAULT_MAX_S) {
            if (c.synthetic) hipLaunchKernelGGL((k_step_vl<N, true, true, false, true, CandLevel, unsigned char *>), g, b, 0, c.stream, c.d, sims_done, nb_next, CandLevel{}, c.inflight);
            else hipLaunchKernelGGL((k_step_vl<N, false, true, false, true, CandLevel, unsigned char *>), g, b, 0, c.stream, c.d, sims_done, nb_next, CandLevel{}, c.inflight);
            return;
        }
        const size_t lds = (size_t)(c.d.S + 2) * sizeof(double);
        if (c.synthetic) hipLaunchKernelGGL((k_step_vl<N, true, false, false, true, CandLevel>), g, b, lds, c.stream, c.d, sims_done, nb_next, CandLevel{});
        else hipLaunchKernelGGL((k_step_vl<N, false, false, false, true, CandLevel>), g, b, lds, c.stream, c.d, sims_done, nb_next, CandLevel{});
        return;
    }
    if (c.d.S > DEFAULT_MAX_S) {
        if (c.synthetic) hipLaunchKernelGGL((k_step_vl<N, true, true, false, false, unsigned char *>), g, b, 0, c.stream, c.d, sims_done, nb_next, c.inflight);
        else hipLaunchKernelGGL((k_step_vl<N, false, true, false, false, unsigned char *>), g, b, 0, c.stream, c.d, sims_done, nb_next, c.inflight);
        return;
    }
    const size_t lds = (size_t)(c.d.S + 2) * sizeof(double);   // sqrt table
    if (c.synthetic)
        hipLaunchKernelGGL((k_step_vl<N, true>), g, b, lds, c.stream, c.d, sims_done, nb_next);
    else
        hipLaunchKernelGGL((k_step_vl<N, false>), g, b, lds, c.stream, c.d, sims_done, nb_next);
}

void root_cache(const LaunchCtx &c)
{
    dim3 g((c.d.B + 3) / 4), b(256);
    hipLaunchKernelGGL(k_root_cache<N>, g, b, 0, c.stream, c.d);
}

constexpr bool HAS_SEARCH = N <= 7;      // the LDS-resident tree needs (S + 1) * n*n * 16 B per game
constexpr bool HAS_SEARCH2 = N <= 5;     // two games per workgroup: beyond 5x5 the rows of two games never fit beside the image

// SOLVER (az_set_solver): one status byte per edge behind the edges, and the SOLVER kernel (no tile-subset variant of it)
template <int GP, bool SY, bool RES, bool SOLVER = false>
int search_prepare_t(int S)
{
    if constexpr (HAS_SEARCH) {
        const size_t dyn = (size_t)GP * (S + 1) * N * N * (sizeof(Edge) + (SOLVER ? 1 : 0));
        const void *fns[2] = {reinterpret_cast<const void *>(&k_search<N, GP, SY, false, RES, SOLVER>),
                              reinterpret_cast<const void *>(&k_search<N, GP, SY, GP == 2 && !SY && !SOLVER, RES, SOLVER>)};     // [1]: the tile-subset variant (search_t)
        for (const void *fn : fns) {
            hipFuncAttributes at;
            if (hipFuncGetAttributes(&at, fn) != hipSuccess) return 0;
            if (at.sharedSizeBytes + dyn > 160u * 1024u) return 0;
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) return 0;
        }
        return 1;
    } else {
        return 0;
    }
}

int search_prepare(int S, int games, int synthetic, int model, int solver)
{
    if (S > DEFAULT_MAX_S) return 0;                   // k_search's static sqrt table holds S + 2 <= 1026 entries
    const bool res = model == 1 && !synthetic;         // the synthetic evaluator has no net: the plain kernels serve it
    if (solver) {                                      // never with the synthetic evaluator
        if (synthetic) return 0;
        if (games == 2) {
            if constexpr (HAS_SEARCH2) return res ? search_prepare_t<2, false, true, true>(S) : search_prepare_t<2, false, false, true>(S);
            return 0;
        }
        if (games == 1) return res ? search_prepare_t<1, false, true, true>(S) : search_prepare_t<1, false, false, true>(S);
        return 0;
    }
    if (games == 2) {
        if constexpr (HAS_SEARCH2)
            return synthetic ? search_prepare_t<2, true, false>(S) : (res ? search_prepare_t<2, false, true>(S) : search_prepare_t<2, false, false>(S));
        return 0;
    }
    if (games == 1) return synthetic ? search_prepare_t<1, true, false>(S) : (res ? search_prepare_t<1, false, true>(S) : search_prepare_t<1, false, false>(S));
    return 0;
}

template <int GP>
void search_t(const LaunchCtx &c)
{
    if constexpr (HAS_SEARCH) {
        dim3 g((c.d.B + GP - 1) / GP), b(NetGeo<N>::NW * 64);
        const size_t dyn = (size_t)GP * c.d.R * N * N * sizeof(Edge);
        const bool ts = GP == 2 && (c.d.cache || c.d.reuse);      // many iterations with one game waiting for the net: compute its tiles only
        if (c.d.proof) {                                          // az_set_solver: the status bytes behind the edges
            const size_t dyns = dyn + (size_t)GP * c.d.R * N * N;
            if (c.model == 1) hipLaunchKernelGGL((k_search<N, GP, false, false, true, true>), g, b, dyns, c.stream, c.d, c.w[0], c.w[1], c.dbg, c.rw[0], c.rw[1]);
            else hipLaunchKernelGGL((k_search<N, GP, false, false, false, true>), g, b, dyns, c.stream, c.d, c.w[0], c.w[1], c.dbg, NoWeights{}, NoWeights{});
            return;
        }
        if (c.synthetic)
            hipLaunchKernelGGL((k_search<N, GP, true, false, false>), g, b, dyn, c.stream, c.d, c.w[0], c.w[1], c.dbg, NoWeights{}, NoWeights{});
        else if (c.model == 1) {
            if (ts) hipLaunchKernelGGL((k_search<N, GP, false, GP == 2, true>), g, b, dyn, c.stream, c.d, c.w[0], c.w[1], c.dbg, c.rw[0], c.rw[1]);
            else hipLaunchKernelGGL((k_search<N, GP, false, false, true>), g, b, dyn, c.stream, c.d, c.w[0], c.w[1], c.dbg, c.rw[0], c.rw[1]);
        } else {
            if (ts) hipLaunchKernelGGL((k_search<N, GP, false, GP == 2, false>), g, b, dyn, c.stream, c.d, c.w[0], c.w[1], c.dbg, NoWeights{}, NoWeights{});
            else hipLaunchKernelGGL((k_search<N, GP, false, false, false>), g, b, dyn, c.stream, c.d, c.w[0], c.w[1], c.dbg, NoWeights{}, NoWeights{});
        }
    }
}

void search(const LaunchCtx &c, int games)
{
    if constexpr (HAS_SEARCH2) {
        if (games == 2) { search_t<2>(c); return; }
    }
    search_t<1>(c);
}

void move(const LaunchCtx &c)
{
    dim3 g((c.d.B + 3) / 4), b(256);
    hipLaunchKernelGGL(k_move<N>, g, b, 0, c.stream, c.d);
}

void eval_tail_l(const LaunchCtx &c, int count, float *pol, float *val)
{
    dim3 g((count + 3) / 4), b(256);
    hipLaunchKernelGGL(k_eval_tail<N>, g, b, 0, c.stream, c.dv, count, pol, val);
}

int batch_slots(const BatchLanes &bl)
{
    int slots = 0;
    for (int l = 0; l < bl.K; l++) slots += bl.lane[l].B;
    return slots;
}

void set_positions(hipStream_t stream, const BatchLanes &bl, const unsigned char *cells, const unsigned char *players, const short *lasts)
{
    dim3 g((batch_slots(bl) + 3) / 4), b(256);
    hipLaunchKernelGGL(k_set_positions<N>, g, b, 0, stream, bl, cells, players, lasts);
}

void gather_roots(hipStream_t stream, const BatchLanes &bl, const DevState &d, const unsigned char *cells, int *visits, double *W, float *prior, float *pi, int *action)
{
    dim3 g((batch_slots(bl) + 3) / 4), b(256);
    hipLaunchKernelGGL(k_gather_roots<N>, g, b, 0, stream, bl, d.R, d.S, cells, (const float *)d.rec_pi,
                       (const short *)d.rec_action, visits, W, prior, pi, action);
}

void build_positions(hipStream_t stream, int count, const unsigned char *cells, const unsigned char *players, const short *lasts, StartPos *table)
{
    dim3 g((count + 3) / 4), b(256);
    hipLaunchKernelGGL(k_build_positions<N>, g, b, 0, stream, count, cells, players, lasts, table);
}

void ext_gather(const LaunchCtx &c, int net, int item_base, int first, int capacity, float *planes, int *map, int *count)
{
    hipLaunchKernelGGL(k_ext_gather<N>, dim3(1), dim3(EXT_GATHER_THREADS), 0, c.stream, c.dv, net, item_base, first, capacity, planes, map, count);
}

void ext_scatter(const LaunchCtx &c, int item_base, int count, const int *map, const float *policy, const float *value)
{
    dim3 g((count + 3) / 4), b(256);
    hipLaunchKernelGGL(k_ext_scatter<N>, g, b, 0, c.stream, c.dv, item_base, count, map, policy, value);
}

void threat(const LaunchCtx &c)
{
    hipLaunchKernelGGL(k_threat<N>, dim3(c.d.B), dim3(64), 0, c.stream, c.d);
}

constexpr bool HAS_DELTA = N == 15;      // the plain float32 trunk of the headline size (az_delta.h)

void trunk_base(const LaunchCtx &c, int net_id)
{
    if constexpr (HAS_DELTA)
        hipLaunchKernelGGL(k_trunk_base<N>, dim3(c.d.B, 2), dim3(NetGeo<N>::NW * 64), 0, c.stream, c.d, c.w[net_id], net_id, c.delta_base, c.delta_cnt);
}

void trunk_delta(const LaunchCtx &c, int net_id)
{
    if constexpr (HAS_DELTA) {
        const dim3 g(c.dv.B), b(NetGeo<N>::NW * 64);
        hipLaunchKernelGGL(k_trunk_delta<N>, g, b, 0, c.stream, c.dv, c.w[net_id], net_id, c.feat, (const float *)c.delta_base, c.delta_done,
                           c.delta_cnt, c.delta_tiles, c.dbg);
    }
}

template <bool ON>
long long delta_floats() { if constexpr (ON) return 2ll * DeltaGeo<N>::STRIDE; else return 0; }
}   // namespace

const SizeOps *AZ_CAT(az_size_ops_, AZ_N)()
{
    static const SizeOps ops = {trunk, trunk_split, split_scratch_floats, fc, step, step_vl, root_cache, search_prepare, search, move, eval_tail_l,
                                set_positions, gather_roots, build_positions, ext_gather, ext_scatter, threat,
                                HAS_DELTA ? trunk_base : nullptr, HAS_DELTA ? trunk_delta : nullptr, delta_floats<HAS_DELTA>()};
    return &ops;
}
