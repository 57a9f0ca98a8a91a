// capi_label.hip: data cost, alpha-expansion, re-estimation, LabelingStep, post-filter statistics — part of the C ABI of include/multih_hip.h (see capi_engine.hpp for the split).
#include "capi_engine.hpp"

namespace {

// Contexts of the concurrent alpha-moves (key 37), bounded by what they cost: a context is 2 nnz + 13 n ints, and the complete
// radius neighbourhood of the reference's rule can hold hundreds of millions of arcs — beyond 8 GiB of contexts fewer moves run
// together (results never depend on the number).
int expand_contexts(const mh_engine* e)
{
    const int want = std::max(1, std::min(e->tune_expand_ctx, EXPAND_MAX_CTX));
    const double per_ctx = 4.0 * (2.0 * (double)e->g_nnz + 13.0 * (double)e->n + 2048.0);
    const int fit = 1 + (int)std::min(64.0, 8.0 * 1024.0 * 1024.0 * 1024.0 / std::max(per_ctx, 1.0));
    return std::max(1, std::min(want, fit));
}

int ensure_expand_work(mh_engine* e)
{
    const int n = e->n, n_ctx = expand_contexts(e);
    HIPCHK(e->ew_label.reserve(n));
    HIPCHK(e->ew_cur.reserve(n));
    HIPCHK(e->h_flags.ensure(EXPAND_HOST_WORDS));
    HIPCHK(e->h_acc.ensure(16));
    // (only batches walk a took list: a single context goes without)
    for (int k = 0; k < n_ctx; ++k) HIPCHK(e->ew_ctx[k].reserve(n, e->g_nnz, n_ctx > 1, e->stream));
    if (n_ctx > 1) {
        HIPCHK(e->ew_bctl.reserve(8 + EXPAND_MAX_CTX));
        HIPCHK(e->h_batch.ensure(8));
    }
    return MH_OK;
}

int do_data_cost(mh_engine* e)
{
    const int L = e->m + 1;
    HIPCHK(e->cost.reserve((size_t)e->n * L));
    {
        ScopedTimer t(e, MH_K_DATACOST);
        HIPCHK(launch_data_cost(e->pts(), e->H.p, e->m, e->lambda, e->thr_H * e->thr_H, e->cost.p, e->stream,
                                e->data_term == MH_DATA_TERM_RISING, e->route_symmetric()));
    }
    e->cost_L = L;
    return MH_OK;
}

// How many workgroups of the solver launch the device holds at once: the occupancy query's answer for k_solve at its
// default dynamic LDS, times the CUs — and never more than one per CU (the kernel is written for that).
int solve_grid_limit(mh_engine* e)
{
    if (e->solve_grid_max > 0) return MH_OK;
    int per_cu = 0;
    HIPCHK(solver_blocks_per_cu(&per_cu));
    if (per_cu < 1) return fail(MH_ERR_HIP, "the alpha-expansion solver kernel does not fit a compute unit");
    e->solve_grid_max = e->cu_count * 1;
    return MH_OK;
}

// init_dev: device pointer to initial labels (GCO numbering) or null.
int do_expand(mh_engine* e, const int* init_dev, long long* energy, int* cycles)
{
    if (!e->have_graph) return fail(MH_ERR_NOT_SET, "neighbour graph is not set");
    if (e->cost_L != e->m + 1) return fail(MH_ERR_NOT_SET, "data cost is stale; call mh_data_cost first");
    int rc = ensure_expand_work(e);
    if (rc) return rc;
    Graph g{ e->d_rowptr.p, e->d_col.p, e->w_dev(), e->d_rev.p, e->n, e->g_nnz, e->d_order.p, e->d_wsum.p };
    // The solver launch synchronises through a grid barrier, so it must be resident as a whole: one 512-thread workgroup
    // per CU at most (what the occupancy query admits for this kernel is checked once per engine, solve_grid_limit).
    // One process per GPU — the deployment — always is.  Engines of several processes that share a GPU can keep each
    // other's workgroups off the chip; a launch whose barrier then gives up (3 s) is not an error any more: the
    // expansion is restarted from its initial labeling with half the workgroups (results never depend on that number),
    // up to four times — a shared GPU degrades instead of failing.  `mh_set_tuning` key 5 sets the starting number.
    rc = solve_grid_limit(e);
    if (rc) return rc;
    int solve_grid = std::max(1, std::min(e->tune_expand[3], e->solve_grid_max));
    ExpandWork w;
    w.label = e->ew_label.p; w.cur_cost = e->ew_cur.p;
    w.n_ctx = expand_contexts(e);
    for (int k = 0; k < w.n_ctx; ++k) w.ctx[k] = e->ew_ctx[k].view(g.n, g.nnz);
    w.h_flags = e->h_flags.h; w.h_flags_dev = e->h_flags.d;
    w.h_acc = e->h_acc.h; w.h_acc_dev = e->h_acc.d;
    if (w.n_ctx > 1) {                                            // batches (expand.hip, k_batch_commit)
        w.bctl = e->ew_bctl.p;
        w.h_batch = e->h_batch.h; w.h_batch_dev = e->h_batch.d;
    }
    ExpandTuning& tu = w.tune;
    tu.relax_rounds = e->tune_expand[0]; tu.push_cycles = e->tune_expand[1]; tu.push_phases = e->tune_expand[2];
    tu.push_mult = e->tune_push_mult;
    tu.reduce_rounds = e->tune_reduce; tu.reduce_launches = e->tune_reduce_launches;
    tu.cascade_iters = e->tune_cascade_iters;
    tu.batch_min_labels = e->tune_batch_min_labels; tu.batch_spw = e->tune_batch_spw;
    // flow recycling (expand_solve.hip, k_solve): L x (nnz + n) ints, cleared per expansion; left out (every move starts from
    // the zero flow) beyond 8 GiB.  Flows are not kept from one call to the next: measured in the alternation, the
    // re-estimated models move the problems far enough for a kept flow to cost more rounds than the zero flow.
    const size_t recycle_words = (size_t)e->cost_L * ((size_t)g.nnz + (size_t)g.n);
    if (e->tune_recycle && recycle_words <= ((size_t)2 << 30)) {
        HIPCHK(e->ew_saved.reserve(recycle_words));
        HIPCHK(hipMemsetAsync(e->ew_saved.p, 0, sizeof(int) * recycle_words, e->stream));
        w.saved_flow = e->ew_saved.p;
        w.saved_sink = e->ew_saved.p + (size_t)e->cost_L * g.nnz;
    }
    if (e->trace_moves > 0) {
        HIPCHK(e->ew_trace.reserve(8 * (size_t)e->trace_moves + 4 * 2048));
        HIPCHK(hipMemsetAsync(e->ew_trace.p, 0, sizeof(int) * (8 * (size_t)e->trace_moves + 4 * 2048), e->stream));
        w.detail_move = e->detail_move;
        w.trace = e->ew_trace.p;
        w.trace_moves = e->trace_moves;
    }
    if (e->comp_moves > 0) {
        HIPCHK(e->ew_comp.reserve(2 * (size_t)g.n));
        HIPCHK(e->ew_comp_out.reserve(16 * (size_t)e->comp_moves));
        HIPCHK(hipMemsetAsync(e->ew_comp_out.p, 0, sizeof(int) * 16 * (size_t)e->comp_moves, e->stream));
        w.comp_out = e->ew_comp_out.p; w.comp_scratch = e->ew_comp.p; w.comp_moves = e->comp_moves;
    }
    const int potts = (int)std::round(100.0 * e->lambda);     // M/MultiH.h:41, MultiH.cpp:510
    ExpandStats st{};
    {
        ScopedTimer t(e, MH_K_EXPAND);
        ExpandResult res;
        e->last_expand_retries = 0;
        for (int attempt = 0; attempt < 5; ++attempt) {
            tu.solve_grid = solve_grid;
            // How long a barrier may wait before the launch gives up and the expansion restarts: a healthy barrier takes
            // about 8 us, so max(20 ms, 50 x the longest steady-state wait this engine has seen) tells "a workgroup is not
            // resident" from "slow" within tens of milliseconds.  The FIRST barrier of a launch is the one that waits for
            // every workgroup to be dispatched — on a GPU shared with another engine's 7 ms sweeps that is a matter of the
            // other work's length, not of this launch's size: it gets 250 ms (ten times the steady limit if that is more).
            // A timed-out attempt is repeated ONCE with the same grid before the grid is halved; only the last attempt (or
            // a launch already down to one workgroup) waits the full 3 s before the call fails.
            const bool last_attempt = attempt == 4 || solve_grid == 1;
            const double steady_ms = std::max(20.0, 50.0 * e->longest_barrier_wait_ms);
            tu.barrier_timeout_ticks = last_attempt ? 300000000ll : (long long)(steady_ms * 1e5);
            tu.barrier_first_timeout_ticks = last_attempt ? 300000000ll : (long long)(std::max(250.0, 10.0 * steady_ms) * 1e5);
            if (w.saved_flow) HIPCHK(hipMemsetAsync(e->ew_saved.p, 0, sizeof(int) * recycle_words, e->stream));
            HIPCHK(launch_init_labeling(e->cost.p, e->cost_L, e->n, init_dev, w.label, w.cur_cost, e->stream));
            w.hooks.inject_group = e->inject_solve_failure >> 4;                    // test hook (mh_set_tuning key 40): first attempt only
            w.hooks.inject_ctx = e->inject_solve_failure & 15;
            e->inject_solve_failure = 0;
            res = run_expansion(g, e->cost.p, e->cost_L, potts, w, 1000, &st, e->stream);
            if (res.status == ExpandStatus::ok && e->inject_barrier_timeouts > 0) {           // test hook (mh_set_tuning key 14)
                --e->inject_barrier_timeouts;
                res.status = ExpandStatus::barrier_timeout;
            }
            e->last_solve_grid = solve_grid;
            if (res.status != ExpandStatus::barrier_timeout || solve_grid == 1 || attempt == 4) break;
            if (attempt >= 1) solve_grid = std::max(1, solve_grid / 2);      // (the first retry keeps the grid)
            ++e->last_expand_retries;
            ++e->expand_retries_total;
        }
        switch (res.status) {
        case ExpandStatus::ok: break;
        case ExpandStatus::too_many_sites:
            return fail(MH_ERR_INVALID, "alpha-expansion: more sites than the solver's per-row state holds (about 1.3 million at 256 workgroups)");
        case ExpandStatus::overflow:
            return fail(MH_ERR_OVERFLOW, "int32 energy term overflow in alpha-expansion");
        case ExpandStatus::barrier_timeout:
            return fail(MH_ERR_HIP, "alpha-expansion: the solver's grid barrier timed out even with the launch cut down to a few workgroups "
                                    "(its workgroups were not all resident; is the GPU shared with other persistent launches?)");
        case ExpandStatus::no_convergence:
            return fail(MH_ERR_HIP, "alpha-expansion: push-relabel did not converge within its iteration bound");
        case ExpandStatus::hip_error: { const hipError_t he = res.hip; HIPCHK(he); }
        }
    }
    e->last_expand = st;
    if (st.max_barrier_wait_ms > e->longest_barrier_wait_ms) e->longest_barrier_wait_ms = std::min(st.max_barrier_wait_ms, 50.0);
    if (st.energy > 0x7fffffffll || st.energy < -0x7fffffffll)
        return fail(MH_ERR_OVERFLOW, "total energy exceeds the reference's int32 EnergyType");
    if (energy) *energy = st.energy;
    if (cycles) *cycles = st.cycles;
    return MH_OK;
}

__global__ void k_shift_labels(int n, const int* in, int delta, int* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i] + delta;
}

} // namespace

extern "C" {

// H / ok given: the caller fitted the trials' homographies (the form until r05); F given instead: the engine fits them itself
static int compat_trial_stats(mh_engine* e, const double* pts_xyxy, const int* cluster_begin, int clusters, const int* tri,
                              const double* H, const unsigned char* ok, const double* F, int trials, double* stats_out, double* H_out,
                              unsigned char* ok_out)
{
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (clusters < 0 || trials < 0) return fail(MH_ERR_INVALID, "negative cluster or trial count");
    if (clusters == 0 || trials == 0) return MH_OK;
    if (!pts_xyxy || !cluster_begin || !tri || !stats_out || (!F && (!H || !ok))) return fail(MH_ERR_INVALID, "null argument");
    if (cluster_begin[0] != 0) return fail(MH_ERR_INVALID, "cluster_begin[0] must be 0");
    for (int c = 0; c < clusters; ++c)
        if (cluster_begin[c + 1] - cluster_begin[c] < 19)
            return fail(MH_ERR_INVALID, "a cluster of fewer than 19 points: the caller handles those itself (the three stale entries of the reference's buffer reach the median ranks)");
    const size_t total = (size_t)cluster_begin[clusters], ct = (size_t)clusters * (size_t)trials;
    if (ct > (size_t)0x7fffffff) return fail(MH_ERR_INVALID, "too many trials");
    for (size_t i = 0; i < ct; ++i) {
        const int nc = cluster_begin[i / trials + 1] - cluster_begin[i / trials];
        for (int j = 0; j < 3; ++j)
            if (tri[3 * i + j] < 0 || tri[3 * i + j] >= nc) return fail(MH_ERR_INVALID, "a trial draws a point outside its cluster");
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->cp_pts.reserve(4 * total)); HIPCHK(e->cp_begin.reserve(clusters + 1)); HIPCHK(e->cp_tri.reserve(3 * ct));
    HIPCHK(e->cp_H.reserve(9 * ct)); HIPCHK(e->cp_ok.reserve(ct)); HIPCHK(e->cp_out.reserve(8 * ct));
    HIPCHK(hipMemcpyAsync(e->cp_pts.p, pts_xyxy, sizeof(double) * 4 * total, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->cp_begin.p, cluster_begin, sizeof(int) * (clusters + 1), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->cp_tri.p, tri, sizeof(int) * 3 * ct, hipMemcpyHostToDevice, e->stream));
    if (F) {
        HIPCHK(launch_compat_fit(e->cp_pts.p, e->cp_begin.p, clusters, e->cp_tri.p, F, trials, e->cp_H.p, e->cp_ok.p, e->stream));
    } else {
        HIPCHK(hipMemcpyAsync(e->cp_H.p, H, sizeof(double) * 9 * ct, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->cp_ok.p, ok, ct, hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(launch_compat_select(e->cp_pts.p, e->cp_begin.p, clusters, e->cp_tri.p, e->cp_H.p, e->cp_ok.p, trials, e->cp_out.p, e->stream));
    HIPCHK(hipMemcpyAsync(stats_out, e->cp_out.p, sizeof(double) * 8 * ct, hipMemcpyDeviceToHost, e->stream));
    if (H_out) HIPCHK(hipMemcpyAsync(H_out, e->cp_H.p, sizeof(double) * 9 * ct, hipMemcpyDeviceToHost, e->stream));
    if (ok_out) HIPCHK(hipMemcpyAsync(ok_out, e->cp_ok.p, ct, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MH_OK;
}

int mh_compat_trial_stats(mh_engine* e, const double* pts_xyxy, const int* cluster_begin, int clusters, const int* tri,
                          const double* H, const unsigned char* ok, int trials, double* stats_out)
{
    return guarded([&]() -> int {
    if (!H || !ok) return fail(MH_ERR_INVALID, "null argument");
    return compat_trial_stats(e, pts_xyxy, cluster_begin, clusters, tri, H, ok, nullptr, trials, stats_out, nullptr, nullptr);
    });
}

int mh_compat_trial_stats_fit(mh_engine* e, const double* pts_xyxy, const int* cluster_begin, int clusters, const int* tri,
                              const double F[9], int trials, double* stats_out, double* H_out, unsigned char* ok_out)
{
    return guarded([&]() -> int {
    if (!F) return fail(MH_ERR_INVALID, "null argument");
    return compat_trial_stats(e, pts_xyxy, cluster_begin, clusters, tri, nullptr, nullptr, F, trials, stats_out, H_out, ok_out);
    });
}

// The check without F (the definition: include/multih_hip.h).  The packed points are staged as a structure of arrays (x1 | y1 |
// x2 | y2 in cp_pts), which is what k_dlt4 reads; nothing but the cp_ staging buffers is written.
int mh_compat_dlt_medians(mh_engine* e, const double* pts_xyxy, const int* cluster_begin, int clusters, unsigned long long seed,
                          long long first, int trials, double* medians_out, double* trial_out, double* H_out, int* idx_out)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (!pts_xyxy || !cluster_begin || !medians_out) return fail(MH_ERR_INVALID, "null argument");
    if (clusters < 1) return fail(MH_ERR_INVALID, "no cluster");
    if (trials < 1 || trials > MH_COMPAT_DLT_MAX_TRIALS) return fail(MH_ERR_INVALID, "trials outside [1, MH_COMPAT_DLT_MAX_TRIALS]");
    if (first < 0) return fail(MH_ERR_INVALID, "negative first counter");
    if ((long long)clusters * trials > (1ll << 22)) return fail(MH_ERR_INVALID, "more than 2^22 trials in one call");
    if (cluster_begin[0] != 0) return fail(MH_ERR_INVALID, "cluster_begin[0] must be 0");
    for (int c = 0; c < clusters; ++c) {
        if (cluster_begin[c + 1] < cluster_begin[c]) return fail(MH_ERR_INVALID, "cluster_begin must not decrease");
        if (cluster_begin[c + 1] - cluster_begin[c] < MH_COMPAT_DLT_MIN_POINTS)
            return fail(MH_ERR_INVALID, "a cluster of fewer than MH_COMPAT_DLT_MIN_POINTS points: the caller keeps those itself");
    }
    const size_t total = (size_t)cluster_begin[clusters], ct = (size_t)clusters * (size_t)trials;
    std::vector<double> soa(4 * total);                                   // (alive until the copies below have been waited for)
    for (size_t i = 0; i < total; ++i)
        for (int k = 0; k < 4; ++k) soa[k * total + i] = pts_xyxy[4 * i + k];
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->cp_pts.reserve(4 * total)); HIPCHK(e->cp_begin.reserve(clusters + 1)); HIPCHK(e->cp_idx.reserve(4 * ct));
    HIPCHK(e->cp_H.reserve(9 * ct)); HIPCHK(e->cp_out.reserve(ct + clusters));
    const double* x1 = e->cp_pts.p;
    const double *y1 = x1 + total, *x2 = x1 + 2 * total, *y2 = x1 + 3 * total;
    double* trial_dev = e->cp_out.p;
    double* med_dev = e->cp_out.p + ct;
    HIPCHK(hipMemcpyAsync(e->cp_pts.p, soa.data(), sizeof(double) * 4 * total, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->cp_begin.p, cluster_begin, sizeof(int) * (clusters + 1), hipMemcpyHostToDevice, e->stream));
    {
        ScopedTimer t(e, MH_K_DLT4);
        HIPCHK(launch_dlt4_segments(x1, y1, x2, y2, (int)total, e->cp_begin.p, trials, seed, first, (int)ct, e->cp_idx.p, e->cp_H.p,
                                    e->stream));
    }
    {
        ScopedTimer t(e, MH_K_SCORE);
        HIPCHK(launch_compat_median4(x1, y1, x2, y2, e->cp_begin.p, clusters, e->cp_idx.p, e->cp_H.p, trials, trial_dev, e->stream));
    }
    {
        ScopedTimer t(e, MH_K_REESTIMATE);
        HIPCHK(launch_compat_cluster_median(trial_dev, clusters, trials, med_dev, e->stream));
    }
    HIPCHK(hipMemcpyAsync(medians_out, med_dev, sizeof(double) * clusters, hipMemcpyDeviceToHost, e->stream));
    if (trial_out) HIPCHK(hipMemcpyAsync(trial_out, trial_dev, sizeof(double) * ct, hipMemcpyDeviceToHost, e->stream));
    if (H_out) HIPCHK(hipMemcpyAsync(H_out, e->cp_H.p, sizeof(double) * 9 * ct, hipMemcpyDeviceToHost, e->stream));
    if (idx_out) HIPCHK(hipMemcpyAsync(idx_out, e->cp_idx.p, sizeof(int) * 4 * ct, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MH_OK;
    });
}

int mh_data_cost(mh_engine* e, int* cost)
{
    return guarded([&]() -> int {
    int rc = require_models(e);
    if (rc) return rc;
    rc = do_data_cost(e);
    if (rc) return rc;
    if (cost) {
        HIPCHK(hipMemcpyAsync(cost, e->cost.p, sizeof(int) * (size_t)e->n * e->cost_L, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return MH_OK;
    });
}

int mh_expand(mh_engine* e, const int* init_labels, int* labels_out, int* energy, int* cycles)
{
    return guarded([&]() -> int {
    int rc = require_models(e);
    if (rc) return rc;
    const int* init_dev = nullptr;
    if (init_labels) {
        for (int i = 0; i < e->n; ++i)
            if (init_labels[i] < 0 || init_labels[i] > e->m)
                return fail(MH_ERR_INVALID, "initial label out of range 0..Nh");
        HIPCHK(e->labels_in.reserve(e->n));
        HIPCHK(hipMemcpyAsync(e->labels_in.p, init_labels, sizeof(int) * e->n, hipMemcpyHostToDevice, e->stream));
        init_dev = e->labels_in.p;
    }
    long long en = 0;
    rc = do_expand(e, init_dev, &en, cycles);
    if (rc) return rc;
    if (energy) *energy = (int)en;
    if (labels_out) {
        HIPCHK(hipMemcpyAsync(labels_out, e->ew_label.p, sizeof(int) * e->n, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return MH_OK;
    });
}

int mh_get_expand_stats(mh_engine* e, long long stats[24])
{
    return guarded([&]() -> int {
    if (!e || !stats) return fail(MH_ERR_INVALID, "null argument");
    const ExpandStats& x = e->last_expand;
    stats[0] = x.cycles;
    stats[1] = x.moves;
    stats[2] = x.accepted;
    stats[3] = x.push_phases;
    stats[4] = x.relax_intervals;
    stats[5] = x.host_syncs;
    stats[6] = x.reduce_launches;
    stats[7] = x.flow_moves;
    stats[8] = x.launches;
    stats[9] = x.moves_run;
    stats[10] = x.moves_solved;
    stats[11] = x.core_sites;
    stats[12] = x.core_max;
    stats[13] = x.barriers;
    stats[14] = x.outer_iterations;
    stats[15] = (long long)(x.solve_ms * 1000.0);      // microseconds inside the solver launches
    stats[16] = (long long)(x.barrier_ms * 1000.0);
    stats[17] = (long long)(x.relax_ms * 1000.0);
    stats[18] = (long long)(x.push_ms * 1000.0);
    stats[19] = (long long)(x.tail_ms * 1000.0);
    stats[20] = e->last_expand_retries;
    stats[21] = e->last_solve_grid;
    stats[22] = e->expand_retries_total;
    stats[23] = (long long)(e->last_expand.max_barrier_wait_ms * 1e3);
    return MH_OK;
    });
}

int mh_get_expand_batch_stats(mh_engine* e, long long stats[8])
{
    return guarded([&]() -> int {
    if (!e || !stats) return fail(MH_ERR_INVALID, "null argument");
    const ExpandStats& x = e->last_expand;
    stats[0] = x.batches;
    stats[1] = x.batch_committed;
    stats[2] = x.batch_invalid;
    stats[3] = x.host_skipped;
    stats[4] = x.solo_moves;
    stats[5] = x.injected_discarded;
    stats[6] = expand_contexts(e);
    stats[7] = e->tune_batch_min_labels;
    return MH_OK;
    });
}

int mh_get_expand_trace(mh_engine* e, int* trace, int moves)
{
    return guarded([&]() -> int {
    int rc = enter(e);
    if (rc) return rc;
    if (!trace || moves <= 0) return fail(MH_ERR_INVALID, "null trace or moves <= 0");
    if (e->trace_moves <= 0 || !e->ew_trace.p) return fail(MH_ERR_NOT_SET, "tracing is off (mh_set_tuning key 8) or no expansion has run");
    // rows [0, trace_moves): the moves; rows behind them: the relabel log of the detail move (key 9), two relabels per row
    // (the buffer was sized by the trace_moves in force at the last expansion: never read past it)
    const int m = std::min(moves, (int)std::min<size_t>((size_t)e->trace_moves + 1024, e->ew_trace.cap / 8));
    HIPCHK(hipMemcpyAsync(trace, e->ew_trace.p, sizeof(int) * 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MH_OK;
    });
}

int mh_get_core_components(mh_engine* e, int* out, int moves)
{
    return guarded([&]() -> int {
    int rc = enter(e);
    if (rc) return rc;
    if (!out || moves <= 0) return fail(MH_ERR_INVALID, "null output or moves <= 0");
    if (e->comp_moves <= 0 || !e->ew_comp_out.p) return fail(MH_ERR_NOT_SET, "the component diagnostic is off (mh_set_tuning key 21) or no expansion has run");
    const int m = std::min(moves, (int)(e->ew_comp_out.cap / 16));
    HIPCHK(hipMemcpyAsync(out, e->ew_comp_out.p, sizeof(int) * 16 * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MH_OK;
    });
}

} // extern "C"

namespace mhe {

int launch_estimator(mh_engine* e, const int* labels_dev, int Nh, double* H_dev, int* counts_dev)
{
    ScopedTimer t(e, MH_K_REESTIMATE);
    if (e->estimator == MH_ESTIMATOR_DLT && e->est_rw_rounds > 0 && e->est_rw_auto) {   // mh_set_estimator_reweighting_auto: the same, the scale from the data
        HIPCHK(launch_autoscale_reweight_h(e->pts(), labels_dev, H_dev, Nh, e->est_rw_scale, e->est_rw_rounds, H_dev, nullptr, nullptr,
                                           nullptr, counts_dev, e->stream));
        return MH_OK;
    }
    if (e->estimator == MH_ESTIMATOR_DLT && e->est_rw_rounds > 0) {      // mh_set_estimator_reweighting: from each label's standing model, in place
        HIPCHK(launch_reweight_h(e->pts(), labels_dev, H_dev, Nh, e->est_rw_c2, e->est_rw_rounds, H_dev, nullptr, nullptr, counts_dev,
                                 e->stream));
        return MH_OK;
    }
    if (e->estimator == MH_ESTIMATOR_DLT) {
        HIPCHK(launch_reestimate_dlt(e->pts(), labels_dev, Nh, H_dev, counts_dev, e->stream));
        return MH_OK;
    }
    if (e->estimator == MH_ESTIMATOR_3PT) {
        HIPCHK(e->r3_scratch.reserve(reestimate_3pt_scratch_ints(e->n, Nh)));
        HIPCHK(launch_reestimate_3pt(e->pts(), labels_dev, Nh, e->epi, H_dev, counts_dev, e->r3_scratch.p, e->stream,
                                     e->tune_3pt_form));
        return MH_OK;
    }
    Affines a{ e->a11.p, e->a12.p, e->a21.p, e->a22.p };
    HIPCHK(launch_reestimate(e->pts(), a, labels_dev, Nh, e->epi, H_dev, counts_dev, e->stream));
    return MH_OK;
}

} // namespace mhe

extern "C" {

int mh_set_estimator(mh_engine* e, int estimator)
{
    return guarded([&]() -> int {
    int rc = enter(e);
    if (rc) return rc;
    if (estimator != MH_ESTIMATOR_HAF && estimator != MH_ESTIMATOR_3PT && estimator != MH_ESTIMATOR_DLT)
        return fail(MH_ERR_INVALID, "unknown estimator");
    e->estimator = estimator;
    return MH_OK;
    });
}

int mh_set_estimator_reweighting(mh_engine* e, int rounds, double c2)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (rounds < 0 || rounds > REWEIGHT_H_MAX_ROUNDS) return fail(MH_ERR_INVALID, "rounds outside [0, 16]");
    if (rounds > 0 && (!(c2 > 0.0) || !std::isfinite(c2)))
        return fail(MH_ERR_INVALID, "c2 is not a finite positive number");
    e->est_rw_rounds = rounds;
    e->est_rw_c2 = rounds > 0 ? c2 : 0.0;
    e->est_rw_auto = false;                      // of the two setters the last call decides
    return MH_OK;
    });
}

int mh_set_estimator_reweighting_auto(mh_engine* e, int rounds, int num, int den, double kappa2, double c2_min, double c2_max)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (rounds < 0 || rounds > REWEIGHT_H_MAX_ROUNDS) return fail(MH_ERR_INVALID, "rounds outside [0, 16]");
    const AutoScale a{ num, den, kappa2, c2_min, c2_max };
    if (rounds > 0 && !autoscale_ok(a))
        return fail(MH_ERR_INVALID, "num / den outside 0 <= num <= den <= 65536, kappa2 not finite and > 0, or bounds not finite with 0 < c2_min <= c2_max");
    e->est_rw_rounds = rounds;
    e->est_rw_c2 = 0.0;
    e->est_rw_auto = rounds > 0;
    if (rounds > 0) e->est_rw_scale = a;
    return MH_OK;
    });
}

int mh_set_data_term(mh_engine* e, int term)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (term != MH_DATA_TERM_REFERENCE && term != MH_DATA_TERM_RISING) return fail(MH_ERR_INVALID, "unknown data term");
    e->data_term = term;
    e->cost_L = 0;                                               // as mh_set_params: the table on the device is another term's
    return MH_OK;
    });
}

int mh_set_residual_scope(mh_engine* e, int scope)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (scope != MH_RESIDUAL_SCOPE_SCORE && scope != MH_RESIDUAL_SCOPE_ROUTE) return fail(MH_ERR_INVALID, "unknown residual scope");
    e->residual_scope = scope;
    e->cost_L = 0;                                               // as mh_set_data_term: the table on the device may be another error's
    return MH_OK;
    });
}

int mh_reestimate(mh_engine* e, const int* labels, double* H_out)
{
    return guarded([&]() -> int {
    int rc = require_models(e);
    if (rc) return rc;
    if (!labels) return fail(MH_ERR_INVALID, "labels is null");
    if (e->estimator == MH_ESTIMATOR_HAF && !e->have_aff) return fail(MH_ERR_NOT_SET, "affinities are not set");
    if (e->estimator != MH_ESTIMATOR_DLT && !e->have_epi) return fail(MH_ERR_NOT_SET, "fundamental matrix / epipole are not set");
    HIPCHK(e->labels_pts.reserve(e->n));
    HIPCHK(e->label_counts.reserve(e->m));
    HIPCHK(hipMemcpyAsync(e->labels_pts.p, labels, sizeof(int) * e->n, hipMemcpyHostToDevice, e->stream));
    rc = launch_estimator(e, e->labels_pts.p, e->m, e->H.p, e->label_counts.p);
    if (rc) return rc;
    e->cost_L = 0;
    if (H_out) {
        HIPCHK(hipMemcpyAsync(H_out, e->H.p, sizeof(double) * 9 * e->m, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return MH_OK;
    });
}

int mh_labeling_step(mh_engine* e, int warm, int* labeling, double* energy, int* cycles)
{
    return guarded([&]() -> int {
    int rc = require_models(e);
    if (rc) return rc;
    if (!labeling) return fail(MH_ERR_INVALID, "labeling is null");
    if (e->estimator == MH_ESTIMATOR_HAF && (!e->have_aff || !e->have_epi))
        return fail(MH_ERR_NOT_SET, "affinities / epipolar geometry are not set");
    if (e->estimator != MH_ESTIMATOR_DLT && !e->have_epi) return fail(MH_ERR_NOT_SET, "epipolar geometry is not set");
    rc = do_data_cost(e);
    if (rc) return rc;
    const int* init_dev = nullptr;
    const dim3 grid((e->n + 255) / 256), blk(256);
    if (warm) {                                                   // M/MultiH.cpp:525-529
        for (int i = 0; i < e->n; ++i)
            if (labeling[i] < -1 || labeling[i] >= e->m)
                return fail(MH_ERR_INVALID, "warm-start label out of range -1..Nh-1");
        HIPCHK(e->labels_in.reserve(e->n));
        HIPCHK(hipMemcpyAsync(e->labels_in.p, labeling, sizeof(int) * e->n, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(k_shift_labels, grid, blk, 0, e->stream, e->n, e->labels_in.p, 1, e->labels_in.p);
        init_dev = e->labels_in.p;
    }
    long long en = 0;
    rc = do_expand(e, init_dev, &en, cycles);
    if (rc) return rc;
    HIPCHK(e->labels_pts.reserve(e->n));
    HIPCHK(e->label_counts.reserve(e->m));
    hipLaunchKernelGGL(k_shift_labels, grid, blk, 0, e->stream, e->n, e->ew_label.p, -1, e->labels_pts.p); // :547-568
    rc = launch_estimator(e, e->labels_pts.p, e->m, e->H.p, e->label_counts.p);
    if (rc) return rc;
    e->cost_L = 0;                                               // models changed
    HIPCHK(hipMemcpyAsync(labeling, e->labels_pts.p, sizeof(int) * e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (energy) *energy = (double)en;
    return MH_OK;
    });
}

static_assert(MH_MERGE_OK == MERGE_OK && MH_MERGE_EMPTY == MERGE_EMPTY && MH_MERGE_NO_FIT == MERGE_NO_FIT, "status codes of merge_energy.hip");

// Writes the me_ staging buffers and nothing else of the engine (the definition: include/multih_hip.h).
int mh_merge_deltas(mh_engine* e, const int* labels, const int* pairs, int npairs, double* H_out, long long* delta, long long* parts,
                    int* status)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (npairs < 0 || npairs > MH_MERGE_MAX_PAIRS) return fail(MH_ERR_INVALID, "npairs outside [0, 2^20]");
    if (npairs > 0 && (!labels || !pairs || !delta || !status)) return fail(MH_ERR_INVALID, "null argument");
    int rc = require_models(e);
    if (rc) return rc;
    if (!e->have_graph) return fail(MH_ERR_NOT_SET, "neighbour graph is not set");
    if (npairs == 0) return MH_OK;
    for (int k = 0; k < npairs; ++k) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 0 || b >= e->m || a >= b) return fail(MH_ERR_INVALID, "a pair is not 0 <= a < b < Nh");
    }
    const size_t np = (size_t)npairs;
    HIPCHK(e->me_labels.reserve(e->n)); HIPCHK(e->me_pairs.reserve(2 * np)); HIPCHK(e->me_status.reserve(np));
    HIPCHK(e->me_H.reserve(9 * np)); HIPCHK(e->me_out.reserve(5 * np));
    HIPCHK(hipMemcpyAsync(e->me_labels.p, labels, sizeof(int) * e->n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->me_pairs.p, pairs, sizeof(int) * 2 * np, hipMemcpyHostToDevice, e->stream));
    const Graph g{ e->d_rowptr.p, e->d_col.p, e->w_dev(), e->d_rev.p, e->n, e->g_nnz, e->d_order.p, e->d_wsum.p };
    HIPCHK(launch_merge_pairs(e->pts(), e->me_labels.p, e->H.p, e->me_pairs.p, npairs, g, e->lambda, e->thr_H * e->thr_H, e->me_H.p,
                              e->me_out.p, e->me_status.p, e->stream, e->data_term == MH_DATA_TERM_RISING, e->route_symmetric()));
    std::vector<double> h_H(H_out ? 9 * np : 0);
    std::vector<long long> h_out(5 * np);
    HIPCHK(hipMemcpyAsync(status, e->me_status.p, sizeof(int) * np, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(h_out.data(), e->me_out.p, sizeof(long long) * 5 * np, hipMemcpyDeviceToHost, e->stream));
    if (H_out) HIPCHK(hipMemcpyAsync(h_H.data(), e->me_H.p, sizeof(double) * 9 * np, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < np; ++k) {            // a pair that is not OK leaves its rows of H_out and parts as they were
        if (status[k] != MH_MERGE_OK) { delta[k] = 0x7fffffffffffffffll; continue; }
        delta[k] = h_out[5 * k + 4];
        if (parts) std::memcpy(parts + 4 * k, &h_out[5 * k], sizeof(long long) * 4);
        if (H_out) std::memcpy(H_out + 9 * k, &h_H[9 * k], sizeof(double) * 9);
    }
    return MH_OK;
    });
}

int mh_labeling_energy(mh_engine* e, const int* labels, long long* energy, long long* parts)
{
    return guarded([&]() -> int {
    int rc = require_models(e);
    if (rc) return rc;
    if (!e->have_graph) return fail(MH_ERR_NOT_SET, "neighbour graph is not set");
    if (!labels || !energy) return fail(MH_ERR_INVALID, "null argument");
    for (int i = 0; i < e->n; ++i)
        if (labels[i] < -1 || labels[i] >= e->m) return fail(MH_ERR_INVALID, "label out of range -1..Nh-1");
    HIPCHK(e->me_labels.reserve(e->n)); HIPCHK(e->me_out.reserve(2));
    HIPCHK(hipMemcpyAsync(e->me_labels.p, labels, sizeof(int) * e->n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->me_out.p, 0, sizeof(long long) * 2, e->stream));
    const Graph g{ e->d_rowptr.p, e->d_col.p, e->w_dev(), e->d_rev.p, e->n, e->g_nnz, e->d_order.p, e->d_wsum.p };
    HIPCHK(launch_labeling_energy(e->pts(), e->me_labels.p, e->H.p, g, e->lambda, e->thr_H * e->thr_H,
                                  reinterpret_cast<unsigned long long*>(e->me_out.p), e->stream, e->data_term == MH_DATA_TERM_RISING,
                                  e->route_symmetric()));
    long long out[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(out, e->me_out.p, sizeof(long long) * 2, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *energy = out[0] + out[1];
    if (parts) { parts[0] = out[0]; parts[1] = out[1]; }
    return MH_OK;
    });
}

static_assert(MH_DROP_OK == DROP_OK && MH_DROP_EMPTY == DROP_EMPTY, "status codes of label_cost.hip");

// The labels checked against -1..Nh-1 and the used flags counted in the same walk; both uploaded (me_labels, lc_used), and the
// arg-min launched into lc_alt / lc_cost (alt_cost, then own_cost).  Writes staging buffers and nothing else of the engine.
static int best_alternative_on_device(mh_engine* e, const int* labels)
{
    std::vector<int> used(e->m, 0);
    for (int i = 0; i < e->n; ++i) {
        if (labels[i] < -1 || labels[i] >= e->m) return fail(MH_ERR_INVALID, "label out of range -1..Nh-1");
        if (labels[i] >= 0) used[labels[i]] = 1;
    }
    const size_t n = (size_t)e->n;
    HIPCHK(e->me_labels.reserve(n)); HIPCHK(e->lc_used.reserve(e->m)); HIPCHK(e->lc_alt.reserve(n)); HIPCHK(e->lc_cost.reserve(2 * n));
    HIPCHK(hipMemcpyAsync(e->me_labels.p, labels, sizeof(int) * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->lc_used.p, used.data(), sizeof(int) * e->m, hipMemcpyHostToDevice, e->stream));
    HIPCHK(launch_best_alternative(e->pts(), e->me_labels.p, e->H.p, e->m, e->lc_used.p, e->lambda, e->thr_H * e->thr_H, e->lc_alt.p,
                                   e->lc_cost.p, e->lc_cost.p + n, e->stream, e->data_term == MH_DATA_TERM_RISING, e->route_symmetric()));
    HIPCHK(hipStreamSynchronize(e->stream));     // `used` is pageable host memory of this frame
    return MH_OK;
}

int mh_best_alternative(mh_engine* e, const int* labels, int* alt, int* alt_cost, int* own_cost)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (!labels || !alt) return fail(MH_ERR_INVALID, "null argument");
    int rc = require_models(e);
    if (rc) return rc;
    rc = best_alternative_on_device(e, labels);
    if (rc) return rc;
    const size_t n = (size_t)e->n;
    HIPCHK(hipMemcpyAsync(alt, e->lc_alt.p, sizeof(int) * n, hipMemcpyDeviceToHost, e->stream));
    if (alt_cost) HIPCHK(hipMemcpyAsync(alt_cost, e->lc_cost.p, sizeof(int) * n, hipMemcpyDeviceToHost, e->stream));
    if (own_cost) HIPCHK(hipMemcpyAsync(own_cost, e->lc_cost.p + n, sizeof(int) * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MH_OK;
    });
}

int mh_drop_deltas(mh_engine* e, const int* labels, const int* cand, int ncand, long long* delta, long long* parts, int* status,
                   int* alt_out)
{
    return guarded([&]() -> int {
    if (!e) return fail(MH_ERR_INVALID, "null engine");
    if (ncand < 0) return fail(MH_ERR_INVALID, "ncand outside [0, Nh]");
    if (ncand > 0 && (!labels || !cand || !delta || !status)) return fail(MH_ERR_INVALID, "null argument");
    int rc = require_models(e);
    if (rc) return rc;
    if (!e->have_graph) return fail(MH_ERR_NOT_SET, "neighbour graph is not set");
    if (ncand > e->m) return fail(MH_ERR_INVALID, "ncand outside [0, Nh]");
    if (ncand == 0) return MH_OK;
    for (int k = 0; k < ncand; ++k)
        if (cand[k] < 0 || cand[k] >= e->m) return fail(MH_ERR_INVALID, "a candidate is outside [0, Nh)");
    rc = best_alternative_on_device(e, labels);
    if (rc) return rc;
    const size_t nc = (size_t)ncand, n = (size_t)e->n;
    HIPCHK(e->lc_cand.reserve(nc)); HIPCHK(e->me_status.reserve(nc)); HIPCHK(e->me_out.reserve(5 * nc));
    HIPCHK(hipMemcpyAsync(e->lc_cand.p, cand, sizeof(int) * nc, hipMemcpyHostToDevice, e->stream));
    const Graph g{ e->d_rowptr.p, e->d_col.p, e->w_dev(), e->d_rev.p, e->n, e->g_nnz, e->d_order.p, e->d_wsum.p };
    HIPCHK(launch_drop_labels(e->pts(), e->me_labels.p, e->H.p, e->lc_cand.p, ncand, e->lc_alt.p, e->lc_cost.p, g, e->lambda,
                              e->thr_H * e->thr_H, e->me_out.p, e->me_status.p, e->stream, e->data_term == MH_DATA_TERM_RISING,
                              e->route_symmetric()));
    std::vector<long long> h_out(5 * nc);
    HIPCHK(hipMemcpyAsync(status, e->me_status.p, sizeof(int) * nc, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(h_out.data(), e->me_out.p, sizeof(long long) * 5 * nc, hipMemcpyDeviceToHost, e->stream));
    if (alt_out) HIPCHK(hipMemcpyAsync(alt_out, e->lc_alt.p, sizeof(int) * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < nc; ++k) {            // a candidate that is not OK leaves its row of parts as it was
        if (status[k] != MH_DROP_OK) { delta[k] = 0x7fffffffffffffffll; continue; }
        const long long* o = &h_out[5 * k];
        delta[k] = o[2] - o[1] + o[4] - o[3];
        if (parts) std::memcpy(parts + 5 * k, o, sizeof(long long) * 5);
    }
    return MH_OK;
    });
}

} // extern "C"
