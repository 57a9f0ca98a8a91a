// capi_engine.hpp — what the translation units of the C ABI share: the engine object, error plumbing and the helpers that
// several entry-point families use.  Internal: nothing here is part of include/multih_hip.h.
//   capi.hip          life cycle, parameters, correspondences, neighbourhood graph, buffers, profiling, tuning keys
//   capi_front.hip    epipolar front half, per-point homographies, mean shift          
//   capi_score.hip    propose, model sets, score / residual matrix / cost matrix, prefetch queue, inlier read-outs
//   capi_propose.hip  HAF proposals: a hypothesis per affine correspondence (mh_propose_haf, mh_get_haf_support); 3-point proposals (mh_propose_3pt)
//   capi_select.hip   transport, greedy selection, best model of a batch (the score exchange)
//   capi_label.hip    data cost, alpha-expansion, re-estimation, LabelingStep, post-filter statistics
//
// Ownership: every HIP resource of an engine sits in an owner defined here (DevBuf, PinnedBuf, Stream, Event) whose destructor
// gives it back; the capi*.hip files allocate, create, free and destroy nothing themselves, and mh_destroy is: set the device,
// quiesce, resolve the timers, delete the engine.  (e->stream is a raw handle: it may be the caller's.)
// The resident batch: what the model set is — how many models, who proposed them, whether their samples are resident — is one
// record (ResidentBatch); drop_models and install_models are the only code that writes it and what hangs on it (cost_L,
// counts_fresh, models_seq).  Every entry point that installs a model set validates its arguments with the resident set
// untouched, then: drop_models, reserve, launch or copy, install_models.  So after a failed allocation or launch inside an
// installer the engine holds an EMPTY model set, on every route: never a record of buffers that were freed or swapped.
#pragma once
#include "../../include/multih_hip.h"
#include "mh_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

using namespace mh;

// text of the last error on this thread (mh_last_error)
extern thread_local std::string g_err;

inline int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(MH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// No owner can be copied (a copy would give its resource back twice); DevBuf and Event can be moved, and a moved-from one holds nothing.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

template <class T>
struct DevBuf : NoCopy {
    T* p = nullptr;
    size_t cap = 0;        // elements
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }     // (o frees what this held)
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
};

// A pinned host block: device-mapped (the device's address of it in d) or plain pinned (the target of copies; d stays null).
// Allocated on first use, zeroed; a larger request later replaces it (contents are not kept).
template <class T>
struct PinnedBuf : NoCopy {
    T* h = nullptr;
    T* d = nullptr;
    size_t cap = 0;        // elements
    ~PinnedBuf() { if (h) (void)hipHostFree(h); }
    hipError_t ensure(size_t n, bool mapped = true)
    {
        if (n <= cap) return hipSuccess;
        if (h) { (void)hipHostFree(h); h = d = nullptr; cap = 0; }
        hipError_t e = hipHostMalloc((void**)&h, n * sizeof(T), mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e == hipSuccess && mapped) e = hipHostGetDevicePointer((void**)&d, h, 0);
        if (e != hipSuccess) { if (h) (void)hipHostFree(h); h = d = nullptr; return e; }
        std::memset(h, 0, n * sizeof(T));
        cap = n;
        return hipSuccess;
    }
};

struct Event : NoCopy {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(ev, o.ev); return *this; }
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};

struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    hipError_t ensure(bool highest_priority = false)
    {
        if (s) return hipSuccess;
        if (!highest_priority) return hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        int lo = 0, hi = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        return e != hipSuccess ? e : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi);
    }
    operator hipStream_t() const { return s; }
};

// The buffers of ONE context of the alpha-expansion (ExpandWork::Ctx, mh_kernels.hpp); the engine holds sixteen, all alike.
// A context packs its arrays by kind: `arcs` holds cap and sent, `sites` excess, sink_cap, height, decided and — when asked
// for — the took list, each array at a multiple of 64 ints (the 256 bytes a buffer of its own would be aligned to); core,
// took, the control words and the accumulators are buffers of their own.  In ints that is 2 nnz + 13 n and change: the
// figure expand_contexts (capi_label.hip) bounds.  Fresh memory is cleared once: a context's capacities and flow counters
// are read for arcs the current move has not written only together with verdicts that make them irrelevant (expand.hip), but
// the control words' rings and tickets must start at zero (k_ctl_init) and nothing is gained by leaving the rest to chance.
struct ExpandCtxBufs {
    DevBuf<int> arcs, sites, core, flags;
    DevBuf<long long> acc;
    DevBuf<unsigned char> took;
    static size_t pitch(int count) { return ((size_t)count + 2 + 63) & ~(size_t)63; }
    hipError_t reserve(int n, int nnz, bool with_took_list, hipStream_t stream)
    {
        auto grow = [&](auto& buf, size_t count) -> hipError_t {
            const size_t had = buf.cap;
            hipError_t e = buf.reserve(count);
            if (e == hipSuccess && buf.cap != had) e = hipMemsetAsync(buf.p, 0, sizeof(*buf.p) * buf.cap, stream);
            return e;
        };
        hipError_t e = grow(arcs, 2 * pitch(nnz));
        if (e == hipSuccess) e = grow(sites, (with_took_list ? 5 : 4) * pitch(n));
        if (e == hipSuccess) e = grow(core, (size_t)EXPAND_CORE_SHARDS * n);
        if (e == hipSuccess) e = grow(flags, EXPAND_FLAG_WORDS);
        if (e == hipSuccess) e = grow(acc, EXPAND_ACC_WORDS);
        if (e == hipSuccess) e = grow(took, (size_t)n + 2);
        return e;
    }
    // the eleven pointers for a graph of n sites and nnz arcs that reserve() was last called for (or a smaller one)
    ExpandWork::Ctx view(int n, int nnz) const
    {
        const size_t pa = pitch(nnz), ps = pitch(n);
        ExpandWork::Ctx x{};
        x.cap = arcs.p; x.sent = arcs.p + pa;
        x.excess = sites.p; x.sink_cap = sites.p + ps; x.height = sites.p + 2 * ps; x.decided = sites.p + 3 * ps;
        x.took_list = sites.cap >= 5 * ps ? sites.p + 4 * ps : nullptr;
        x.took = took.p; x.core = core.p; x.flags = flags.p; x.acc = acc.p;
        return x;
    }
};

struct KernelTimer {
    std::vector<std::pair<Event, Event>> pending;
    int launches = 0;
    double total_ms = 0.0;
};

// The resident model set: the one record of it.  Written by drop_models / install_models (below) and by nothing else.
enum class BatchOrigin { GIVEN, DLT4, HAF, P3 };      // the caller's models (mh_set_models), or none; mh_propose_dlt4 / mh_adopt_prefetched; mh_propose_haf; mh_propose_3pt
struct ResidentBatch {
    int m = 0;
    BatchOrigin origin = BatchOrigin::GIVEN;           // travels in the selection records' mode word (the table beside SelRecord, mh_kernels.hpp)
    int haf_members = 0;                               // of a HAF batch: the `members` it was proposed with
    bool have_samples = false;                         // `samples` holds the batch's index tuples (mh_get_samples)
};

// A counts buffer that waits for its turn: two of them beside the current one (mh_engine::counts, counts_zeroed)
struct CountsSlot {
    DevBuf<int> buf;
    bool zeroed = false;                               // cleared behind the exchange that last read it (the next sweep skips its memset)
    int wait = -1;                                     // which ev_x that exchange records (-1: none)
};

struct mh_engine : ResidentBatch {                    // (e->m, e->origin, e->haf_members, e->have_samples: read anywhere)
    int device = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;                      // where the engine enqueues: own_stream, or the caller's (mh_set_stream) — not owned
    // MultiH ctor members, M/MultiH.cpp:10-21
    double thr_F = 3.0, thr_H = 2.5, locality = 0.002, lambda = 0.5;
    int min_inliers = 0;

    int n = 0;
    bool have_aff = false, have_epi = false, have_graph = false;
    DevBuf<double> x1, y1, x2, y2, a11, a12, a21, a22;
    Epipolar epi{};

    // symmetric weighted graph
    std::vector<int> g_rowptr, g_col, g_mult, g_rev;   // host copy of the symmetric graph (built here by the fallback path, else fetched on demand)
    bool g_host_valid = false;
    std::vector<int> g_w;                    // host copy of the weights in force (mh_get_sym_graph), fetched on demand:
    bool g_w_valid = false;                  //   every change of the graph or of the rule makes it stale
    int g_nnz = 0;
    DevBuf<int> gb_deg, gb_start, gb_cursor, gb_raw, gb_mult, gb_uniq, gb_info, gb_hits_rp, gb_hits_col;   // graph.hip scratch
    int order_n = -1;                        // d_order holds the solver's site order for this many sites
    DevBuf<int> d_rowptr, d_col, d_mult, d_rev;   // (d_mult: the hit multiplicities, what launch_sym_finish / upload_graph fill)
    // mh_set_smoothness_weights (sticky): under MH_SMOOTH_CAUCHY d_wq holds mult x q and is what the labeling reads; under
    // MH_SMOOTH_UNIFORM the labeling reads d_mult itself.  k_arc_weights writes the spare pair, which is swapped in on success.
    int smooth_rule = MH_SMOOTH_UNIFORM, smooth_q_max = 1;
    double smooth_rho = 0.0;
    DevBuf<int> d_wq, d_wq_spare, d_wsum_spare, aw_flag;
    const int* w_dev() const { return smooth_rule == MH_SMOOTH_CAUCHY ? d_wq.p : d_mult.p; }

    // model set (its record: ResidentBatch)
    DevBuf<double> H, H_one;
    DevBuf<int> samples, counts;
    DevBuf<unsigned> haf_used;               // per hypothesis of a HAF batch, the mask of consistent neighbours (mh_get_haf_support)
    DevBuf<double> R;
    long long ldr = 0;
    DevBuf<int> C;                            // mh_cost_matrix
    long long ldc = 0;
    DevBuf<unsigned char> mask;
    DevBuf<double> rh_H;                      // mh_refit_homography: H_in and H_out (18 doubles),
    DevBuf<unsigned char> rh_mask;            // the inlier flags of H_out (n bytes),
    DevBuf<int> rh_out;                       // its inlier count and the fits accepted
    DevBuf<int> ph_labels, ph_info;           // mh_polish_homographies: the labels (n) and per model members, iterations, steps, status,
    DevBuf<double> ph_H, ph_cost;             // H_in and H_out (2 x m x 9), S before and after (m x 2)
    DevBuf<int> rw_labels, rw_info;           // mh_reweight_homographies: the labels (n) and per model members, support, rounds, status,
    DevBuf<double> rw_H, rw_gain;             // H_in and H_out (2 x m x 9), W before and after (m x 2); mh_reweight_homographies_auto: then the
                                              //   scales (m x 2); mh_label_residual_quantile: the labels, H, d2_out in rw_gain, info
    DevBuf<int> me_labels, me_pairs, me_status;   // mh_merge_deltas / mh_labeling_energy: the labels (n), the pairs (npairs x 2), their status,
    DevBuf<double> me_H;                      // the unions' fits (npairs x 9),
    DevBuf<long long> me_out;                 // per pair |S|, data_old, data_new, cut, delta; mh_labeling_energy: data, smooth
    DevBuf<int> lc_used, lc_cand, lc_alt, lc_cost;    // mh_best_alternative / mh_drop_deltas (labels in me_labels, status in me_status, sums in
                                              //   me_out): the used flags (m), the candidates, alt (n), alt_cost | own_cost (2 n)
    DevBuf<double> moments, min_eig;
    DevBuf<double> cp_pts, cp_H, cp_out;     // mh_compat_trial_stats staging
    DevBuf<int> cp_begin, cp_tri;
    DevBuf<int> cp_idx;                      // mh_compat_dlt_medians: the trials' 4-tuples (it stages its points in cp_pts, its fits in cp_H, its values in cp_out)
    DevBuf<unsigned char> cp_ok;
    // greedy selection (select.hip): two candidate lists, control words, exchange buffers
    DevBuf<int> sel_orig[2], sel_counts, sel_carried[2], sel_left, sel_rec, sel_scores, sel_gathered;     // (sel_carried / sel_left: r05, the decremental rounds of mh_select_greedy)
    DevBuf<int> sel_weights, sel_carried_w[2], sel_left_w;     // mh_select_greedy_msac: the candidates' weights beside sel_counts / sel_carried / sel_left
    DevBuf<double> sel_cand_H[2], sel_out_H;
    DevBuf<SelRecord> sel_records;             // [0] this rank's offer, [1 .. world] the gathered offers
    DevBuf<long long> sel_counter;
    DevBuf<unsigned long long> sel_keys;
    // transport of the sharded propose stage (mh_set_transport): stream-ordered (RCCL) or host-synchronised (test hook)
    int t_rank = 0, t_world = 1;
    mh_allgather_stream_fn t_stream_fn = nullptr;
    mh_allgather_dev_fn t_host_fn = nullptr;
    void* t_ctx = nullptr;
    // pipelined propose (mh_prefetch_dlt4): the spare batch and the second stream it is prepared on
    Stream side_stream;
    Event ev_main, ev_side_pre;
    int tune_score32_resident = 12;          // key 24: the FP32 pre-test score as a resident grid with n point slices (12: 1.98 ms against 2.14 hardware-dispatched at 50k x 100k, tools/score32_probe.py); 0 = hardware dispatch, -1 = ~37 500 items
    int occ_score32 = -1, occ_cost32 = -1;   // workgroups per compute unit of the resident score / cost kernels on THIS engine's device (-1: not asked yet)
    int tune_cost32_batched = 0;             // key 28: 1 = experiment: k_cost32 evaluates the near pairs of several models together (score32.hip, cost32_wg_batched; slower: 4.45 vs 4.10 ms)
    int tune_cost32_slice_major = 0;         // key 27: the resident cost-matrix kernel takes its items slice-major (experiment)
    int tune_sweep_slices = 0;               // key 26: > 0 = the resident sweep takes its items slice-major with this many point slices (experiment)
    int tune_dlt_variant = 0;                // key 25: 0 = by context (below), 1 = the LDS-staged proposer everywhere, 2 = the register-resident one everywhere (same bits)
    int tune_cost32_resident = 8;            // key 23: the int32 cost matrix as a resident grid with n point slices (8: 4.12 ms against 4.25 hardware-dispatched at 50k x 100k, tools/cost32_probe.py); 0 = hardware dispatch, -1 = ~37 500 items
    int tune_stream_shift = 0;               // key 22 (experiment): dummy streams created in front of the second / third stream (shifts their hardware queue / pipe)
    Stream dummy_streams[16];                // (key 22 admits 0 .. 16)
    int tune_dlt_first = 1;                  // key 20: the sweep waits until the second stream has reached the pending DLT's dispatch (1) or not (0)
    // up to two prefetched batches wait in a FIFO (r04: with the batch after next prepared too, the DLT a sweep has to wait
    // for was dispatched a whole sweep earlier — nothing is handed from stream to stream between two sweeps)
    static constexpr int PF_DEPTH = 2;
    DevBuf<double> pf_H[PF_DEPTH];
    DevBuf<int> pf_samples[PF_DEPTH];
    int pf_m[PF_DEPTH] = { 0, 0 };
    Event pf_ev[PF_DEPTH];                               // recorded behind the slot's DLT on the second stream
    int pf_head = 0, pf_count = 0;                       // oldest queued slot, number of queued batches
    // best model of a scored batch (mh_select_best).  The (all-gather +) arg-max of batch i runs on a third stream behind an
    // event of sweep i, so sweep i+1 starts at once: the batch's counts buffer goes to the exchange and the next sweep
    // writes the other one (r04)
    Stream xchg_stream;
    Event ev_sweep, ev_x[3];
    // two counts buffers wait in a FIFO beside the current one ([0] the longer): a buffer handed to exchange k comes back for sweep
    // k + 3, so an exchange has TWO sweeps to finish in before anything waits for it (with one spare buffer it had one).
    // hand_counts_to_exchange (below) is the hand-over.
    CountsSlot counts_waiting[2];
    long long xchg_calls = 0;                  // exchanges enqueued on xchg_stream so far (parity selects ev_x)
    long long models_seq = 0, best_models_seq = -1;   // model-set generation; the one the last mh_select_best result belongs to
    bool counts_zeroed = false;                // the current counts buffer was cleared behind the exchange that last read it (the next sweep skips its memset)
    bool counts_fresh = false;                 // the current counts buffer holds the scores of the current model set (a scoring call wrote it)
    bool xchg_pending = false;                 // something enqueued on xchg_stream since the last host wait for it
    PinnedBuf<int> h_best;                     // count, global index, sequence number, error word
    int best_seq = 0;
    PinnedBuf<int> h_sel;                      // mirror of the control words
    long long copies_h2d = 0, copies_d2h = 0;  // explicit host<->device copies issued by mh_select_greedy (mh_get_copy_stats)

    // epipolar front half
    int fm = 0;
    int fund_metric = 0;                       // mh_set_fundamental_metric: MH_FUND_SAMPSON / MH_FUND_EPIPOLAR_MAX (changes results: not a tuning key)
    DevBuf<double> fund, fund_one;
    DevBuf<int> fund_samples, fund_counts, fund_inl;
    int fund_tuple = 8;                        // indices per sample in fund_samples: 8 after mh_propose_fund8, 7 after mh_propose_fund7
    int f7_m = 0;                              // samples of the last mh_propose_fund7 (fm = 3 * f7_m slots)
    DevBuf<int> fund_nvalid, fund_stop;        // k_fund7: finite slots per sample; k_ransac_stop: its four words
    DevBuf<unsigned char> fund_mask, ref_keep, ref_in, ref_reason;
    int ref_reason_n = 0;                      // rows of the last mh_refine_correspondences (mh_get_refine_reasons)
    DevBuf<double> ref_out;

    // reference-style initialisation
    DevBuf<double> loc_H, loc_feat, ms_data, ms_mean;
    DevBuf<int> ms_votes, ms_out, ms_list, ms_pcnt, ms_heads, ms_tickets;
    DevBuf<double> ms_partial, ms_partial2;
    DevBuf<unsigned long long> ms_ticks;     // MULTIH_MS_STATS: phase ticks of the persistent kernel
    DevBuf<int> ms_ctl, ms_pcnt2;            // the persistent tail of a mean-shift batch (meanshift.hip, k_ms_persist)
    int ms_persist_per_cu = -1, ms_persist_per_cu6 = -1;   // workgroups of k_ms_persist<10> / <6> a compute unit holds (-1: not queried; a failed query is not kept)
    int tune_select_refine = 0;              // key 30: mh_select_greedy refits each round's winner to its inliers before the claim (0 = off)
    int estimator = MH_ESTIMATOR_HAF;        // mh_set_estimator: the re-estimator of mh_reestimate, mh_labeling_step and the key-30 refit
    int est_rw_rounds = 0;                   // mh_set_estimator_reweighting: > 0 = the MH_ESTIMATOR_DLT re-estimator runs that many reweighted rounds
    double est_rw_c2 = 0.0;                  //   at this scale from each label's standing model (reweight_h.hip) instead of the plain fit; sticky
    bool est_rw_auto = false;                //   mh_set_estimator_reweighting_auto (the last of the two setters decides): the scale of each round is
    AutoScale est_rw_scale{ 1, 2, 1.0, 1.0, 1.0 };   //   taken from the label's residuals by this rule (label_scale.hip)
    int data_term = MH_DATA_TERM_REFERENCE;  // mh_set_data_term: the data term of mh_data_cost, mh_cost_matrix and mh_labeling_step (changes results: not a tuning key)
    DevBuf<int> r3_scratch;                  // member lists of the 3-point re-estimator (reestimate3pt.hip)
    int tune_3pt_form = 0;                   // key 34 (measurement libraries): 0 by size, 1 the match loop, 2 the compacted member lists (reestimate3pt.hip)
    DevBuf<double> sel_refit;                // the refit (9 doubles) and its inlier count
    DevBuf<int> sel_refit_ctr;
    DevBuf<double> ms_rs;                    // the mean-shift index of one call (meanshift.hip, k_ms_indexed): rows in cell order,
    DevBuf<int> ms_order, ms_cells, ms_cursor, ms_cellcount;   // position -> row, cell starts, scatter cursors, cell counts
    int tune_ms_indexed = 1;                 // key 32: climbs through the index, a workgroup each, a launch per batch (0: the launched / persistent schedule)
    int tune_ms_dense = 8;                  // key 33: an indexed climb that meets more members than this in an iteration is handed to the per-group kernels
    long long ms_indexed_launches = 0;
    int tune_ms_persist = 12;                // key 29: the tail runs persistently once at most this many climbs are left (0 = never)
    long long ms_persist_launches = 0, ms_persist_fallbacks = 0, ms_rounds = 0;

    // labeling
    int cost_L = 0;
    DevBuf<int> cost, labels_in, labels_pts, label_counts;
    DevBuf<int> ew_label, ew_cur, ew_trace, ew_saved, d_order, d_wsum;
    int comp_moves = 0;                      // > 0: component diagnostic of the first n moves' cores (mh_set_tuning key 21)
    DevBuf<int> ew_comp, ew_comp_out;
    int trace_moves = 0;                     // > 0: k_solve logs 8 ints per move (mh_set_tuning key 8)
    int detail_move = -1;                    // move whose relabels are logged one by one (key 9)
    ExpandCtxBufs ew_ctx[EXPAND_MAX_CTX];    // the contexts of the alpha-moves in flight; only those in use hold memory
    DevBuf<int> ew_bctl;                     // the batch control words
    PinnedBuf<int> h_batch;                  // k_commit's publication
    int tune_expand_ctx = 16;                // key 37: alpha-moves solved together (1 = one after the other, the form until r05)
    int tune_batch_min_labels = 16;          // key 38: label sets of at least this many labels are batched from the first cycle on (smaller ones from the second)
    int tune_batch_spw = 0;                  // key 39: sites per wave in the setup and reduction launches of a batch of moves (16 / 32 / 64; 0 = by the size of the launch); schedule only
    int cu_count = 256;
    DevBuf<int> sweep_ctl;                   // work counter + exit counter of the resident sweep (cleared by the launch itself)
    int sweep_wg_per_cu = -1;                // workgroups of the materialising sweep a compute unit holds (-1 = not queried yet)
    int tune_sweep_headroom = 0;             // key 19: workgroup slots the resident sweep leaves free beyond its own occupancy (-1 = hardware dispatch)
    int solve_grid_max = 0;                  // workgroups of the solver launch that can be resident at once (0 = not queried yet)
    double longest_barrier_wait_ms = 0.0;    // longest wait at a grid barrier any completed expansion of this engine has seen
    int last_expand_retries = 0;             // restarts of the last expansion after a barrier timeout (shared GPU)
    long long expand_retries_total = 0;      // ... of all expansions of this engine (mh_get_expand_stats word 22)
    int last_solve_grid = 0;                 // workgroups of the solver launch in the attempt that completed
    int inject_select_failure = 0;           // test hook (key 18): the n-th scoring round of the coming greedy selections fails on this rank
    int inject_barrier_timeouts = 0;         // test hook: the next n expansions' first attempts count as timed out
    int inject_solve_failure = 0;            // test hook (key 40): (group << 4) | context of the next expansion's solve marked failed
    PinnedBuf<int> h_flags;
    PinnedBuf<long long> h_acc;
    PinnedBuf<MeanShiftResultBlock> h_ms;      // the result blocks of the mean-shift climbs, then 3 ints per climb (seed rows, list offsets, list lengths)
    PinnedBuf<int> h_ms_list;                  // not mapped: the (row, votes) lists of a batch's climbs, packed (grows with the need)
    DevBuf<double> sel_pts[4];               // the active points of a greedy-selection round, packed (select.hip)
    DevBuf<int> sel_pack_count;
    DevBuf<double> sel_gone[4];              // the points the last claim of a greedy-selection round took out of the support set, packed
    int tune_select_decrement = 1;           // key 36: rounds count their candidates on the points that LEFT and subtract (1, default) or count again on what is left (0): same selection
    int tune_knn_grid = 1;                   // key 31: the k-NN table through the grid over the source image (0 = exhaustive pass)
    DevBuf<int> knn_cell, knn_count, knn_start, knn_orig;
    DevBuf<float> knn_P;
    DevBuf<int> knn_tmp, knn_part_i;
    DevBuf<float> knn_part_d;
    // the proposer's sampler (mh_set_sampler, sticky) and its table (mh_build_sample_neighbours): the dense n x smp_k k-NN table
    // in a buffer of its own — the labeling graph neither feeds it nor sees it; mh_set_correspondences drops it (smp_k = 0)
    int sampler = MH_SAMPLER_UNIFORM, sampler_uniform_per_16 = 0;
    DevBuf<int> smp_nbr;
    int smp_k = 0;
    // what launch_dlt4 gets under the engine's sampler (nbr == null: the uniform kernels)
    Dlt4Local dlt_local() const { return sampler == MH_SAMPLER_LOCAL ? Dlt4Local{ smp_nbr.p, smp_k, sampler_uniform_per_16 } : Dlt4Local{}; }

    bool profiling = false;
    KernelTimer timers[MH_K_COUNT_];
    int tune_residual_variant = 0;
    int tune_ld = 0;                         // measurement builds only: row pitch of R in doubles (0 = residual_ld)
    int tune_score_variant = 0;
    int residual_mode = MH_RESIDUAL_FORWARD;
    int residual_scope = MH_RESIDUAL_SCOPE_SCORE;   // mh_set_residual_scope: which calls follow residual_mode (changes results: not a tuning key)
    // "is the route symmetric": what the data cost, the cost matrix, the moments and the single-model labelling are launched with
    bool route_symmetric() const { return residual_scope == MH_RESIDUAL_SCOPE_ROUTE && residual_mode == MH_RESIDUAL_SYMMETRIC; }
    int tune_ms_batch = 6;                   // mean-shift climb iterations per host round trip
    int tune_reduce = 2;                     // dominance-reduction rounds per launch (0 = off); 2 measured best (loop 0.262 s at 4, 0.250 s at 2)
    int tune_reduce_launches = 1;            // reduction launches per move in front of the solver (1 = the compacting one alone, 2; loop 0.250 vs 0.254 s)
    int tune_recycle = 1;                    // from the second cycle on a label's max-flow starts from the flow its last expansion left (0 = off, A/B)
    int tune_expand[4] = { 128, 512, 1, 256 };
    int tune_cascade_iters = 2;              // key 17: passes of the dominance cascade inside the solver launch (0 = to the fixed point; 2 measured best: 15.6 -> 14.5 ms per LabelingStep at 50k sites)
    int tune_push_mult = 6;                  // push cycles per phase = this x (depth of the last relabel + 3)  // solver: relax rounds per barrier interval, push cycles per phase, push phases per relabel, workgroups
    ExpandStats last_expand{};

    double bbox[4] = { NAN, NAN, NAN, NAN };   // xmin xmax ymin ymax of the source points
    // FP32 pre-test of the score kernels (pretest32.hpp): usable when every coordinate is finite and below 2^20
    bool coords32_ok = false;
    double absmax_x = NAN, absmax_y = NAN, absmax_dst = NAN;
    int tune_score32_tiling = 0;               // key 16: points per lane / models per workgroup of the pre-test kernel (schedule only)
    int tune_score32 = 1;                      // mh_set_tuning key 15: 0 = always the FP64 sweep (A/B; counts are equal by construction)
    DevBuf<float> H32;
    DevBuf<unsigned long long> fb_pairs;
    long long score_pairs = 0;                 // pairs scored through the pre-test since the last reset (mh_get_score_stats)
    long long score_pairs_plain_fp64 = 0;      // ... of which mh_score_msac's plain FP64 form took (all of them through the FP64 formula)
    // mh_score_msac: the weights, a copy of the counts they belong to (the counts buffer itself may go to an exchange: mh_select_best),
    // and the model-set generation both were computed for (-1: none; mh_set_correspondences resets it)
    DevBuf<int> weights, weights_counts;
    long long weights_models_seq = -1;
    PinnedBuf<int> h_best_w;                   // mh_select_best_msac's weight, index, sequence number, error word
    Points pts() const { return Points{ x1.p, y1.p, x2.p, y2.p, n, bbox[0], bbox[1], bbox[2], bbox[3] }; }
};

namespace mhe {

// No exception may cross the C ABI (include/multih_hip.h): host-side allocation failures and
// anything else thrown by the standard library become a status code with the text in mh_last_error.
template <typename Fn>
int guarded(Fn&& fn)
{
    try {
        return fn();
    } catch (const std::bad_alloc&) {
        return fail(MH_ERR_INVALID, "out of host memory");
    } catch (const std::exception& ex) {
        return fail(MH_ERR_INVALID, std::string("internal error: ") + ex.what());
    } catch (...) {
        return fail(MH_ERR_INVALID, "internal error");
    }
}

struct ScopedTimer {
    mh_engine* e;
    int k;
    hipStream_t st;
    Event a, b;
    bool on = false;                                   // both events exist and `a` is recorded
    ScopedTimer(mh_engine* e_, int k_, hipStream_t on_stream = nullptr) : e(e_), k(k_), st(on_stream ? on_stream : e_->stream)
    {
        if (!e->profiling || a.ensure(hipEventDefault) != hipSuccess || b.ensure(hipEventDefault) != hipSuccess) return;
        (void)hipEventRecord(a, st);
        on = true;
    }
    ~ScopedTimer()
    {
        if (!on) return;
        (void)hipEventRecord(b, st);
        e->timers[k].pending.emplace_back(std::move(a), std::move(b));
    }
};

// ---- the resident batch: the two functions that change it ----
// No model set: what every installer leaves behind when it fails after this point, and what mh_set_correspondences leaves for a
// new point count.  One new generation (models_seq) per installing call — install_models does not count again.
inline void drop_models(mh_engine* e)
{
    static_cast<ResidentBatch&>(*e) = ResidentBatch{};
    e->cost_L = 0;
    e->counts_fresh = false;
    ++e->models_seq;
}

// The buffers hold the batch: commit its record (behind drop_models, the reservations and the launch or copy).
inline void install_models(mh_engine* e, int m, BatchOrigin origin, bool have_samples, int haf_members = 0)
{
    static_cast<ResidentBatch&>(*e) = ResidentBatch{ m, origin, haf_members, have_samples };
}

// ---- the counts buffers ----
// a scoring call has written the current buffer
inline void counts_scored(mh_engine* e) { e->counts_fresh = true; e->counts_zeroed = false; }

// The current buffer stays with the exchange that records ev_x[par] and clears it; the buffer that has waited longest becomes the
// current one.  Returns which ev_x the main stream has to wait for before it writes that one (-1: none).
inline int hand_counts_to_exchange(mh_engine* e, int par)
{
    CountsSlot* w = e->counts_waiting;
    const int wait = w[0].wait;
    std::swap(e->counts, w[0].buf);
    e->counts_zeroed = w[0].zeroed;
    w[0].zeroed = true;
    w[0].wait = par;
    std::swap(w[0], w[1]);
    return wait;
}

// ---- shared helpers (defined in capi.hip unless noted) ----
void resolve_timers(mh_engine* e);
int enter(mh_engine* e);
int require_points(mh_engine* e);
int require_models(mh_engine* e);
int require_models_or_empty_shard(mh_engine* e, bool* empty);
hipError_t reserve_counts(mh_engine* e, size_t n);
int quiesce(mh_engine* e);
int join_xchg(mh_engine* e);
// inlier counts of m models over the points p: FP32 pre-test where its preconditions hold, the FP64 sweep otherwise (capi_score.hip)
int score_models(mh_engine* e, const Points& p, const double* Hs, int m, double thr2, const unsigned char* dmask, int* counts_dev);
// counts and MSAC weights, k_msac32 behind the pre-test where it is usable, k_msac64 otherwise (capi_score.hip).  Forward
// residual; the caller has checked 256 n against int32.  plain_variant_only: true for the selection ranked by weight, which
// follows score_models' preconditions to the letter; false for mh_score_msac (pretest_usable, capi_score.hip).
int msac_models(mh_engine* e, const Points& p, const double* Hs, int m, double thr2, const unsigned char* dmask, int* counts_dev,
                int* weights_dev, bool plain_variant_only);
// the engine's re-estimator over labels_dev (n ints) for models H_dev (Nh x 9, in place) — HAF, 3-point or N-point DLT (capi_label.hip)
int launch_estimator(mh_engine* e, const int* labels_dev, int Nh, double* H_dev, int* counts_dev);
// the exchange's stream and events (capi_select.hip); the second stream of the prefetch queue and its events (capi_score.hip)
int ensure_xchg_stream(mh_engine* e);
int ensure_side_stream(mh_engine* e);

} // namespace mhe

using namespace mhe;
