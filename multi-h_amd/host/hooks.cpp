// hooks.cpp — the C hook layer over class MultiH (ctypes; plain arrays in and out) for the GPU tests and the tools: the
// mhh_set_* functions write into ONE record of settings for the next mhh_run_process calls of this process (one process per
// GPU), mhh_run_process applies the record to a fresh MultiH, runs Process() and keeps what the mhh_get_* functions hand out.
#include <algorithm>
#include <cstring>

#include "merge_step.h"
#include "multih_internal.h"

using multih::detail::MatFrom9;

namespace {

// What the mhh_set_* functions set.  -1 ("< 0") in a mode stands for the class default: Apply leaves that setter alone.
struct HookSettings {
    // mhh_set_sharding / mhh_set_sharding_stream
    int shard_rank = 0, shard_world = 1;
    MultiH::AllGatherFn shard_fn = nullptr;
    MultiH::StreamAllGatherFn shard_stream_fn = nullptr;
    void* shard_ctx = nullptr;
    int device = 0;
    // the neighbourhood: radius > 0 selects the complete radius list, else k > 0 the k nearest hits within 1 / locality; both
    // 0: the class default (k = 16).  max_hits bounds the radius list (<= 0: the default); approx_trees > 0: SetNeighbourApprox
    int knn = 0;
    double radius = 0.0;
    long long max_hits = 0;
    int approx_trees = 0, approx_checks = 32;
    unsigned long long approx_seed = 0;
    std::vector<std::vector<int>> hits;                       // caller-supplied directed hit lists (MultiH::SetNeighbours)
    int post_filter = 1;
    int proposal_refit = 1;
    int proposal_sampler = 0, proposal_sampler_k = 0, proposal_uniform_per_16 = 0;       // default: uniform
    int proposal_source = 0, proposal_haf_members = 16, proposal_haf_stride = 1;         // default: DLT
    std::vector<std::pair<int, int>> tuning;                  // schedule knobs (mh_set_tuning) for the engines
    int fund_metric = -1;
    int fund_estimator = -1, fund_max_samples = 1000;
    double fund_confidence = 0.99;
    int merge_mode = -1;
    double label_cost = 0.0;                                  // (any other value is handed on, so that a bad one fails in Process())
    int data_term = -1, residual = -1, tail_score = -1, tail_refit = -1, tail_polish = -1, model_polish = -1;
    int model_reweight = -1, estimator_reweight = -1, model_reweight_auto = -1, estimator_reweight_auto = -1;
    int estimator = -1, epipolar_free = 0;
    int compat_fit = 0, compat_trials = 501;                  // (COMPAT_FIT_3PT, 501, 0) is the class's default
    double compat_limit_scale = 0.0;
    int selection_score = -1;
    int smoothness_rule = -1, smoothness_q_max = 16;          // mhh_set_smoothness_weights
    double smoothness_rho = 0.0;
    int compat_fits_on_engine = 1;                            // mhh_compatibility_medians_on_engine: 1 = the fits on the device too (as Process() runs it since r06), 0 = on the host

    void Apply(MultiH& mh) const;
};

void HookSettings::Apply(MultiH& mh) const
{
    if (shard_stream_fn) mh.SetShardingStream(shard_rank, shard_world, shard_stream_fn, shard_ctx);
    else mh.SetSharding(shard_rank, shard_world, shard_fn, shard_ctx);
    mh.SetDevice(device);
    mh.SetCompatibilityCheck(post_filter != 0);
    mh.SetProposalRefit(proposal_refit != 0);
    if (proposal_sampler != 0) mh.SetProposalSampler(proposal_sampler, proposal_sampler_k, proposal_uniform_per_16);
    if (proposal_source != 0) mh.SetProposalSource(proposal_source, proposal_haf_members, proposal_haf_stride);
    if (fund_metric >= 0) mh.SetFundamentalMetric(fund_metric);
    if (data_term >= 0) mh.SetDataTerm(data_term);
    if (smoothness_rule >= 0) mh.SetSmoothnessWeights(smoothness_rule, smoothness_rho, smoothness_q_max);
    if (merge_mode >= 0) mh.SetMergeMode(merge_mode);
    if (label_cost != 0.0) mh.SetLabelCost(label_cost);
    if (residual >= 0) mh.SetResidual(residual);
    if (tail_score >= 0) mh.SetTailScore(tail_score);
    if (tail_refit >= 0) mh.SetTailRefit(tail_refit);
    if (tail_polish >= 0) mh.SetTailPolish(tail_polish);
    if (model_polish >= 0) mh.SetModelPolish(model_polish);
    if (model_reweight >= 0) mh.SetModelReweight(model_reweight);
    if (estimator_reweight >= 0) mh.SetEstimatorReweight(estimator_reweight);
    if (model_reweight_auto >= 0) mh.SetModelReweightAuto(model_reweight_auto);
    if (estimator_reweight_auto >= 0) mh.SetEstimatorReweightAuto(estimator_reweight_auto);
    if (selection_score >= 0) mh.SetSelectionScore(selection_score);
    if (estimator >= 0) mh.SetEstimator(estimator);
    mh.SetEpipolarFree(epipolar_free != 0);
    mh.SetCompatibilityFit(compat_fit, compat_trials, compat_limit_scale);
    if (fund_estimator >= 0) mh.SetFundamentalEstimator(fund_estimator, fund_max_samples, fund_confidence);
    for (const auto& kv : tuning) mh.SetEngineTuning(kv.first, kv.second);
    if (radius > 0.0 && max_hits > 0) { mh.SetNeighbourRadius(radius, max_hits); if (knn > 0) mh.SetFallbackK(knn); }
    else if (radius > 0.0) mh.SetNeighbourRadius(radius);
    else if (knn > 0) mh.SetNeighbourK(knn);
    if (approx_trees > 0) mh.SetNeighbourApprox(approx_trees, approx_checks, approx_seed);
}

// What the last mhh_run_process left for the mhh_get_* functions.
struct HookResults {
    int labeling_steps = 0;
    int front_stages[4] = { 0, 0, 0, 0 };
    std::vector<MultiH::MergeLogRecord> merge_log;
    std::vector<MultiH::DropLogRecord> drop_log;
};

HookSettings g_set;
HookResults g_last;

} // namespace

#define MHH_API extern "C" __attribute__((visibility("default")))

MHH_API void mhh_set_sharding(int rank, int world, MultiH::AllGatherFn fn, void* ctx)
{
    g_set.shard_rank = rank; g_set.shard_world = world; g_set.shard_fn = fn; g_set.shard_stream_fn = nullptr; g_set.shard_ctx = ctx;
}
// Stream-ordered transport (RCCL: host/rccl_transport.cpp) for the next mhh_run_process calls; fn = NULL returns to
// whatever mhh_set_sharding set.  world == 1 is allowed: the whole sharded protocol on a one-rank communicator.
MHH_API void mhh_set_sharding_stream(int rank, int world, MultiH::StreamAllGatherFn fn, void* ctx)
{
    g_set.shard_rank = rank; g_set.shard_world = world; g_set.shard_stream_fn = fn; g_set.shard_fn = nullptr; g_set.shard_ctx = ctx;
}
MHH_API void mhh_set_device(int device) { g_set.device = device; }
MHH_API void mhh_set_post_filter(int on) { g_set.post_filter = on; }
MHH_API void mhh_set_neighbourhood(int knn_k, double radius) { g_set.knn = knn_k; g_set.radius = radius; }
// MultiH::SetNeighbourApprox (trees <= 0 switches it off again)
MHH_API void mhh_set_neighbourhood_approx(int trees, int checks, unsigned long long seed)
{
    g_set.approx_trees = trees; g_set.approx_checks = checks; g_set.approx_seed = seed;
}
MHH_API void mhh_set_neighbour_max_hits(long long max_hits) { g_set.max_hits = max_hits; }
// CSR; n <= 0 clears them.  For tools/neighbourhood_sweep.py: which neighbourhood rule reproduces the reference's recorded
// barrsmith result.
MHH_API void mhh_set_neighbour_hits(const int* rowptr, const int* col, int n)
{
    g_set.hits.clear();
    if (n <= 0 || !rowptr || !col) return;
    g_set.hits.resize(n);
    for (int i = 0; i < n; ++i) g_set.hits[i].assign(col + rowptr[i], col + rowptr[i + 1]);
}
MHH_API void mhh_set_proposal_refit(int on) { g_set.proposal_refit = on; }
MHH_API void mhh_set_proposal_sampler(int mode, int k, int uniform_per_16)
{
    g_set.proposal_sampler = mode; g_set.proposal_sampler_k = k; g_set.proposal_uniform_per_16 = uniform_per_16;
}
MHH_API void mhh_set_proposal_source(int source, int members, int stride)
{
    g_set.proposal_source = source; g_set.proposal_haf_members = members; g_set.proposal_haf_stride = stride;
}
// key < 0 clears the list
MHH_API void mhh_set_engine_tuning(int key, int value) { if (key < 0) g_set.tuning.clear(); else g_set.tuning.emplace_back(key, value); }
MHH_API void mhh_set_fundamental_metric(int metric) { g_set.fund_metric = metric; }
// for mhh_run_process and mhh_filter_correspondences
MHH_API void mhh_set_fundamental_estimator(int mode, int max_samples, double confidence)
{
    g_set.fund_estimator = mode; g_set.fund_max_samples = max_samples; g_set.fund_confidence = confidence;
}
MHH_API void mhh_set_merge_mode(int mode) { g_set.merge_mode = mode; }
MHH_API void mhh_set_label_cost(double points) { g_set.label_cost = points; }
MHH_API void mhh_set_data_term(int term) { g_set.data_term = term; }
// MultiH::SetSmoothnessWeights (rule < 0: the class default again)
MHH_API void mhh_set_smoothness_weights(int rule, double rho_px, int q_max)
{
    g_set.smoothness_rule = rule; g_set.smoothness_rho = rho_px; g_set.smoothness_q_max = q_max;
}
MHH_API void mhh_set_residual(int residual) { g_set.residual = residual; }
MHH_API void mhh_set_tail_score(int score) { g_set.tail_score = score; }
MHH_API void mhh_set_tail_refit(int iterations) { g_set.tail_refit = iterations; }
MHH_API void mhh_set_tail_polish(int iterations) { g_set.tail_polish = iterations; }
MHH_API void mhh_set_model_polish(int iterations) { g_set.model_polish = iterations; }
// (scale and kappa: the class defaults)
MHH_API void mhh_set_model_reweight(int rounds) { g_set.model_reweight = rounds; }
MHH_API void mhh_set_estimator_reweight(int rounds) { g_set.estimator_reweight = rounds; }
MHH_API void mhh_set_model_reweight_auto(int rounds) { g_set.model_reweight_auto = rounds; }
MHH_API void mhh_set_estimator_reweight_auto(int rounds) { g_set.estimator_reweight_auto = rounds; }
MHH_API void mhh_set_estimator(int estimator) { g_set.estimator = estimator; }
MHH_API void mhh_set_epipolar_free(int on) { g_set.epipolar_free = on; }
MHH_API void mhh_set_compat_fit(int mode, int trials, double limit_scale)
{
    g_set.compat_fit = mode; g_set.compat_trials = trials; g_set.compat_limit_scale = limit_scale;
}
MHH_API void mhh_set_selection_score(int score) { g_set.selection_score = score; }
MHH_API void mhh_set_compat_fits_on_engine(int on) { g_set.compat_fits_on_engine = on; }

// LabelingSteps the last mhh_run_process ran (MultiH::GetLabelingStepsRun), and its stage table (MultiH::GetFrontStages)
MHH_API int mhh_get_labeling_steps() { return g_last.labeling_steps; }
MHH_API void mhh_get_front_stages(int out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_last.front_stages[i]; }
// records_out: capacity x 9 long long (iteration, models before, pairs, merges accepted, models filtered, E_before, sum_delta,
// E_start, E_expansion), nullable; returns the number of records of the last mhh_run_process
MHH_API int mhh_get_merge_log(long long* records_out, int capacity)
{
    static_assert(sizeof(MultiH::MergeLogRecord) == 9 * sizeof(long long), "a record travels as 9 long long");
    for (int i = 0; records_out && i < capacity && i < (int)g_last.merge_log.size(); ++i)
        std::memcpy(records_out + 9 * (size_t)i, &g_last.merge_log[i], sizeof(MultiH::MergeLogRecord));
    return (int)g_last.merge_log.size();
}
// records_out: capacity x 9 long long (iteration, candidates, dropped label or -1, members, members to the outlier label, delta,
// beta, E_before, E_after), nullable; returns the number of records of the last mhh_run_process
MHH_API int mhh_get_drop_log(long long* records_out, int capacity)
{
    static_assert(sizeof(MultiH::DropLogRecord) == 9 * sizeof(long long), "a record travels as 9 long long");
    for (int i = 0; records_out && i < capacity && i < (int)g_last.drop_log.size(); ++i)
        std::memcpy(records_out + 9 * (size_t)i, &g_last.drop_log[i], sizeof(MultiH::DropLogRecord));
    return (int)g_last.drop_log.size();
}

// test hook (tests/test_gpu_alternation.py): one MergingStep of the product on `engine`, to be compared bit for bit with
// the oracle's mho_merging_step.  kept: capacity nh x 9; returns the number kept or a negative MH_* status.
MHH_API int mhh_merging_step(mh_engine* engine, const double* H, int nh, const double* F, double thr_h, double straightness,
                             unsigned long long seed, double* kept_out, int* changed, unsigned long long* draws)
{
    std::vector<double> kept;
    uint64_t d = 0;
    const int rc = multih::detail::MergingStepOnEngine(engine, H, nh, F, thr_h, straightness, seed, kept, &d);
    if (rc != MH_OK) return rc;
    std::copy(kept.begin(), kept.end(), kept_out);
    if (changed) *changed = (int)(kept.size() / 9) != nh;
    if (draws) *draws = d;
    return (int)(kept.size() / 9);
}

// multih::FilterCorrespondencesByEpipolarGeometry on plain arrays: mask (n flags) out; returns the number kept, -1 on failure
MHH_API int mhh_filter_correspondences(const double* src_xy, const double* dst_xy, int n, double threshold, unsigned long long seed,
                                       int hypotheses, int metric, int device, unsigned char* mask)
{
    std::vector<cv::Point2d> s(n), d(n);
    std::vector<cv::Mat> a(n);
    for (int i = 0; i < n; ++i) {
        s[i] = cv::Point2d(src_xy[2 * i], src_xy[2 * i + 1]);
        d[i] = cv::Point2d(dst_xy[2 * i], dst_xy[2 * i + 1]);
    }
    std::vector<unsigned char> m;
    MultiH::FundEstimator est;
    if (g_set.fund_estimator >= 0) { est.mode = g_set.fund_estimator; est.max_samples = g_set.fund_max_samples; est.confidence = g_set.fund_confidence; }
    if (!multih::FilterCorrespondencesByEpipolarGeometry(s, d, a, threshold, seed, hypotheses, metric, device, &m, est)) return -1;
    for (int i = 0; i < n; ++i) mask[i] = m[i];
    return (int)s.size();
}

// multih::CompatibilityCheck with the trials' order statistics from an engine (mh_compat_trial_stats), as Process() runs
// it, returning the per-cluster median-of-medians too; -1 if the engine fails.  For the GPU tests.
MHH_API int mhh_compatibility_medians_on_engine(mh_engine* engine, const double* src_xy, const double* dst_xy, int n, int* labels, double* H,
                                                int nh, const double* F, double sqr_thr, int min_inliers, unsigned long long seed,
                                                double* medians)
{
    multih::CompatStatsFn fn = [engine, F](const double* pts, const int* begin, int clusters, const int* tri, const double* Ht,
                                           const unsigned char* ok, int trials, double* out) {
        if (!Ht) return mh_compat_trial_stats_fit(engine, pts, begin, clusters, tri, F, trials, out, nullptr, nullptr) == MH_OK;
        return mh_compat_trial_stats(engine, pts, begin, clusters, tri, Ht, ok, trials, out) == MH_OK;
    };
    bool failed = false;
    const int kept = multih::CompatibilityCheck(src_xy, dst_xy, n, labels, H, nh, F, sqr_thr, min_inliers, seed, medians, &fn, &failed,
                                                g_set.compat_fits_on_engine != 0);
    return failed ? -1 : kept;
}

// multih::CompatibilityCheckDlt with the statistics from an engine (mh_compat_dlt_medians), as Process() runs it under
// COMPAT_FIT_DLT, returning the per-cluster medians too (NaN where a cluster got none); -1 if the engine fails.  For the GPU tests.
MHH_API int mhh_compatibility_dlt_on_engine(mh_engine* engine, const double* src_xy, const double* dst_xy, int n, int* labels, double* H,
                                            int nh, double limit, int min_inliers, unsigned long long seed, int trials, double* medians)
{
    if (!multih::detail::LinkedEngineCaps().compat_dlt) return -1;
    const multih::CompatDltFn fn = [engine](const double* pts, const int* begin, int clusters, uint64_t sd, int tr, double* out) {
        return mh_compat_dlt_medians(engine, pts, begin, clusters, sd, 0, tr, out, nullptr, nullptr, nullptr) == MH_OK;
    };
    bool failed = false;
    const int kept = multih::CompatibilityCheckDlt(src_xy, dst_xy, n, labels, H, nh, limit, min_inliers, seed, trials, medians, &fn, &failed);
    return failed ? -1 : kept;
}

// The whole Process() on plain arrays, with the settings of the mhh_set_* functions.  aff == NULL: the point-only route,
// Process(src, dst).  Returns the number of clusters, -1 when Process() fails.
MHH_API int mhh_run_process(const double* src_xy, const double* dst_xy, const double* aff, int n,
                            const double* F, const double* e2, double thr_F, double thr_H, double locality,
                            double lambda, int min_inliers, unsigned long long seed, int hypotheses,
                            int max_models, int fixed_iterations, const double* init_H, int n_init,
                            int* labels_out, double* H_out, int max_H, int* iterations, double* energy,
                            double* loop_seconds, int iter_hypotheses, int iter_max_new)
{
    std::vector<cv::Point2d> s(n), d(n);
    std::vector<cv::Mat> a(n);
    // r06: the affinities as NON-owning 2 x 2 headers over one copy of the caller's array (cv::Mat(rows, cols, type, data): the
    // same with the real library) — 50 000 matrices that each own a 32-byte allocation cost 5 ms to build and to copy, a third
    // of what this hook reported as "Process()" at configs[4].  The copy outlives the call below.
    std::vector<double> aff_copy;
    if (aff) aff_copy.assign(aff, aff + 4 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        s[i] = cv::Point2d(src_xy[2 * i], src_xy[2 * i + 1]);
        d[i] = cv::Point2d(dst_xy[2 * i], dst_xy[2 * i + 1]);
        if (aff) a[i] = cv::Mat(2, 2, CV_64F, aff_copy.data() + 4 * (size_t)i);
    }
    MultiH mh(thr_F, thr_H, locality, lambda, min_inliers);
    if (F && e2) mh.SetEpipolarGeometry(F, e2);
    mh.SetProposal(seed, hypotheses, max_models);
    mh.SetFixedIterations(fixed_iterations);
    mh.SetIterativeProposal(iter_hypotheses, iter_max_new < 0 ? 4 : iter_max_new);
    g_set.Apply(mh);
    if (!g_set.hits.empty() && (int)g_set.hits.size() == n) mh.SetNeighbours(g_set.hits);
    if (iter_max_new < 0) mh.SetInitialisation(MultiH::INIT_STABLE_SETS);      // test hook: negative = reference-style init
    if (init_H && n_init > 0) {
        std::vector<cv::Mat> hs;
        for (int i = 0; i < n_init; ++i) hs.push_back(MatFrom9(init_H + 9 * (size_t)i));
        mh.SetInitialHomographies(hs);
    }
    g_last.merge_log.clear();
    g_last.drop_log.clear();
    if (aff ? !mh.Process(s, d, a) : !mh.Process(s, d)) return -1;
    const MultiH::FrontStages st = mh.GetFrontStages();
    g_last.front_stages[0] = st.input; g_last.front_stages[1] = st.in_ransac_mask; g_last.front_stages[2] = st.triangulated; g_last.front_stages[3] = st.affine_consistent;
    std::vector<int> lab;
    mh.GetLabels(lab);
    for (size_t i = 0; i < lab.size() && i < (size_t)n; ++i) labels_out[i] = lab[i];
    const int k = mh.GetClusterNumber();
    for (int i = 1; i <= k && i <= max_H; ++i) {
        cv::Mat h = mh.GetHomography(i);
        for (int q = 0; q < 9; ++q) H_out[9 * (size_t)(i - 1) + q] = reinterpret_cast<double*>(h.data)[q];
    }
    if (iterations) *iterations = mh.GetIterationNumber();
    if (energy) *energy = mh.GetEnergy();
    if (loop_seconds) *loop_seconds = mh.GetLastLoopSeconds();
    g_last.labeling_steps = mh.GetLabelingStepsRun();
    g_last.merge_log = mh.GetMergeLog();
    g_last.drop_log = mh.GetDropLog();
    return k;
}
