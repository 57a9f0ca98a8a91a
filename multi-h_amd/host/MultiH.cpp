// MultiH.cpp — the reference's orchestrator (M/MultiH.cpp) re-created over the
// gfx950 engine's C ABI.  Every heavy step is one mh_* call; this file holds the
// control flow of Process / ClusterMergingAndLabeling / MergingStep /
// LabelingStep with the reference's stop rules and conventions.
#include "MultiH.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <sstream>

#include "merge_step.h"
#include "multih_internal.h"

using multih::detail::BorrowEngine;
using multih::detail::Check;
using multih::detail::MatFrom9;
using multih::detail::MergingStepOnEngine;
using multih::detail::ReturnEngine;

namespace {

// A matrix that OWNS its storage, filled from a raw array: allocate, then copy.  (cv::Mat(rows, cols, type, ptr) would
// only be a header over the caller's memory.)
cv::Mat OwnedMat(int rows, int cols, const double* v)
{
    cv::Mat m(rows, cols, CV_64F);
    double* p = reinterpret_cast<double*>(m.data);
    for (int i = 0; i < rows * cols; ++i) p[i] = v[i];
    return m;
}

// Points — and, given `aff`, their 2 x 2 affinities row by row — as the flat arrays the engine takes.
struct PackedPoints {
    std::vector<double> s, d, a;
    const double* affinities() const { return a.empty() ? nullptr : a.data(); }
};
PackedPoints PackPoints(const std::vector<cv::Point2d>& src, const std::vector<cv::Point2d>& dst, const std::vector<cv::Mat>* aff = nullptr)
{
    const size_t n = src.size();
    PackedPoints p;
    p.s.resize(2 * n); p.d.resize(2 * n);
    if (aff) p.a.resize(4 * n);
    for (size_t i = 0; i < n; ++i) {
        p.s[2 * i] = src[i].x; p.s[2 * i + 1] = src[i].y;
        p.d[2 * i] = dst[i].x; p.d[2 * i + 1] = dst[i].y;
        if (!aff) continue;
        const cv::Mat& A = (*aff)[i];
        p.a[4 * i] = A.at<double>(0, 0); p.a[4 * i + 1] = A.at<double>(0, 1);
        p.a[4 * i + 2] = A.at<double>(1, 0); p.a[4 * i + 3] = A.at<double>(1, 1);
    }
    return p;
}

} // namespace

cv::Mat multih::detail::MatFrom9(const double* h) { return OwnedMat(3, 3, h); }

bool multih::detail::Check(int rc, const char* what)
{
    if (rc == MH_OK) return true;
    std::cerr << "[Multi-H] engine error in " << what << ": " << mh_last_error() << "\n";
    return false;
}

MultiH::EngineCaps multih::detail::LinkedEngineCaps()
{
    MultiH::EngineCaps c;
    c.point_only = mh_set_estimator && mh_refine_points;
    c.fundamental_minimal = mh_estimate_fundamental_minimal;
    c.set_sampler = mh_set_sampler;
    c.sample_neighbours = mh_build_sample_neighbours;
    c.data_term = mh_set_data_term;
    c.residual_route = mh_set_residual_mode && mh_set_residual_scope;
    c.msac_scores = mh_score_msac && mh_select_best_msac;
    c.get_model = mh_get_model;
    c.refit = mh_refit_homography;
    c.polish = mh_polish_homographies;
    c.reweight = mh_reweight_homographies;
    c.estimator_reweighting = mh_set_estimator_reweighting;
    c.reweight_auto = mh_reweight_homographies_auto;
    c.estimator_reweighting_auto = mh_set_estimator_reweighting_auto;
    c.select_greedy_msac = mh_select_greedy_msac;
    c.propose_haf = mh_propose_haf;
    c.propose_3pt = mh_propose_3pt;
    c.compat_dlt = mh_compat_dlt_medians;
    c.energy_merge = mh_merge_deltas && mh_labeling_energy;
    c.drop_deltas = mh_drop_deltas;
    c.smoothness_weights = mh_set_smoothness_weights;
    return c;
}

MultiH::MultiH(double _thr_fund_mat, double _thr_hom, double _locality, double _lambda,
               int _minimum_inlier_number)
    : minimum_inlier_number(_minimum_inlier_number),
      threshold_fundamental_matrix(_thr_fund_mat),
      threshold_homography(_thr_hom),
      sqr_threshold_homography(_thr_hom * _thr_hom),
      locality_lambda(_locality),
      energy_lambda(_lambda),
      affine_threshold(DEFAULT_AFFINE_THRESHOLD),
      straightness_threshold(DEFAULT_LINENESS_THRESHOLD)
{
    for (double& f : fundamental_matrix) f = 0.0;
    epipole_2[0] = epipole_2[1] = 0.0;
}

MultiH::~MultiH() { Release(); }

// Engines are REUSED from one MultiH object to the next (r04).  The reference's harness makes a new MultiH per image pair
// (M/main.cpp:262); creating and destroying an engine — streams, a few dozen device buffers, their release with the device
// synchronisations that implies — costs 2.5 ms, a third of a whole Process() on a scene of 500 correspondences.  An engine
// carries no result from one call to the next: every Process() sets parameters, transport and correspondences anew, and
// mh_set_correspondences drops everything derived from the previous point set.  Engines that were given tuning knobs, or
// whose stream does not drain cleanly, are destroyed instead.  MULTIH_ENGINE_POOL=0 switches the reuse off.
namespace {
struct EnginePool {
    std::mutex mu;
    std::vector<std::pair<int, mh_engine*>> idle;      // (device, engine), at most two
};
EnginePool& engine_pool()
{
    static EnginePool* p = new EnginePool();           // never destroyed: the HIP runtime may be gone by the time statics are
    return *p;
}
bool engine_pool_enabled()
{
    const char* v = std::getenv("MULTIH_ENGINE_POOL");
    return !(v && v[0] == '0');
}
} // namespace

extern "C" __attribute__((visibility("default")))
void mhh_release_engine_pool()
{
    EnginePool& p = engine_pool();
    std::lock_guard<std::mutex> lock(p.mu);
    for (auto& de : p.idle) mh_destroy(de.second);
    p.idle.clear();
}

void MultiH::Release()
{
    if (!engine) return;
    if (engine_tuning.empty() && engine_pool_enabled() && mh_synchronize(engine) == MH_OK &&
        mh_set_transport(engine, 0, 1, nullptr, nullptr, nullptr) == MH_OK) {
        EnginePool& p = engine_pool();
        std::lock_guard<std::mutex> lock(p.mu);
        if (p.idle.size() < 2) {
            p.idle.emplace_back(device, engine);
            engine = nullptr;
            return;
        }
    }
    mh_destroy(engine);
    engine = nullptr;
}

void MultiH::SetEpipolarGeometry(const double F[9], const double e2[2])
{
    for (int i = 0; i < 9; ++i) fundamental_matrix[i] = F[i];
    epipole_2[0] = e2[0];
    epipole_2[1] = e2[1];
    have_epipolar = true;
}

void MultiH::SetNeighbours(const std::vector<std::vector<int>>& hits) { neighbours = hits; }

void MultiH::SetInitialHomographies(const std::vector<cv::Mat>& Hs)
{
    initial_homographies.clear();
    for (const cv::Mat& h : Hs) initial_homographies.push_back(h.clone());
}

void MultiH::SetProposal(uint64_t seed, int hypotheses, int max_models)
{
    proposal_seed = seed;
    proposal_hypotheses = hypotheses;
    proposal_max_models = max_models;
}

bool MultiH::Process(std::vector<cv::Point2d> _srcPoints, std::vector<cv::Point2d> _dstPoints,
                     std::vector<cv::Mat> _affines)
{
    printf("[Multi-H] Processing has been started.\n");
    src_points_original = _srcPoints;
    dst_points_original = _dstPoints;
    affinities_original = _affines;
    return Process();
}

bool MultiH::Process(std::vector<cv::Point2d> _srcPoints, std::vector<cv::Point2d> _dstPoints)
{
    printf("[Multi-H] Processing has been started.\n");
    src_points_original = _srcPoints;
    dst_points_original = _dstPoints;
    affinities_original.clear();
    return Run(true);
}

bool MultiH::Process()
{
    return Run(false);
}

bool MultiH::EnsureEngine()
{
    if (!engine && engine_tuning.empty() && engine_pool_enabled()) {
        EnginePool& p = engine_pool();
        std::lock_guard<std::mutex> lock(p.mu);
        for (size_t i = 0; i < p.idle.size(); ++i)
            if (p.idle[i].first == device) { engine = p.idle[i].second; p.idle.erase(p.idle.begin() + (long)i); break; }
    }
    if (!engine) {
        if (!Check(mh_create(&engine, device), "mh_create")) return false;
        for (const auto& kv : engine_tuning)
            if (!Check(mh_set_tuning(engine, kv.first, kv.second), "mh_set_tuning")) return false;
    }
    if (!Check(mh_set_transport(engine, shard_rank, std::max(shard_world, 1), shard_stream_allgather, shard_allgather, shard_ctx),
               "mh_set_transport"))
        return false;
    if (!Check(mh_set_fundamental_metric(engine, fundamental_metric), "mh_set_fundamental_metric")) return false;   // (sticky, and engines are reused)
    return Check(mh_set_params(engine, threshold_fundamental_matrix, threshold_homography,
                               locality_lambda, energy_lambda, minimum_inlier_number),
                 "mh_set_params");
}

mh_engine* multih::detail::BorrowEngine(int device)
{
    if (engine_pool_enabled()) {
        EnginePool& p = engine_pool();
        std::lock_guard<std::mutex> lock(p.mu);
        for (size_t i = 0; i < p.idle.size(); ++i)
            if (p.idle[i].first == device) { mh_engine* e = p.idle[i].second; p.idle.erase(p.idle.begin() + (long)i); return e; }
    }
    mh_engine* e = nullptr;
    return Check(mh_create(&e, device), "mh_create") ? e : nullptr;
}
void multih::detail::ReturnEngine(int device, mh_engine* e)
{
    if (!e) return;
    if (engine_pool_enabled() && mh_synchronize(e) == MH_OK) {
        EnginePool& p = engine_pool();
        std::lock_guard<std::mutex> lock(p.mu);
        if (p.idle.size() < 2) { p.idle.emplace_back(device, e); return; }
    }
    mh_destroy(e);
}

bool multih::FilterCorrespondencesByEpipolarGeometry(std::vector<cv::Point2d>& srcPoints, std::vector<cv::Point2d>& dstPoints,
                                                     std::vector<cv::Mat>& affines, double threshold, uint64_t seed,
                                                     int hypotheses, int metric, int device, std::vector<unsigned char>* mask_out,
                                                     const MultiH::FundEstimator& estimator)
{
    const size_t n = srcPoints.size();
    const bool points_only = affines.empty();              // no affinities: filter the points alone
    if (n < 8 || dstPoints.size() != n || (!points_only && affines.size() != n)) return false;
    if (estimator.mode != MultiH::FUND_ESTIMATOR_LS8 && estimator.mode != MultiH::FUND_ESTIMATOR_MINIMAL7) {
        std::cerr << "Error: unknown F estimator " << estimator.mode << " (FUND_ESTIMATOR_LS8 or FUND_ESTIMATOR_MINIMAL7)\n";
        return false;
    }
    const bool minimal = estimator.mode == MultiH::FUND_ESTIMATOR_MINIMAL7;
    if (minimal && !multih::detail::LinkedEngineCaps().fundamental_minimal) {
        std::cerr << "Error: the engine library has no minimal-sample F estimator (mh_estimate_fundamental_minimal)\n";
        return false;
    }
    mh_engine* e = BorrowEngine(device);
    if (!e) return false;
    const PackedPoints p = PackPoints(srcPoints, dstPoints);
    std::vector<unsigned char> mask(n, 0);
    double F[9], e2[2];
    int inl = 0;
    const bool ok = Check(mh_set_fundamental_metric(e, metric), "mh_set_fundamental_metric") &&
                    Check(mh_set_correspondences(e, p.s.data(), p.d.data(), nullptr, (int)n), "mh_set_correspondences") &&
                    (minimal ? Check(mh_estimate_fundamental_minimal(e, seed, estimator.max_samples, estimator.confidence, threshold, F, e2,
                                                                     mask.data(), &inl, nullptr), "mh_estimate_fundamental_minimal")
                             : Check(mh_estimate_fundamental(e, seed, hypotheses, threshold, F, e2, mask.data(), &inl), "mh_estimate_fundamental"));
    ReturnEngine(device, e);
    if (!ok) return false;
    if (mask_out) *mask_out = mask;
    size_t k = 0;
    for (size_t i = 0; i < n; ++i)
        if (mask[i]) {
            if (k != i) { srcPoints[k] = srcPoints[i]; dstPoints[k] = dstPoints[i]; if (!points_only) affines[k] = affines[i]; }
            ++k;
        }
    srcPoints.resize(k); dstPoints.resize(k);
    if (!points_only) affines.resize(k);
    return true;
}

// diagnostic: where Process() spends its time
struct MultiH::StageClock {
    const bool on = std::getenv("MULTIH_TIMING") != nullptr;
    const std::chrono::system_clock::time_point began = std::chrono::system_clock::now();
    void operator()(const char* what) const
    {
        if (on) printf("[Multi-H] %s done %.1f ms after Process() began\n", what,
                       std::chrono::duration<double, std::milli>(std::chrono::system_clock::now() - began).count());
    }
};

bool MultiH::Run(bool points_only)
{
    std::string error;
    caps = multih::detail::LinkedEngineCaps();
    if (!PlanRun(points_only, caps, plan, error)) {
        std::cerr << error;
        return false;
    }
    const StageClock stage;
    if (!EnsureEngine() || !ConfigureEngine(plan)) return false;
    stage("engine");

    // GetFundamentalMatrixAndRefineData (M/MultiH.cpp:52, :770-848; §8(f) row 4): with
    // SetEpipolarGeometry the caller's F / e2 are used and the points are taken as already
    // filtered; otherwise F is estimated on the GPU (FrontHalf).
    src_points = src_points_original;
    dst_points = dst_points_original;
    affinities = affinities_original;
    degenerate_case = false;
    cluster_homographies.clear();
    labeling.clear();
    front_stages = FrontStages();
    front_stages.input = front_stages.in_ransac_mask = front_stages.triangulated = front_stages.affine_consistent =
        static_cast<int>(src_points.size());
    if (!UploadCorrespondences(src_points, dst_points, affinities)) return false;
    stage("correspondences on the device");

    if (!FrontHalf()) return false;
    if (degenerate_case) {
        HandleDegenerateCase();
        return true;
    }
    if (!epipolar_free && !Check(mh_set_epipolar(engine, fundamental_matrix, epipole_2), "mh_set_epipolar")) return false;
    if (!BuildProposalTables(stage) || !InitialModels()) return false;
    stage("initial models");
    ClusterMergingAndLabeling();
    stage("neighbourhood + alternation");
    return PostFilter() && Finish();
}

namespace {
// A refusal of PlanRun: `return Refuse(error) << text << value;` leaves what was streamed in `error` and returns false.
struct Refuse {
    explicit Refuse(std::string& e) : error(e) {}
    ~Refuse() { error = text.str(); }
    template <class T> Refuse& operator<<(const T& v) { text << v; return *this; }
    operator bool() const { return false; }
    std::string& error;
    std::ostringstream text;
};
// The idiom of every optional mode — no entry point: fine while the setting is at its default, an error otherwise.
bool Offers(bool have, bool wanted, const char* message, std::string& error)
{
    return have || !wanted || (Refuse(error) << message);
}
} // namespace

// Every check of Process() that depends on nothing but the settings and on what the engine library offers, in the order the
// checks have always had, and what the run derives from the settings.  Touches no engine and prints nothing: Run() prints
// `error`.  All of these checks precede the creation of the engine and the engine's own setters, so where two settings are
// wrong at once — or no device can be opened — the message can be that of a check which once came behind an engine call;
// with one wrong setting the message and the return value are what they were.  The checks behind the front half
// (FrontHalf: the F estimator; BuildProposalTables: the sampler and the HAF table) stay there, because a degenerate front
// half returns true ahead of them, and what the engine validates (the data term, the fundamental metric) the engine refuses.
bool MultiH::PlanRun(bool points_only, const EngineCaps& have, RunPlan& out, std::string& error) const
{
    out = RunPlan();
    out.points_only = points_only;
    if (src_points_original.size() < 8 || dst_points_original.size() != src_points_original.size() ||
        (!points_only && affinities_original.size() != src_points_original.size()))
        return Refuse(error) << "Error: Features are not set!\n";                       // M/MultiH.cpp:48
    if (points_only && initial_homographies.empty() && init_mode == INIT_STABLE_SETS)
        return Refuse(error) << "Error: the stable point sets (INIT_STABLE_SETS) need affinities; the point-only Process() cannot use them\n";
    if (estimator != ESTIMATOR_HAF && estimator != ESTIMATOR_3PT && estimator != ESTIMATOR_DLT)
        return Refuse(error) << "Error: unknown estimator " << estimator << " (ESTIMATOR_HAF, ESTIMATOR_3PT or ESTIMATOR_DLT)\n";
    if (epipolar_free) {      // what needs F cannot run without one
        if (init_mode == INIT_STABLE_SETS)
            return Refuse(error) << "Error: the stable point sets (INIT_STABLE_SETS) need the fundamental matrix; the epipolar-free route (SetEpipolarFree) cannot use them\n";
        if (proposal_source == PROPOSAL_SOURCE_HAF || proposal_source == PROPOSAL_SOURCE_3PT)
            return Refuse(error) << "Error: " << (proposal_source == PROPOSAL_SOURCE_HAF ? "HAF proposals (PROPOSAL_SOURCE_HAF)" : "3-point proposals (PROPOSAL_SOURCE_3PT)")
                                 << " need the fundamental matrix; the epipolar-free route (SetEpipolarFree) cannot use them\n";
    }
    if (compat_fit != COMPAT_FIT_3PT && compat_fit != COMPAT_FIT_DLT)
        return Refuse(error) << "Error: unknown compatibility fit " << compat_fit << " (COMPAT_FIT_3PT or COMPAT_FIT_DLT)\n";
    if (compat_fit == COMPAT_FIT_DLT && run_compatibility_check) {
        if (!Offers(have.compat_dlt, true, "Error: the engine library has no compatibility check with 4-point trials (mh_compat_dlt_medians)\n", error))
            return false;
        if (compat_trials < 1 || compat_trials > MH_COMPAT_DLT_MAX_TRIALS || !(compat_limit_scale >= 0.0) || std::isinf(compat_limit_scale))
            return Refuse(error) << "Error: SetCompatibilityFit: trials outside [1, " << MH_COMPAT_DLT_MAX_TRIALS << "] or a limit scale that is negative or not finite\n";
    }
    // where the batches come from (looked at only where a batch is proposed)
    if (initial_homographies.empty() && init_mode != INIT_STABLE_SETS) {
        if (proposal_source == PROPOSAL_SOURCE_3PT) {      // points and F are all it needs: the point-only Process() may use it
            if (!Offers(have.propose_3pt, true, "Error: the engine library has no 3-point proposals (mh_propose_3pt)\n", error)) return false;
            out.initial_source = out.iterative_source = PROPOSAL_SOURCE_3PT;
        } else if (proposal_source != PROPOSAL_SOURCE_DLT && proposal_source != PROPOSAL_SOURCE_HAF) {
            return Refuse(error) << "Error: unknown proposal source " << proposal_source << " (PROPOSAL_SOURCE_DLT or PROPOSAL_SOURCE_HAF)\n";
        }
        if (proposal_source == PROPOSAL_SOURCE_HAF) {
            if (points_only)
                return Refuse(error) << "Error: HAF proposals (PROPOSAL_SOURCE_HAF) need affinities; the point-only Process() cannot use them\n";
            if (!Offers(have.propose_haf, true, "Error: the engine library has no HAF proposals (mh_propose_haf)\n", error)) return false;
            if (proposal_haf_stride < 1 || proposal_haf_members < 0 || proposal_haf_members == 1 || proposal_haf_members == 2 ||
                proposal_haf_members > 32)
                return Refuse(error) << "Error: SetProposalSource: members = " << proposal_haf_members << ", stride = " << proposal_haf_stride
                                     << " (members 0 or in [3, 32], stride >= 1)\n";
            if (proposal_sampler == PROPOSAL_LOCAL && proposal_haf_members > proposal_sampler_k)
                return Refuse(error) << "Error: SetProposalSource: members = " << proposal_haf_members << " exceeds k = " << proposal_sampler_k
                                     << " of the local sampler, whose table the HAF proposals share\n";
            out.initial_source = PROPOSAL_SOURCE_HAF;      // (the iterative batches stay DLT)
        }
    }
    // the re-estimator of the loop and of the proposal refit
    // (the epipolar-free route: the N-point DLT, which reads no F; the point-only route: the 3-point fit unless the DLT is asked for)
    out.est = epipolar_free || estimator == ESTIMATOR_DLT ? MH_ESTIMATOR_DLT : points_only ? MH_ESTIMATOR_3PT : estimator;
    if (!Offers(have.point_only, out.est != MH_ESTIMATOR_HAF,
                "Error: the engine library has no point-only entry points (mh_set_estimator, mh_refine_points)\n", error))
        return false;
    if (merge_mode != MERGE_MEAN_SHIFT && merge_mode != MERGE_ENERGY) return Refuse(error) << "Error: unknown merge mode (SetMergeMode)\n";
    if (!Offers(have.energy_merge, merge_mode == MERGE_ENERGY,
                "Error: the engine library has no energy-tested merge (mh_merge_deltas, mh_labeling_energy)\n", error))
        return false;
    if (!(label_cost_points >= 0.0) || !std::isfinite(label_cost_points))
        return Refuse(error) << "Error: the label cost must be finite and not negative (SetLabelCost)\n";
    if (label_cost_points > 0.0 && merge_mode != MERGE_ENERGY)
        return Refuse(error) << "Error: a label cost needs the energy-tested merge (SetLabelCost with SetMergeMode(MERGE_ENERGY))\n";
    if (!Offers(have.drop_deltas, label_cost_points > 0.0, "Error: the engine library has no label-drop evaluation (mh_drop_deltas)\n", error))
        return false;
    // beta in energy units: `points` outliers' worth, round(lam * T) each (mh_data_cost's outlier cost)
    const double outlier = std::round((100.0 / energy_lambda) * (threshold_homography * threshold_homography * 81.0 / 16.0));
    const double beta = label_cost_points * outlier;
    if (!(beta < 9.0e18)) return Refuse(error) << "Error: the label cost is too large (SetLabelCost)\n";
    out.label_cost_beta = std::llround(beta);
    // the data term of the labeling (an unknown value is the engine's to refuse)
    if (!Offers(have.data_term, data_term != DATA_TERM_REFERENCE, "Error: the engine library has no selectable data term (mh_set_data_term)\n", error))
        return false;
    // the weights of the smoothness term
    if (smoothness_rule != SMOOTHNESS_UNIFORM && smoothness_rule != SMOOTHNESS_CAUCHY)
        return Refuse(error) << "Error: unknown smoothness rule " << smoothness_rule << " (SMOOTHNESS_UNIFORM or SMOOTHNESS_CAUCHY)\n";
    if (smoothness_rule == SMOOTHNESS_CAUCHY) {
        if (!std::isfinite(smoothness_rho) || !(smoothness_rho > 0.0) || smoothness_q_max < 1 || smoothness_q_max > MH_SMOOTH_Q_MAX)
            return Refuse(error) << "Error: SetSmoothnessWeights: rho = " << smoothness_rho << ", q_max = " << smoothness_q_max
                                 << " (rho finite and > 0, q_max in [1, " << MH_SMOOTH_Q_MAX << "])\n";
        if (!Offers(have.smoothness_weights, true, "Error: the engine library has no distance-weighted smoothness (mh_set_smoothness_weights)\n", error))
            return false;
        out.smoothness_rule = MH_SMOOTH_CAUCHY; out.smoothness_rho = smoothness_rho; out.smoothness_q_max = smoothness_q_max;
    }
    // the error of the whole route
    if (residual != RESIDUAL_FORWARD && residual != RESIDUAL_SYMMETRIC)
        return Refuse(error) << "Error: unknown residual " << residual << " (RESIDUAL_FORWARD or RESIDUAL_SYMMETRIC)\n";
    if (residual == RESIDUAL_SYMMETRIC && (tail_score == TAIL_SCORE_MSAC || (init_mode != INIT_STABLE_SETS && selection_score == SELECTION_SCORE_MSAC)))
        return Refuse(error) << "Error: the MSAC weights (TAIL_SCORE_MSAC, SELECTION_SCORE_MSAC) measure the forward error only; they do not combine with RESIDUAL_SYMMETRIC\n";
    if (!Offers(have.residual_route, residual != RESIDUAL_FORWARD,
                "Error: the engine library has no symmetric route (mh_set_residual_mode, mh_set_residual_scope)\n", error))
        return false;
    out.residual_mode = residual == RESIDUAL_SYMMETRIC ? MH_RESIDUAL_SYMMETRIC : MH_RESIDUAL_FORWARD;
    out.residual_scope = residual == RESIDUAL_SYMMETRIC ? MH_RESIDUAL_SCOPE_ROUTE : MH_RESIDUAL_SCOPE_SCORE;
    return PlanFinishModes(have, out, error);
}

// ... continued: the degenerate tail, the refits of the results and of the loop's estimator, the selection.
bool MultiH::PlanFinishModes(const EngineCaps& have, RunPlan& out, std::string& error) const
{
    // how the degenerate tail ranks its hypotheses
    if (tail_score != TAIL_SCORE_COUNT && tail_score != TAIL_SCORE_MSAC)
        return Refuse(error) << "Error: unknown tail score " << tail_score << " (TAIL_SCORE_COUNT or TAIL_SCORE_MSAC)\n";
    if (!Offers(have.msac_scores && have.get_model, tail_score == TAIL_SCORE_MSAC,
                "Error: the engine library has no MSAC scores (mh_score_msac, mh_select_best_msac, mh_get_model)\n", error))
        return false;
    // whether the degenerate tail refits its winner
    if (tail_refit < 0 || tail_refit > 16) return Refuse(error) << "Error: tail refit iterations " << tail_refit << " outside [0, 16]\n";
    if (!Offers(have.refit && have.get_model, tail_refit > 0,
                "Error: the engine library has no homography refit (mh_refit_homography, mh_get_model)\n", error))
        return false;
    // whether the tail's result and the final models are polished
    if (tail_polish < 0 || tail_polish > 32) return Refuse(error) << "Error: tail polish iterations " << tail_polish << " outside [0, 32]\n";
    if (model_polish < 0 || model_polish > 32) return Refuse(error) << "Error: model polish iterations " << model_polish << " outside [0, 32]\n";
    if (!Offers(have.polish, tail_polish > 0 || model_polish > 0, "Error: the engine library has no homography polish (mh_polish_homographies)\n", error))
        return false;
    if (!Offers(have.get_model, tail_polish > 0, "Error: the engine library has no single-model read-back for the tail's polish (mh_get_model)\n", error))
        return false;
    // whether the final models and the loop's DLT re-estimator run reweighted rounds
    if (model_reweight < 0 || model_reweight > 16 || estimator_reweight < 0 || estimator_reweight > 16)
        return Refuse(error) << "Error: reweighting rounds " << model_reweight << " (final) / " << estimator_reweight << " (estimator) outside [0, 16]\n";
    if (!(model_reweight_scale >= 0.0) || !(estimator_reweight_scale >= 0.0) || std::isinf(model_reweight_scale) ||
        std::isinf(estimator_reweight_scale))
        return Refuse(error) << "Error: reweighting scale " << model_reweight_scale << " (final) / " << estimator_reweight_scale
                             << " (estimator) is not a finite number >= 0\n";
    if (!Offers(have.reweight, model_reweight > 0, "Error: the engine library has no reweighted refit (mh_reweight_homographies)\n", error))
        return false;
    const bool dlt = out.est == MH_ESTIMATOR_DLT;      // the estimator's rounds are off unless the DLT estimator runs
    if (!Offers(have.estimator_reweighting, dlt && estimator_reweight > 0,
                "Error: the engine library has no reweighted estimator (mh_set_estimator_reweighting)\n", error))
        return false;
    // ... or reweighted rounds whose scale follows each label's own residuals (SetModelReweightAuto, SetEstimatorReweightAuto)
    if (model_reweight_auto < 0 || model_reweight_auto > 16 || estimator_reweight_auto < 0 || estimator_reweight_auto > 16)
        return Refuse(error) << "Error: self-scaled reweighting rounds " << model_reweight_auto << " (final) / " << estimator_reweight_auto
                             << " (estimator) outside [0, 16]\n";
    if (!(model_reweight_kappa >= 0.0) || !(estimator_reweight_kappa >= 0.0) || model_reweight_kappa > 1e150 ||
        estimator_reweight_kappa > 1e150)
        return Refuse(error) << "Error: self-scaled reweighting kappa " << model_reweight_kappa << " (final) / " << estimator_reweight_kappa
                             << " (estimator) is not a finite number >= 0\n";
    if ((model_reweight > 0 && model_reweight_auto > 0) || (estimator_reweight > 0 && estimator_reweight_auto > 0))
        return Refuse(error) << "Error: both the fixed and the self-scaled reweighting are set for the "
                             << (model_reweight > 0 && model_reweight_auto > 0 ? "final refit" : "estimator") << "; choose one\n";
    if (!Offers(have.reweight_auto, model_reweight_auto > 0,
                "Error: the engine library has no self-scaled reweighted refit (mh_reweight_homographies_auto)\n", error))
        return false;
    if (!Offers(have.estimator_reweighting_auto, dlt && estimator_reweight_auto > 0,
                "Error: the engine library has no self-scaled reweighted estimator (mh_set_estimator_reweighting_auto)\n", error))
        return false;
    const double px = estimator_reweight_scale > 0.0 ? estimator_reweight_scale : threshold_homography;
    out.estimator_reweight_auto = dlt && estimator_reweight_auto > 0;
    out.estimator_reweight_rounds = !dlt ? 0 : out.estimator_reweight_auto ? estimator_reweight_auto : estimator_reweight;
    out.estimator_reweight_c2 = px * px;
    // how ProposeModels ranks a batch (INIT_STABLE_SETS proposes nothing: the mode is not looked at)
    if (init_mode == INIT_STABLE_SETS) return true;
    if (selection_score != SELECTION_SCORE_COUNT && selection_score != SELECTION_SCORE_MSAC)
        return Refuse(error) << "Error: unknown selection score " << selection_score << " (SELECTION_SCORE_COUNT or SELECTION_SCORE_MSAC)\n";
    return Offers(have.select_greedy_msac, selection_score == SELECTION_SCORE_MSAC,
                  "Error: the engine library has no selection ranked by MSAC weight (mh_select_greedy_msac)\n", error);
}

// The engine's sticky settings, every one on every call because engines are reused.  A setter the library lacks is skipped:
// PlanRun has made sure that the setting is then at its default.
bool MultiH::ConfigureEngine(const RunPlan& p)
{
    if (caps.point_only && !Check(mh_set_estimator(engine, p.est), "mh_set_estimator")) return false;
    if (caps.data_term && !Check(mh_set_data_term(engine, data_term), "mh_set_data_term")) return false;
    if (caps.smoothness_weights &&
        !Check(mh_set_smoothness_weights(engine, p.smoothness_rule, p.smoothness_rho, p.smoothness_q_max), "mh_set_smoothness_weights"))
        return false;
    if (caps.residual_route && (!Check(mh_set_residual_mode(engine, p.residual_mode), "mh_set_residual_mode") ||
                                !Check(mh_set_residual_scope(engine, p.residual_scope), "mh_set_residual_scope")))
        return false;
    if (caps.estimator_reweighting &&
        !Check(mh_set_estimator_reweighting(engine, p.estimator_reweight_auto ? 0 : p.estimator_reweight_rounds, p.estimator_reweight_c2),
               "mh_set_estimator_reweighting"))
        return false;
    // set behind the fixed setting, and only with rounds: of the engine's two setters the last call decides
    return !p.estimator_reweight_auto ||
           Check(mh_set_estimator_reweighting_auto(engine, p.estimator_reweight_rounds, 1, 2, AutoKappa2(estimator_reweight_kappa), DBL_MIN,
                                                   AutoScaleMax()),
                 "mh_set_estimator_reweighting_auto");
}

bool MultiH::UploadCorrespondences(const std::vector<cv::Point2d>& src, const std::vector<cv::Point2d>& dst, const std::vector<cv::Mat>& aff)
{
    const PackedPoints p = PackPoints(src, dst, plan.points_only ? nullptr : &aff);
    return Check(mh_set_correspondences(engine, p.s.data(), p.d.data(), p.affinities(), static_cast<int>(src.size())), "mh_set_correspondences");
}

// GetFundamentalMatrixAndRefineData (M/MultiH.cpp:770-848) on the GPU: RANSAC over normalised 8-point hypotheses with
// Sampson scoring, LS refit, epipoles from F^T F / F F^T, then the per-correspondence refinement of :807-838 (RefineData).
// Nothing to do with the caller's F or on the route without one.  Leaves degenerate_case set where no F can be had.
bool MultiH::FrontHalf()
{
    if (epipolar_free) {
        // no F is estimated, no correspondence refined or dropped: the stage table keeps the input count four times
        if (have_epipolar) printf("[Multi-H] Epipolar-free route: the epipolar geometry given by SetEpipolarGeometry is ignored.\n");
        return true;
    }
    if (have_epipolar) return true;
    std::vector<unsigned char> mask(src_points.size(), 0);
    int inl = 0;
    if (fundamental_estimator.mode != FUND_ESTIMATOR_LS8 && fundamental_estimator.mode != FUND_ESTIMATOR_MINIMAL7) {
        std::cerr << "Error: unknown F estimator " << fundamental_estimator.mode << " (FUND_ESTIMATOR_LS8 or FUND_ESTIMATOR_MINIMAL7)\n";
        return false;
    }
    const bool minimal = fundamental_estimator.mode == FUND_ESTIMATOR_MINIMAL7;
    if (minimal && !caps.fundamental_minimal) {
        std::cerr << "Error: the engine library has no minimal-sample F estimator (mh_estimate_fundamental_minimal)\n";
        return false;
    }
    const bool ok = minimal ? Check(mh_estimate_fundamental_minimal(engine, proposal_seed ^ 0xf00dull, fundamental_estimator.max_samples,
                                                                    fundamental_estimator.confidence, threshold_fundamental_matrix,
                                                                    fundamental_matrix, epipole_2, mask.data(), &inl, nullptr),
                                    "mh_estimate_fundamental_minimal")
                            : Check(mh_estimate_fundamental(engine, proposal_seed ^ 0xf00dull, fundamental_hypotheses,
                                                            threshold_fundamental_matrix, fundamental_matrix, epipole_2,
                                                            mask.data(), &inl),
                                    "mh_estimate_fundamental");
    double nrm = 0.0;
    for (double f : fundamental_matrix) nrm += f * f;
    degenerate_case = !ok || !(std::sqrt(nrm) >= 1e-5) || !std::isfinite(epipole_2[0]) ||
                      !std::isfinite(epipole_2[1]);                             // :779
    if (degenerate_case) {
        printf("[Multi-H] Degenerate case, the fundamental matrix cannot be estimated.\n");
        return true;
    }
    return RefineData(mask);
}

// :807-838 on the GPU: Hartley-Sturm correction, affine consistency filter, optimal affinity (the point-only route: the
// correction alone, mh_refine_points); what is kept replaces the correspondences here and on the engine.
bool MultiH::RefineData(const std::vector<unsigned char>& mask)
{
    const int N = static_cast<int>(src_points.size());
    const bool points_only = plan.points_only;
    double e1[2];
    std::vector<unsigned char> keep(N, 0);
    const int stride = points_only ? 4 : 8;
    std::vector<double> refined(stride * (size_t)N);
    if (!Check(mh_epipoles(engine, fundamental_matrix, e1, epipole_2), "mh_epipoles"))
        return false;
    if (points_only ? !Check(mh_refine_points(engine, fundamental_matrix, e1, epipole_2, mask.data(), keep.data(), refined.data()),
                             "mh_refine_points")
                    : !Check(mh_refine_correspondences(engine, fundamental_matrix, e1, epipole_2, mask.data(), keep.data(),
                                                       refined.data()),
                             "mh_refine_correspondences"))
        return false;
    std::vector<unsigned char> reason(N, 0);
    if (!Check(mh_get_refine_reasons(engine, reason.data(), N), "mh_get_refine_reasons")) return false;
    front_stages.in_ransac_mask = front_stages.triangulated = front_stages.affine_consistent = 0;
    for (int i = 0; i < N; ++i) {
        if (reason[i] != MH_REFINE_NOT_IN_MASK) ++front_stages.in_ransac_mask;
        if (reason[i] == MH_REFINE_KEPT || reason[i] == MH_REFINE_AFFINE_TEST) ++front_stages.triangulated;
        if (reason[i] == MH_REFINE_KEPT) ++front_stages.affine_consistent;
    }
    std::vector<cv::Point2d> s2, d2;
    std::vector<cv::Mat> a2;
    for (int i = 0; i < N; ++i)
        if (keep[i]) {
            const double* r = &refined[stride * (size_t)i];
            s2.push_back(cv::Point2d(r[0], r[1]));
            d2.push_back(cv::Point2d(r[2], r[3]));
            if (!points_only) a2.push_back(OwnedMat(2, 2, r + 4));
        }
    printf("[Multi-H] %d points kept from the initial %d after filtering.\n", (int)s2.size(), N);   // :840
    if (log_to_console)
        printf("[Multi-H]   stages: %d in the RANSAC mask at %.2f px, %d after OptimalTriangulation, %d after distanceError <= 1\n",
               front_stages.in_ransac_mask, threshold_fundamental_matrix, front_stages.triangulated, front_stages.affine_consistent);
    if (s2.size() < 8) {
        degenerate_case = true;
        printf("[Multi-H] Degenerate case, not enough points remained.\n");                         // :845
        return true;
    }
    src_points.swap(s2); dst_points.swap(d2); affinities.swap(a2);
    return UploadCorrespondences(src_points, dst_points, affinities);
}

// The proposal sampler: its three arguments are checked here, once; then the local sampler's table, once, on the
// correspondences the proposer samples (the refined ones); then the HAF proposals' neighbour table.
bool MultiH::BuildProposalTables(const StageClock& stage)
{
    const bool haf = plan.initial_source == PROPOSAL_SOURCE_HAF;
    if (proposal_sampler != PROPOSAL_UNIFORM && proposal_sampler != PROPOSAL_LOCAL) {
        std::cerr << "Error: unknown proposal sampler " << proposal_sampler << " (PROPOSAL_UNIFORM or PROPOSAL_LOCAL)\n";
        return false;
    }
    plan.proposal_local = proposal_sampler == PROPOSAL_LOCAL && init_mode != INIT_STABLE_SETS;
    if (plan.proposal_local) {
        if (proposal_sampler_k < 3 || proposal_sampler_k > 32) {
            std::cerr << "Error: SetProposalSampler: k = " << proposal_sampler_k << " is outside [3, 32]\n";
            return false;
        }
        if (proposal_uniform_per_16 < 0 || proposal_uniform_per_16 > 16) {
            std::cerr << "Error: SetProposalSampler: uniform_per_16 = " << proposal_uniform_per_16 << " is outside [0, 16]\n";
            return false;
        }
        if (!caps.set_sampler || !caps.sample_neighbours) {
            std::cerr << "Error: the engine library has no local proposal sampler (mh_set_sampler, mh_build_sample_neighbours)\n";
            return false;
        }
        const int points = static_cast<int>(src_points.size());          // (at least 8 here, so k stays >= 3)
        int k = proposal_sampler_k;
        if (k > points - 1) {
            k = points - 1;
            printf("[Multi-H] Proposal sampler: k reduced from %d to %d (%d correspondences)\n", proposal_sampler_k, k, points);
        }
        if (!Check(mh_build_sample_neighbours(engine, k), "mh_build_sample_neighbours")) return false;
        stage("sampling table");
        if (haf && proposal_haf_members > k) {
            std::cerr << "Error: SetProposalSource: members = " << proposal_haf_members << " exceeds k = " << k << " of the local sampler's table\n";
            return false;
        }
    }
    // The HAF proposals' neighbour table: the sampler's when there is one, else built here, once, with k = members.
    plan.haf_members = haf ? proposal_haf_members : 0;
    if (haf && plan.haf_members > 0 && !plan.proposal_local) {
        if (!caps.sample_neighbours) {
            std::cerr << "Error: the engine library has no neighbour table for the HAF proposals (mh_build_sample_neighbours)\n";
            return false;
        }
        const int points = static_cast<int>(src_points.size());          // (at least 8 here, so members stays >= 3)
        if (plan.haf_members > points - 1) {
            plan.haf_members = points - 1;
            // (said whatever the verbosity, like the sampler's "k reduced": the caller's setting is not what runs)
            printf("[Multi-H] HAF proposals: members reduced from %d to %d (%d correspondences)\n", proposal_haf_members, plan.haf_members, points);
        }
        if (!Check(mh_build_sample_neighbours(engine, plan.haf_members), "mh_build_sample_neighbours")) return false;
        stage("HAF neighbour table");
    }
    return true;
}

bool MultiH::InitialModels()
{
    if (!initial_homographies.empty()) {
        for (const cv::Mat& h : initial_homographies) cluster_homographies.push_back(h.clone());
        return true;
    }
    if (init_mode != INIT_STABLE_SETS) return ProposeInitialModels();
    auto t0 = std::chrono::system_clock::now();
    if (!EstablishStablePointSets()) return false;
    std::chrono::duration<double> el = std::chrono::system_clock::now() - t0;
    printf("[Multi-H] Stable cluster estimation time = %f secs\n", el.count());          // :74
    return true;
}

bool MultiH::PostFilter()
{
    if (cluster_homographies.size() <= 1 || !run_compatibility_check) return true;
    const int before = static_cast<int>(cluster_homographies.size());
    auto t0 = std::chrono::system_clock::now();
    post_filter_failed = false;
    if (compat_fit == COMPAT_FIT_DLT) {
        HomographyCompatibilityCheckDlt();
        if (post_filter_failed) return false;                                // the engine refused: no host fallback
        std::chrono::duration<double> el = std::chrono::system_clock::now() - t0;
        printf("[Multi-H] Compatibility check (4-point trials) time = %f secs (%d clusters removed from %d)\n", el.count(),
               before - (int)cluster_homographies.size(), before);
    } else if (epipolar_free) {
        printf("[Multi-H] Epipolar-free route: the compatibility check is skipped (its trials are 3-point fits with F).\n");
    } else {                                                                 // :78-86
        HomographyCompatibilityCheck();
        if (post_filter_failed) return false;                                // the engine refused: no host fallback
        std::chrono::duration<double> el = std::chrono::system_clock::now() - t0;
        printf("[Multi-H] Compatibility check time = %f secs (%d clusters removed from %d)\n", el.count(),
               before - (int)cluster_homographies.size(), before);
    }
    return true;
}

// The one-cluster exit (:88-94), or every cluster's homography refitted (reweighted rounds, then the polish) over its
// labelled (refined) correspondences: the engine still holds them.
bool MultiH::Finish()
{
    if (cluster_homographies.size() <= 1) {
        labeling.clear();
        labeling.resize(src_points.size(), -1);
        cluster_homographies.resize(0);
        HandleDegenerateCase();
        return true;
    }
    if (model_reweight <= 0 && model_reweight_auto <= 0 && model_polish <= 0) return true;
    const int nh = static_cast<int>(cluster_homographies.size());
    if (labeling.size() != src_points.size()) {
        std::cerr << "Error: model refit: " << labeling.size() << " labels for " << src_points.size() << " correspondences\n";
        return false;
    }
    std::vector<double> H = FlatModels();
    if (model_reweight > 0) {
        const double px = model_reweight_scale > 0.0 ? model_reweight_scale : threshold_homography;
        if (!Check(mh_reweight_homographies(engine, labeling.data(), H.data(), nh, px * px, model_reweight, H.data(), nullptr, nullptr),
                   "mh_reweight_homographies"))
            return false;
    }
    if (model_reweight_auto > 0 &&
        !Check(mh_reweight_homographies_auto(engine, labeling.data(), H.data(), nh, 1, 2, AutoKappa2(model_reweight_kappa), DBL_MIN,
                                             AutoScaleMax(), model_reweight_auto, H.data(), nullptr, nullptr, nullptr),
               "mh_reweight_homographies_auto"))
        return false;
    if (model_polish > 0 &&
        !Check(mh_polish_homographies(engine, labeling.data(), H.data(), nh, model_polish, H.data(), nullptr, nullptr),
               "mh_polish_homographies"))
        return false;
    for (int i = 0; i < nh; ++i) cluster_homographies[i] = MatFrom9(&H[9 * (size_t)i]);
    return true;
}

// The tail's model polished over its inliers (labeling: 0 = inlier) on the original points, which the engine holds here
bool MultiH::PolishTailModel(double H[9])
{
    if (tail_polish <= 0) return true;
    return Check(mh_polish_homographies(engine, labeling.data(), H, 1, tail_polish, H, nullptr, nullptr), "mh_polish_homographies");
}

void MultiH::HomographyCompatibilityCheck()
{
    const int N = static_cast<int>(src_points.size());
    const int nh = static_cast<int>(cluster_homographies.size());
    if (nh == 0 || (int)labeling.size() != N) return;
    const PackedPoints xy = PackPoints(src_points, dst_points);
    std::vector<double> H = FlatModels();
    // the trials' 3-point fits (r06) and their order statistics come from the engine (csrc/compat.hip); the replay of the draws
    // and the reference's stale-buffer bookkeeping are host work (merge_step.cpp)
    multih::CompatStatsFn on_engine;
    if (engine)
        on_engine = [this](const double* pts, const int* begin, int clusters, const int* tri, const double* Ht,
                           const unsigned char* ok, int trials, double* out) {
            if (!Ht) return Check(mh_compat_trial_stats_fit(engine, pts, begin, clusters, tri, fundamental_matrix, trials, out, nullptr, nullptr),
                                  "mh_compat_trial_stats_fit");
            return Check(mh_compat_trial_stats(engine, pts, begin, clusters, tri, Ht, ok, trials, out), "mh_compat_trial_stats");
        };
    bool failed = false;
    const int kept = multih::CompatibilityCheck(xy.s.data(), xy.d.data(), N, labeling.data(), H.data(), nh,
                                                fundamental_matrix, sqr_threshold_homography,
                                                minimum_inlier_number, proposal_seed ^ 0xc0117a7ull, nullptr,
                                                engine ? &on_engine : nullptr, &failed, engine != nullptr);
    if (failed) { post_filter_failed = true; return; }
    cluster_homographies.clear();
    for (int i = 0; i < kept; ++i) cluster_homographies.push_back(MatFrom9(&H[9 * (size_t)i]));
}

void MultiH::HomographyCompatibilityCheckDlt()
{
    const int N = static_cast<int>(src_points.size());
    const int nh = static_cast<int>(cluster_homographies.size());
    if (nh == 0 || (int)labeling.size() != N) return;
    const PackedPoints xy = PackPoints(src_points, dst_points);
    std::vector<double> H = FlatModels();
    const multih::CompatDltFn on_engine = [this](const double* pts, const int* begin, int clusters, uint64_t seed, int trials,
                                                 double* medians) {
        return Check(mh_compat_dlt_medians(engine, pts, begin, clusters, seed, 0, trials, medians, nullptr, nullptr, nullptr),
                     "mh_compat_dlt_medians");
    };
    const double scale = compat_limit_scale > 0.0 ? compat_limit_scale : COMPAT_DLT_LIMIT_SCALE;
    bool failed = false;
    const int kept = multih::CompatibilityCheckDlt(xy.s.data(), xy.d.data(), N, labeling.data(), H.data(), nh,
                                                   scale * sqr_threshold_homography, minimum_inlier_number,
                                                   proposal_seed ^ 0xc0117a7ull, compat_trials, nullptr, &on_engine, &failed);
    if (failed) { post_filter_failed = true; return; }
    cluster_homographies.clear();
    for (int i = 0; i < kept; ++i) cluster_homographies.push_back(MatFrom9(&H[9 * (size_t)i]));
}

// DrawClusters, M/MultiH.cpp:314-350: one filled circle per labelled correspondence in each image, colour by plane.
// The reference's fixed palette (:322-332) for the first eleven planes; it writes all eleven entries whatever the
// number of planes (out of bounds below eleven planes), which is not reproduced: the palette is sized first.
void MultiH::DrawClusters(cv::Mat& img1, cv::Mat& img2, int size)
{
    static const double fixed[11][3] = { { 255, 0, 0 }, { 255, 255, 255 }, { 0, 0, 255 }, { 255, 255, 0 }, { 255, 0, 255 },
                                         { 0, 255, 255 }, { 0, 255, 0 }, { 127, 255, 0 }, { 0, 255, 127 }, { 127, 127, 0 },
                                         { 63, 255, 127 } };
    const size_t k = cluster_homographies.size();
    std::vector<cv::Scalar> colors(std::max<size_t>(k + 1, 12));
    colors[0] = cv::Scalar(0, 0, 0);
    uint64_t z = proposal_seed ^ 0xc0105ull;                              // planes beyond the palette: counter RNG, not rand()
    for (size_t i = 1; i < colors.size(); ++i) {
        if (i <= 11) { colors[i] = cv::Scalar(fixed[i - 1][0], fixed[i - 1][1], fixed[i - 1][2]); continue; }
        double c[3];
        for (double& v : c) {
            z += 0x9E3779B97F4A7C15ull;
            uint64_t x = z;
            x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
            x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
            v = 255.0 * (double)((x ^ (x >> 31)) >> 11) * (1.0 / 9007199254740992.0);
        }
        colors[i] = cv::Scalar(c[0], c[1], c[2]);
    }
    for (size_t i = 0; i < labeling.size(); ++i) {
        if (labeling[i] == -1) continue;                                                  // :336
        const cv::Scalar& col = colors[(size_t)labeling[i] + 1];
        if (k == 1 && i < src_points_original.size()) {                                   // degenerate path labels the ORIGINAL points, :339-343
            cv::circle(img1, src_points_original[i], size, col, -1);
            cv::circle(img2, dst_points_original[i], size, col, -1);
        } else if (i < src_points.size()) {
            cv::circle(img1, src_points[i], size, col, -1);
            cv::circle(img2, dst_points[i], size, col, -1);
        }
    }
}

std::vector<double> MultiH::FlatModels() const
{
    std::vector<double> H(9 * cluster_homographies.size());
    for (size_t i = 0; i < cluster_homographies.size(); ++i) {
        const double* p = reinterpret_cast<const double*>(cluster_homographies[i].data);
        for (int k = 0; k < 9; ++k) H[9 * i + k] = p[k];
    }
    return H;
}

bool MultiH::UploadModels()
{
    const std::vector<double> H = FlatModels();
    return Check(mh_set_models(engine, H.data(), static_cast<int>(cluster_homographies.size())), "mh_set_models");
}

bool MultiH::DownloadModels(int count)
{
    std::vector<double> H(9 * (size_t)count);
    if (!Check(mh_get_models(engine, H.data()), "mh_get_models")) return false;
    cluster_homographies.clear();
    for (int i = 0; i < count; ++i) cluster_homographies.push_back(MatFrom9(&H[9 * (size_t)i]));
    return true;
}

// EstablishStablePointSets (M/MultiH.cpp:604-694) preceded by ComputeLocalHomographies (:696-717):
// point-wise HAF homographies and their 10-D features on the GPU (mh_local_homographies), mean
// shift with bandwidth thr_H whose climbs run on the GPU (mh_mean_shift), then per cluster of at
// least three points one least-squares 3-point homography with LM refinement (host, :664-688).
bool MultiH::EstablishStablePointSets()
{
    const int N = static_cast<int>(src_points.size());
    const bool timing = std::getenv("MULTIH_TIMING") != nullptr;          // diagnostic: where the initialisation's time goes
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    std::vector<double> feat(10 * (size_t)N);
    if (!Check(mh_local_homographies(engine, locality_lambda, nullptr, feat.data()), "mh_local_homographies"))
        return false;
    const double ms_local = ms_since(t0);
    // a degenerate per-point solve (NaN features) would poison the L1 ball test; park such rows far away
    for (double& f : feat) if (!std::isfinite(f)) f = 1e300;
    std::vector<int> assign(N);
    int k = 0;
    if (!Check(mh_mean_shift(engine, feat.data(), N, 10, threshold_homography, proposal_seed ^ 0x57ab1eull,
                             nullptr, 0, assign.data(), &k),
               "mh_mean_shift"))
        return false;
    const double ms_shift = ms_since(t0) - ms_local;
    std::vector<std::vector<int>> members(k);
    for (int i = 0; i < N; ++i) if (assign[i] >= 0) members[assign[i]].push_back(i);
    {
        // one 3-point fit with LM per cluster of at least three points (:664-688), on the host's cores (r06), taken in cluster order
        const PackedPoints xy = PackPoints(src_points, dst_points);
        std::vector<double> Hc;
        std::vector<unsigned char> okc;
        multih::Homography3PTClusters(xy.s.data(), xy.d.data(), members, fundamental_matrix, Hc, okc);
        for (int c = 0; c < k; ++c)
            if (okc[c]) cluster_homographies.push_back(MatFrom9(&Hc[9 * (size_t)c]));
    }
    if (timing)
        printf("[Multi-H] stable sets: per-point homographies %.2f ms, mean shift %.2f ms (%d modes), 3-point fits %.2f ms\n",
               ms_local, ms_shift, k, ms_since(t0) - ms_local - ms_shift);
    if (log_to_console)
        printf("[Multi-H] Number of stable, local clusters = %d\n", (int)cluster_homographies.size());   // :693
    return true;
}

// north_star "propose": a batch of minimal-sample DLT hypotheses scored against all points,
// then greedy selection — take the best-supported hypothesis, remove its inliers from the
// support mask, re-score, repeat (the sequential-RANSAC scheme of the dead
// M/MultipleHomographies.h:146-175, where points already claimed are skipped via usabilityMask).
bool MultiH::ProposeInitialModels()
{
    std::vector<unsigned char> mask(src_points.size(), 1);
    if (plan.initial_source == PROPOSAL_SOURCE_HAF) {
        // one hypothesis per stride-th refined correspondence: counters 0 .. M - 1, anchors c * stride
        const int M = (static_cast<int>(src_points.size()) + proposal_haf_stride - 1) / proposal_haf_stride;
        if (log_to_console || std::getenv("MULTIH_TIMING") != nullptr)      // (part of the stage log too)
            printf("[Multi-H] HAF proposals: %d hypotheses (members %d, stride %d); SetProposal's count of %d is ignored\n", M, plan.haf_members,
                   proposal_haf_stride, proposal_hypotheses);
        const bool ok = ProposeModels(PROPOSAL_SOURCE_HAF, proposal_seed, 0, M, proposal_max_models, mask);
        if (ok && log_to_console)
            printf("[Multi-H] Proposed %d models from %d HAF hypotheses\n", (int)cluster_homographies.size(), M);
        return ok;
    }
    const bool ok = ProposeModels(plan.initial_source, proposal_seed, 0, proposal_hypotheses, proposal_max_models, mask);
    if (ok && plan.initial_source == PROPOSAL_SOURCE_3PT && (log_to_console || std::getenv("MULTIH_TIMING") != nullptr))      // (part of the stage log too)
        printf("[Multi-H] Proposed %d models from %d 3PT hypotheses\n", (int)cluster_homographies.size(), proposal_hypotheses);
    else if (ok && log_to_console)
        printf("[Multi-H] Proposed %d models from %d DLT hypotheses\n", (int)cluster_homographies.size(),
               proposal_hypotheses);
    return ok;
}

// The engine's sampler for the coming batch.  An engine library without the entry point has the uniform sampler only.
bool MultiH::ApplyProposalSampler(bool local)
{
    if (!caps.set_sampler) return !local;
    return Check(mh_set_sampler(engine, local ? MH_SAMPLER_LOCAL : MH_SAMPLER_UNIFORM, local ? proposal_uniform_per_16 : 0), "mh_set_sampler");
}

// `mask`: 1 = point still unexplained (in/out).  Appends the selected models to cluster_homographies.
// One hypothesis batch -> mh_propose_dlt4 (this rank's shard of it; mh_propose_3pt under PROPOSAL_SOURCE_3PT) -> mh_select_greedy: scoring, arg-max, claiming
// the winner's inliers and pruning the candidates all stay on the device; per round the host reads three control
// words.  Sharded (SetSharding): rank r owns counters [first + off_r, first + off_r + m_r); the ranks all-gather
// their int32 score vectors and the H each offers through the caller's transport on DEVICE buffers, and the selection
// order is the single-GPU one (highest score, lowest counter on ties), so world sizes 1..G give identical model lists.
bool MultiH::ProposeModels(int source, uint64_t seed, long long first, int M, int max_models, std::vector<unsigned char>& mask)
{
    const int need = std::max(minimum_inlier_number, 8);
    if (M <= 0 || max_models <= 0) return true;
    const int W = std::max(shard_world, 1), base = M / W, rem = M % W;
    const int mine = base + (shard_rank < rem ? 1 : 0);
    const long long off = (long long)shard_rank * base + std::min(shard_rank, rem);
    if (!ApplyProposalSampler(plan.proposal_local)) return false;      // (sticky on the engine, and engines are reused)
    if (source == PROPOSAL_SOURCE_HAF) {      // an empty shard too: mh_propose_haf(.., 0, ..) keeps the batch's record, which every rank's selection compares
        if (!Check(mh_propose_haf(engine, first + off, mine, proposal_haf_stride, plan.haf_members, sqr_threshold_homography), "mh_propose_haf"))
            return false;
    } else if (source == PROPOSAL_SOURCE_3PT) {      // the initial and the iterative batches alike; an empty shard keeps the batch's record here too
        if (!Check(mh_propose_3pt(engine, seed, first + off, mine), "mh_propose_3pt")) return false;
    } else if (mine > 0) {
        if (!Check(mh_propose_dlt4(engine, seed, first + off, mine), "mh_propose_dlt4")) return false;
    } else if (!Check(mh_set_models(engine, nullptr, 0), "mh_set_models")) {
        return false;
    }
    std::vector<double> H(9 * (size_t)max_models);
    int selected = 0;
    if (!Check(mh_set_tuning(engine, 30, proposal_refit ? 1 : 0), "mh_set_tuning(30)")) return false;
    if (selection_score == SELECTION_SCORE_MSAC && init_mode != INIT_STABLE_SETS) {      // (validated at the head of Process())
        if (!Check(mh_select_greedy_msac(engine, sqr_threshold_homography, need, max_models, mask.data(), H.data(), nullptr, nullptr,
                                         nullptr, &selected, (long long)M),
                   "mh_select_greedy_msac"))
            return false;
    } else if (!Check(mh_select_greedy(engine, sqr_threshold_homography, need, max_models, mask.data(), H.data(), nullptr, nullptr,
                                       &selected, (long long)M),
                      "mh_select_greedy"))
        return false;
    for (int i = 0; i < selected; ++i) cluster_homographies.push_back(MatFrom9(&H[9 * (size_t)i]));
    return true;
}

void MultiH::SetSharding(int rank, int world, AllGatherFn fn, void* ctx)
{
    shard_stream_allgather = nullptr;
    if (world <= 1 || !fn || rank < 0 || rank >= world) {
        shard_rank = 0; shard_world = 1; shard_allgather = nullptr; shard_ctx = nullptr;
        return;
    }
    shard_rank = rank; shard_world = world; shard_allgather = fn; shard_ctx = ctx;
}

void MultiH::SetShardingStream(int rank, int world, StreamAllGatherFn fn, void* ctx)
{
    shard_allgather = nullptr;
    if (world < 1 || !fn || rank < 0 || rank >= world) {
        shard_rank = 0; shard_world = 1; shard_stream_allgather = nullptr; shard_ctx = nullptr;
        return;
    }
    shard_rank = rank; shard_world = world; shard_stream_allgather = fn; shard_ctx = ctx;      // world == 1: a one-rank communicator
}

// Neighbourhood (M/MultiH.cpp:233-253).  Given hits are used as they are; otherwise the engine builds them in the
// same float32 (x1,y1,x2,y2) space (MultiH.h, SetNeighbourK / SetNeighbourRadius).
bool MultiH::BuildNeighbourhood()
{
    const int N = static_cast<int>(src_points.size());
    bool ok;
    if (!neighbours.empty()) {
        std::vector<int> rowptr(N + 1, 0), col;
        for (int i = 0; i < N; ++i) {
            if (i < (int)neighbours.size()) col.insert(col.end(), neighbours[i].begin(), neighbours[i].end());
            rowptr[i + 1] = static_cast<int>(col.size());
        }
        ok = Check(mh_set_neighbors_csr(engine, rowptr.data(), col.data(), N), "mh_set_neighbors_csr");
    } else if (neighbour_mode == NEIGHBOURS_APPROX) {
        // the reference's own rule as FLANN's default search answers it (MultiH.h, SetNeighbourApprox): built on the host —
        // where the reference builds it — from the float32 (x1, y1, x2, y2) vectors of :233-250, handed over as directed hits
        std::vector<double> pv(4 * (size_t)N);
        for (int i = 0; i < N; ++i) {
            pv[4 * (size_t)i] = (double)static_cast<float>(src_points[i].x);
            pv[4 * (size_t)i + 1] = (double)static_cast<float>(src_points[i].y);
            pv[4 * (size_t)i + 2] = (double)static_cast<float>(dst_points[i].x);
            pv[4 * (size_t)i + 3] = (double)static_cast<float>(dst_points[i].y);
        }
        std::vector<std::vector<int>> hits;
        multih::ApproxNeighbourHits(pv.data(), N, approx_trees, approx_checks, 1.0 / locality_lambda, approx_seed, hits);
        std::vector<int> rowptr(N + 1, 0), col;
        for (int i = 0; i < N; ++i) {
            col.insert(col.end(), hits[i].begin(), hits[i].end());
            rowptr[i + 1] = static_cast<int>(col.size());
        }
        if (log_to_console) printf("[Multi-H] %d approximate neighbourhood hits (%d trees, %d checks)\n", (int)col.size(), approx_trees, approx_checks);
        ok = Check(mh_set_neighbors_csr(engine, rowptr.data(), col.data(), N), "mh_set_neighbors_csr");
    } else if (neighbour_mode == NEIGHBOURS_KNN) {
        // the k nearest hits within the reference's radius 1 / locality_lambda (M/MultiH.cpp:252-253); see MultiH.h
        ok = Check(mh_build_neighbors_knn_radius(engine, std::min(knn, N - 1), 1.0 / locality_lambda), "mh_build_neighbors_knn_radius");
    } else {
        // the complete radius list, answered exactly; it grows like N^2, and beyond `neighbour_max_hits` the engine refuses
        long long hits = 0;
        const int rc = mh_build_neighbors_radius(engine, neighbour_radius, neighbour_max_hits, &hits);
        if (rc == MH_ERR_OVERFLOW) {
            printf("[Multi-H] %lld neighbourhood hits within %.1f px exceed the limit of %lld: using the %d nearest hits instead\n",
                   hits, neighbour_radius, neighbour_max_hits, std::min(knn, N - 1));
            ok = Check(mh_build_neighbors_knn_radius(engine, std::min(knn, N - 1), neighbour_radius), "mh_build_neighbors_knn_radius");
        } else {
            ok = Check(rc, "mh_build_neighbors_radius");
            if (ok && log_to_console) printf("[Multi-H] %lld neighbourhood hits within %.1f px\n", hits, neighbour_radius);
        }
    }
    return ok;
}

void MultiH::ClusterMergingAndLabeling()
{
    auto start = std::chrono::system_clock::now();
    const int N = static_cast<int>(src_points.size());
    const bool ok = BuildNeighbourhood();
    std::chrono::duration<double> el = std::chrono::system_clock::now() - start;
    printf("[Multi-H] Adjacency-matrix calculation time = %f secs\n", el.count());      // :258
    if (!ok) { cluster_homographies.clear(); return; }

    start = std::chrono::system_clock::now();
    int iteration_number = 0;
    labeling.resize(N, -1);                                                             // :263
    double lastEnergy = INT_MAX;
    int not_changed_number = 0;
    labeling_steps_run = 0;
    labeling_is_current = false;
    merge_log_open = false;
    merge_log.clear();
    drop_log.clear();

    const bool timing = std::getenv("MULTIH_TIMING") != nullptr;                        // diagnostic: where the loop's time goes
    double merge_s = 0.0, label_s = 0.0;
    auto seconds_since = [](std::chrono::time_point<std::chrono::system_clock> t0) {
        return std::chrono::duration<double>(std::chrono::system_clock::now() - t0).count();
    };
    while (iteration_number++ < MAX_ITERATION_NUMBER) {                                 // :267
        bool changed = false;
        loop_iteration = iteration_number;
        const auto t_merge = std::chrono::system_clock::now();
        const bool merged = MergingStep(changed);
        merge_s += seconds_since(t_merge);
        if (!merged) break;
        if (iter_hypotheses > 0 && iteration_number > 1) {
            // PEARL re-proposal on the points the current labeling leaves unexplained
            std::vector<unsigned char> mask(N);
            for (int i = 0; i < N; ++i) mask[i] = labeling[i] < 0 ? 1 : 0;
            const size_t before = cluster_homographies.size();
            if (!ProposeModels(plan.iterative_source, proposal_seed, (long long)iteration_number * iter_hypotheses + proposal_hypotheses,
                               iter_hypotheses, iter_max_new, mask))
                break;
            if (cluster_homographies.size() != before) changed = true;
        }
        if (changed) not_changed_number = 0;
        else ++not_changed_number;

        if (cluster_homographies.size() == 1) {                                         // :280-285
            labeling.resize(N, -1);
            ComputeInliersOfHomography(0);
            break;
        } else if (cluster_homographies.size() == 0)
            break;

        double energy;
        const auto t_label = std::chrono::system_clock::now();
        const bool labelled = LabelingStep(energy, changed);
        label_s += seconds_since(t_label);
        if (labelled) ++labeling_steps_run;
        if (timing) {
            long long st[24] = {};
            (void)mh_get_expand_stats(engine, st);
            printf("[Multi-H] iteration %d: %d clusters, changed %d, merging %.1f ms so far, labeling %.1f ms so far (this step %.1f ms: "
                   "%lld cycles, %lld moves solved, core %lld / max %lld, %lld relabels, %lld barriers, solver %.1f ms of which tail rounds %.1f ms)\n",
                   iteration_number, (int)cluster_homographies.size(), changed ? 1 : 0, merge_s * 1e3, label_s * 1e3,
                   seconds_since(t_label) * 1e3, st[0], st[10], st[11], st[12], st[14], st[13], (double)st[15] * 1e-3, (double)st[19] * 1e-3);
            std::vector<int> tr(8 * 64, 0);              // per-move log, when the caller switched it on (mh_set_tuning key 8)
            if (mh_get_expand_trace(engine, tr.data(), 64) == MH_OK)
                for (int mv = 0; mv < 64; ++mv)
                    if (tr[8 * mv + 6] > 200000)          // moves of more than 2 ms
                        printf("[Multi-H]    move %d: core %d, %d workgroups, %d relabels, %d intervals, %d push phases, %d barriers, %.1f ms\n",
                               mv, tr[8 * mv], tr[8 * mv + 1], tr[8 * mv + 2], tr[8 * mv + 3], tr[8 * mv + 4], tr[8 * mv + 5],
                               tr[8 * mv + 6] * 1e-5);
        }
        {
            // a labeling that ran on a cut-down solver grid (barrier timeouts on a shared GPU) is not silent: same
            // labels, but slower — say so whenever it happens
            long long st[24] = {};
            if (labelled && mh_get_expand_stats(engine, st) == MH_OK && st[20] > 0)
                printf("[Multi-H] iteration %d: the alpha-expansion's solver launch was restarted %lld time(s) after a grid-barrier "
                       "timeout and ran on %lld workgroups (is the GPU shared?)\n", iteration_number, st[20], st[21]);
        }
        if (!labelled) break;
        if (log_to_console)
            printf("Iteration %d.   Number of clusters = %d   Energy = %f\n", iteration_number,
                   (int)cluster_homographies.size(), energy);

        if ((!changed && std::abs(lastEnergy - energy) < CONVERGENCE_THRESHOLD) || not_changed_number > 10 ||
            (fixed_iterations > 0 && iteration_number >= fixed_iterations)) {           // :295
            final_energy = energy;
            break;
        }
        lastEnergy = energy;
    }
    printf("[Multi-H] Optimization started... Iteration %d\n", iteration_number);       // :305
    el = std::chrono::system_clock::now() - start;
    loop_seconds = el.count();
    printf("[Multi-H] Alternating optimization time = %f secs\n", el.count());          // :310
    final_iteration_number = iteration_number - 1;                                      // :311
}

// MergingStep, M/MultiH.cpp:352-471: models -> 6-D features -> mean-shift modes -> one
// homography per mode -> inlier scoring + collinearity filter -> `changed` iff the count changed.
// Mode -> homography is GetHomography3PT with its LM refinement (:995-1055, multih::Homography3PT).
// The N x modes scoring and the 3x3 scatter eigen test (:430-463) run on the GPU
// (mh_inlier_moments).
// (multih_internal.h says what goes in and out)
int multih::detail::MergingStepOnEngine(mh_engine* engine, const double* H, int nh, const double F[9], double thr_h, double straightness,
                                        uint64_t seed, std::vector<double>& kept, uint64_t* draws)
{
    kept.clear();
    std::vector<double> cand;
    const int nc = F ? multih::MergeCandidates(H, nh, F, thr_h, seed, nullptr, nullptr, cand, nullptr, draws)
                     : multih::MergeCandidatesMedoid(H, nh, thr_h, seed, nullptr, nullptr, cand, nullptr, draws);
    if (nc == 0) return MH_OK;
    int rc = mh_set_models(engine, cand.data(), nc);
    if (rc != MH_OK) return rc;
    std::vector<double> mom(6 * (size_t)nc), mineig(nc);
    rc = mh_inlier_moments(engine, thr_h * thr_h, mom.data(), mineig.data());
    if (rc != MH_OK) return rc;
    for (int i = 0; i < nc; ++i) {
        const int inl = static_cast<int>(mom[6 * (size_t)i]);
        if (mineig[i] < straightness || inl < 3) continue;                             // :462
        kept.insert(kept.end(), cand.begin() + 9 * (size_t)i, cand.begin() + 9 * (size_t)(i + 1));
    }
    return MH_OK;
}

bool MultiH::MergingStep(bool& changed)
{
    if (merge_mode == MERGE_ENERGY) return MergingStepEnergy(changed);
    const int nh = static_cast<int>(cluster_homographies.size());
    changed = false;
    if (nh == 0) return true;
    std::vector<double> H = FlatModels();
    std::vector<double> kept9;
    const int rc = MergingStepOnEngine(engine, H.data(), nh, epipolar_free ? nullptr : fundamental_matrix, threshold_homography, straightness_threshold,
                                       proposal_seed ^ 0x4d53u ^ (merge_rng_counter << 20), kept9, nullptr);
    ++merge_rng_counter;
    if (!Check(rc, "MergingStep (mh_set_models / mh_inlier_moments)")) return false;
    std::vector<cv::Mat> kept;
    for (size_t i = 0; i + 9 <= kept9.size(); i += 9) kept.push_back(MatFrom9(&kept9[i]));
    changed = kept.size() != cluster_homographies.size();                               // :468
    if (changed) cluster_homographies = kept;                                           // :469-470
    return true;
}

// MergingStep under MERGE_ENERGY (MultiH.h, SetMergeMode): the collinearity filter of MergingStepOnEngine on the models as they
// stand, and — once a labeling exists — in front of it the joins that lower the labeling's energy.
bool MultiH::MergingStepEnergy(bool& changed)
{
    const int nh = static_cast<int>(cluster_homographies.size());
    const int N = static_cast<int>(labeling.size());
    changed = false;
    if (nh == 0) return true;
    std::vector<double> H = FlatModels();
    int count = nh;
    MergeLogRecord rec;
    const bool evaluate = labeling_is_current;
    if (!Check(mh_set_models(engine, H.data(), nh), "MergingStep (mh_set_models)")) return false;
    if (evaluate) {
        rec.iteration = loop_iteration;
        rec.models_before = nh;
        const std::vector<int> pairs = multih::MergePairList(H.data(), nh);
        const int npairs = static_cast<int>(pairs.size() / 2);
        rec.pairs = npairs;
        if (!Check(mh_labeling_energy(engine, labeling.data(), &rec.E_before, nullptr), "MergingStep (mh_labeling_energy)")) return false;
        std::vector<double> H_ab(9 * (size_t)npairs);
        std::vector<long long> delta(npairs);
        std::vector<int> status(npairs);
        if (!Check(mh_merge_deltas(engine, labeling.data(), pairs.data(), npairs, H_ab.data(), delta.data(), nullptr, status.data()),
                   "MergingStep (mh_merge_deltas)"))
            return false;
        const std::vector<int> accepted = multih::SelectMergesWithLabelCost(pairs.data(), delta.data(), status.data(), npairs, nh, plan.label_cost_beta);
        for (int k : accepted) rec.sum_delta += delta[k];
        rec.merges_accepted = static_cast<long long>(accepted.size());
        count = multih::ApplyMerges(pairs.data(), H_ab.data(), accepted, N, labeling.data(), H.data(), nh);
        if (count != nh && !Check(mh_set_models(engine, H.data(), count), "MergingStep (mh_set_models)")) return false;
        // the drop move, on the labeling and models the joins left: at most one label per step
        if (plan.label_cost_beta > 0 && count > 0) {
            DropLogRecord drop;
            drop.iteration = loop_iteration;
            drop.beta = plan.label_cost_beta;
            std::vector<char> in_use(count, 0);
            for (int j = 0; j < N; ++j)
                if (labeling[j] >= 0 && labeling[j] < count) in_use[labeling[j]] = 1;
            std::vector<int> cand;
            for (int l = 0; l < count; ++l)
                if (in_use[l]) cand.push_back(l);
            const int ncand = static_cast<int>(cand.size());
            drop.candidates = ncand;
            drop.E_before = rec.E_before + rec.sum_delta;
            if (!accepted.empty() &&
                !Check(mh_labeling_energy(engine, labeling.data(), &drop.E_before, nullptr), "MergingStep (mh_labeling_energy)"))
                return false;
            drop.E_after = drop.E_before;
            if (ncand > 0) {
                std::vector<long long> d_delta(ncand), d_parts(5 * (size_t)ncand);
                std::vector<int> d_status(ncand), alt(N);
                if (!Check(mh_drop_deltas(engine, labeling.data(), cand.data(), ncand, d_delta.data(), d_parts.data(), d_status.data(),
                                          alt.data()),
                           "MergingStep (mh_drop_deltas)"))
                    return false;
                const int pick = multih::SelectDrop(cand.data(), d_delta.data(), d_status.data(), ncand, plan.label_cost_beta);
                if (pick >= 0) {
                    int to_outlier = 0;
                    drop.dropped = cand[pick];
                    drop.members = d_parts[5 * (size_t)pick];
                    drop.delta = d_delta[pick];
                    count = multih::ApplyDrop(cand[pick], alt.data(), N, labeling.data(), H.data(), count, &to_outlier);
                    drop.to_outlier = to_outlier;
                    if (count > 0) {
                        if (!Check(mh_set_models(engine, H.data(), count), "MergingStep (mh_set_models)")) return false;
                        if (!Check(mh_labeling_energy(engine, labeling.data(), &drop.E_after, nullptr), "MergingStep (mh_labeling_energy)"))
                            return false;
                    } else {
                        drop.E_after = drop.E_before + drop.delta;       // no model is left to ask: every site is an outlier
                    }
                    rec.sum_delta += drop.delta;
                }
            }
            drop_log.push_back(drop);
        }
    }
    // the collinearity filter (M/MultiH.cpp:446-463) on the models as they stand
    std::vector<double> mom(6 * (size_t)count), mineig(count);
    if (count > 0 &&                                 // (0: the drop took the last label, the engine's models are stale)
        !Check(mh_inlier_moments(engine, threshold_homography * threshold_homography, mom.data(), mineig.data()), "MergingStep (mh_inlier_moments)"))
        return false;
    std::vector<char> remove(count, 0);
    int filtered = 0;
    for (int i = 0; i < count; ++i)
        if (mineig[i] < straightness_threshold || static_cast<int>(mom[6 * (size_t)i]) < 3) { remove[i] = 1; ++filtered; }
    if (filtered) count = multih::RemoveModels(remove, N, labeling.data(), H.data(), count);
    if (evaluate) {
        rec.models_filtered = filtered;
        rec.E_start = rec.E_before + rec.sum_delta;
        if (count > 0 && (filtered || count != nh)) {
            if (!Check(mh_set_models(engine, H.data(), count), "MergingStep (mh_set_models)")) return false;
            if (!Check(mh_labeling_energy(engine, labeling.data(), &rec.E_start, nullptr), "MergingStep (mh_labeling_energy)")) return false;
        }
        merge_log.push_back(rec);
        merge_log_open = true;
    }
    changed = count != nh;
    if (changed || evaluate) {
        cluster_homographies.clear();
        for (int i = 0; i < count; ++i) cluster_homographies.push_back(MatFrom9(&H[9 * (size_t)i]));
    }
    return true;
}

bool MultiH::LabelingStep(double& energy, bool changed)
{
    energy = 0;
    if (!UploadModels()) return false;
    int cycles = 0;
    // under MERGE_ENERGY the merges keep the labeling valid for the models: warm whenever there is one
    const int warm = (merge_mode == MERGE_ENERGY && labeling_is_current) ? 1 : (changed ? 0 : 1);
    if (!Check(mh_labeling_step(engine, warm, labeling.data(), &energy, &cycles), "mh_labeling_step"))
        return false;
    labeling_is_current = true;
    if (merge_log_open) {
        merge_log.back().E_expansion = static_cast<long long>(energy);
        merge_log_open = false;
    }
    return DownloadModels(static_cast<int>(cluster_homographies.size()));
}

void MultiH::ComputeInliersOfHomography(int idx)
{
    if (!UploadModels()) return;
    Check(mh_inliers_of_model(engine, idx, sqr_threshold_homography, idx, labeling.data()), "mh_inliers_of_model");
}

// HandleDegenerateCase (M/MultiH.cpp:719-741) calls cv::findHomography(RANSAC) on the ORIGINAL
// points and labels its inliers 0.  Here: best-supported of `proposal_hypotheses` DLT hypotheses.
void MultiH::HandleDegenerateCase()
{
    const int N = static_cast<int>(src_points_original.size());
    labeling.assign(N, -1);
    // The engine may still hold the FILTERED, refined correspondences (Process() re-uploads them after
    // GetFundamentalMatrixAndRefineData); the reference fits and labels the originals here (:725-739).
    if (!UploadCorrespondences(src_points_original, dst_points_original, affinities_original)) return;
    const int M = std::max(proposal_hypotheses, 1000);
    if (!ApplyProposalSampler(false)) return;          // this batch is uniform whatever SetProposalSampler says (the oracle's mho_handle_degenerate defines it)
    if (!Check(mh_propose_dlt4(engine, proposal_seed ^ 0xdeadull, 0, M), "mh_propose_dlt4")) return;
    // the winner: by weight (the scores stay on the device, the engine's arg-max picks) or by count (the first maximum)
    long long best = 0;
    if (tail_score == TAIL_SCORE_MSAC) {
        if (!Check(mh_score_msac(engine, sqr_threshold_homography, nullptr, nullptr, nullptr), "mh_score_msac")) return;
        if (!Check(mh_select_best_msac(engine, &best, nullptr, nullptr), "mh_select_best_msac")) return;
    } else {
        std::vector<int> counts(M);
        if (!Check(mh_score(engine, sqr_threshold_homography, nullptr, counts.data()), "mh_score")) return;
        best = std::max_element(counts.begin(), counts.end()) - counts.begin();
    }
    if (tail_refit > 0) {
        // that ONE model comes back, is refitted to all its inliers on the original points, and the refit's inliers are labelled
        double Hb[9], Hr[9];
        if (!Check(mh_get_model(engine, (int)best, Hb), "mh_get_model")) return;
        std::vector<unsigned char> inl(N);
        if (!Check(mh_refit_homography(engine, Hb, sqr_threshold_homography, tail_refit, Hr, inl.data(), nullptr, nullptr),
                   "mh_refit_homography"))
            return;
        for (int i = 0; i < N; ++i) labeling[i] = inl[i] ? 0 : -1;
        if (!PolishTailModel(Hr)) return;
        cluster_homographies.push_back(MatFrom9(Hr));
        return;
    }
    if (tail_score == TAIL_SCORE_MSAC || tail_polish > 0) {
        // one H comes back; its inliers are labelled, and with SetTailPolish it is polished over them
        if (!Check(mh_inliers_of_model(engine, (int)best, sqr_threshold_homography, 0, labeling.data()), "mh_inliers_of_model"))
            return;
        double Hb[9];
        if (!Check(mh_get_model(engine, (int)best, Hb), "mh_get_model")) return;
        if (!PolishTailModel(Hb)) return;
        cluster_homographies.push_back(MatFrom9(Hb));
        return;
    }
    std::vector<double> H(9 * (size_t)M);
    if (!Check(mh_get_models(engine, H.data()), "mh_get_models")) return;
    if (!Check(mh_inliers_of_model(engine, (int)best, sqr_threshold_homography, 0, labeling.data()), "mh_inliers_of_model"))
        return;
    cluster_homographies.push_back(MatFrom9(&H[9 * (size_t)best]));
}
