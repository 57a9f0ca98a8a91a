// MultiH.h — host-side mirror of the reference's class `MultiH`
// (M/MultiH.h:20-149, M/ = /root/reference/MultiH/MultiH/) implemented over the
// C ABI of the gfx950 engine (include/multih_hip.h).  Same class name, same
// public signatures, same defaults, same label / index conventions, same error
// behaviour (Process() returns false and writes "Error: Features are not set!"
// to stderr, M/MultiH.cpp:44-50), so `ApplyMultiH` (M/main.cpp:232-311) can
// construct it, call Process and read the getters unchanged.
//
// Scope: Process() follows the reference's Process() (M/MultiH.cpp:42-98) stage by stage with every heavy
// stage on the GPU.  The front half (GetFundamentalMatrixAndRefineData, M/MultiH.cpp:770-848) has two routes: the
// caller hands over F and the epipole (SetEpipolarGeometry — e.g. the reference's own OpenCV code; the points are
// then taken as already refined), or the engine estimates them itself (8-point RANSAC with Sampson scoring and a
// least-squares refit, then the per-correspondence Hartley-Sturm correction, affine-consistency filter and optimal
// affinity of :807-838).  Initial models: SetInitialHomographies, the reference's stable point sets
// (INIT_STABLE_SETS: per-point HAF homographies -> mean shift -> 3-point fits, :604-717), or — the default — random
// minimal samples with the batched 4-point DLT (north_star).  Neighbour hits can be supplied (SetNeighbours) or are
// built on the GPU.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "cv_shim.h"

#define DEFAULT_THRESHOLD_FUNDAMENTAL_MATRIX 3.0    // M/MultiH.h:7
#define DEFAULT_THRESHOLD_HOMOGRAPHY 2.5            // :8
#define DEFAULT_LOCALITY 0.002                      // :9
#define DEFAULT_LAMBDA 0.5                          // :10
#define DEFAULT_AFFINE_THRESHOLD 1.0                // :12
#define DEFAULT_LINENESS_THRESHOLD 0.005            // :13
#define MAX_ITERATION_NUMBER 500                    // :14
#define CONVERGENCE_THRESHOLD 1e-5                  // :15

struct mh_engine;

class MultiH {
public:
    MultiH(double _thr_fund_mat = DEFAULT_THRESHOLD_FUNDAMENTAL_MATRIX,
           double _thr_hom = DEFAULT_THRESHOLD_HOMOGRAPHY, double _locality = DEFAULT_LOCALITY,
           double _lambda = DEFAULT_LAMBDA, int _minimum_inlier_number = 0);
    ~MultiH();
    void Release();

    // M/MultiH.h:58-59.  Arguments by value, copied into *_original (M/MultiH.cpp:32-40).
    bool Process(std::vector<cv::Point2d> _srcPoints, std::vector<cv::Point2d> _dstPoints,
                 std::vector<cv::Mat> _affines);
    bool Process();
    // The point-only route (no affinities; the reference has no such route): the same stages as Process() with the
    // per-correspondence refinement reduced to the Hartley-Sturm correction (mh_refine_points) and every homography refit —
    // the loop's re-estimation and the proposal refit — by the 3-point least squares GetHomography3PT without LM refinement
    // (MH_ESTIMATOR_3PT), which needs only the points and F.  GetAffinities() then returns an empty vector.  The stable point
    // sets (INIT_STABLE_SETS) need per-point HAF homographies: with that initialisation this call prints an error and
    // returns false.
    bool Process(std::vector<cv::Point2d> _srcPoints, std::vector<cv::Point2d> _dstPoints);

    // M/MultiH.h:61-75
    int GetLabel(int idx) { return labeling[idx]; }
    void GetLabels(std::vector<int>& _labeling) { _labeling = labeling; }
    void GetSourcePoints(std::vector<cv::Point2d>& _src_points) { _src_points = src_points; }
    // The reference returns the SOURCE points here (M/MultiH.h:64, SURVEY A-9); result files
    // written by the harness therefore carry x2,y2 = x1,y1.  Reproduced for drop-in parity.
    void GetDestinationPoints(std::vector<cv::Point2d>& _dst_points) { _dst_points = src_points; }
    void GetAffinities(std::vector<cv::Mat>& _affinities) { _affinities = affinities; }
    int GetPointNumber() { return static_cast<int>(labeling.size()); }
    int GetClusterNumber() { return static_cast<int>(cluster_homographies.size()); }
    int GetIterationNumber() { return final_iteration_number; }
    cv::Mat GetHomography(int idx) { return cluster_homographies[idx - 1]; }   // 1-based, :69
    double GetEnergy() { return final_energy; }
    double GetHomographyThreshold() { return threshold_homography; }
    // M/MultiH.h:71, M/MultiH.cpp:314-350: a filled circle per labelled correspondence, colour by plane.
    void DrawClusters(cv::Mat& img1, cv::Mat& img2, int size);
    // Post-filter of the reference (M/MultiH.cpp:100-222): multih::CompatibilityCheck with the trials' order statistics
    // from the engine (mh_compat_trial_stats).
    void HomographyCompatibilityCheck();
    // The same place in Process() under COMPAT_FIT_DLT: multih::CompatibilityCheckDlt with the statistics from the engine
    // (mh_compat_dlt_medians).  Needs no F.
    void HomographyCompatibilityCheckDlt();

    // ---- extension points: outputs of the reference's OpenCV front half ----
    // fundamental_matrix (row-major) and epipole_2 = (x, y, 1) (M/MultiH.cpp:775-799).
    void SetEpipolarGeometry(const double F[9], const double e2[2]);
    // `neighbours` (M/MultiH.cpp:252-253): per query the hit indices (self allowed).
    void SetNeighbours(const std::vector<std::vector<int>>& hits);
    // Without SetNeighbours the hits are built on the GPU in the reference's float32 (x1,y1,x2,y2) space.  The reference
    // asks FLANN for every correspondence within 1 / locality_lambda pixels (radiusMatch, :252-253), but with FLANN's
    // default search (4 randomised KD-trees, 32 checks) the answer is a few dozen approximate nearest neighbours
    // inside that ball, never the ball itself — which at the harness defaults holds hundreds of points, enough for the
    // Potts term to swamp the data term (on the reference's own barrsmith pair the complete list leaves no plane
    // standing).  Default here: the k = 16 EXACT nearest hits that lie within the reference's radius.
    void SetNeighbourK(int k) { neighbour_mode = NEIGHBOURS_KNN; knn = k; }
    // The complete radius list instead (every hit within `radius`, exact), bounded by `max_hits` because it grows like
    // N^2: beyond the bound the k nearest hits within the radius are used and a line says so.
    void SetNeighbourRadius(double radius, long long max_hits = 1ll << 28) { neighbour_mode = NEIGHBOURS_RADIUS; neighbour_radius = radius; neighbour_max_hits = max_hits; }
    // r05: the reference's neighbourhood as FLANN's DEFAULT search answers it — `trees` randomised KD-trees (4), best-bin-first
    // with `checks` examined points per query (32), the hits among them inside 1 / locality_lambda — re-enacted on the host
    // with the engine's counter RNG (approx_neighbours.cpp; OpenCV / FLANN are outside /root/reference: restated from the
    // published algorithm, parity unpinned).  About 29 one-way hits per correspondence, 70 % of the exact 31 nearest.
    void SetNeighbourApprox(int trees = 4, int checks = 32, uint64_t seed = 0x464c414e4eull)
    { neighbour_mode = NEIGHBOURS_APPROX; approx_trees = trees; approx_checks = checks; approx_seed = seed; }
    // k of that fallback (default 16) without leaving the radius mode
    void SetFallbackK(int k) { knn = k; }
    // Initial cluster_homographies (what EstablishStablePointSets hands to the loop).
    void SetInitialHomographies(const std::vector<cv::Mat>& Hs);
    // How the initial models are made when SetInitialHomographies was not called:
    //   INIT_DLT          random minimal samples -> batched 4-point DLT -> greedy selection (north_star)
    //   INIT_STABLE_SETS  the reference's own route: per-point HAF homographies
    //                     (ComputeLocalHomographies, M/MultiH.cpp:696-717) -> 10-D mean shift ->
    //                     one 3-point LSQ homography per cluster of >= 3 points
    //                     (EstablishStablePointSets, :604-694), all heavy steps on the GPU.
    enum { INIT_DLT = 0, INIT_STABLE_SETS = 1 };
    void SetInitialisation(int mode) { init_mode = mode; }
    // Propose step used when no initial models are given: `hypotheses` random 4-tuples ->
    // DLT -> greedy selection of at most `max_models` models with >= max(min inliers, 8).
    void SetProposal(uint64_t seed, int hypotheses, int max_models);
    // A CAP on the loop's iterations (north_star configs[4]: "20 propose-expand iterations"): with n > 0 the loop also stops
    // after its n-th LabelingStep.  The reference's own stop rule (:295: no change and the same energy, or more than ten
    // unchanged iterations) stays in force — a loop that has converged after three iterations runs three, not n.  0 = the
    // reference's rule alone.  How many LabelingSteps the last Process() ran: GetLabelingStepsRun() (GetIterationNumber()
    // is the reference's iteration_number - 1, :311, i.e. one less when the loop ended behind a LabelingStep).
    void SetFixedIterations(int n) { fixed_iterations = n; }
    int GetLabelingStepsRun() const { return labeling_steps_run; }
    // PEARL-style re-proposal (north_star "propose-expand iterations"; the reference proposes only
    // once, before the loop): every iteration samples `hypotheses` fresh DLT hypotheses, scores them
    // on the points currently labelled outlier and appends at most `max_new` models that gather
    // >= max(min inliers, 8) of them.  0 hypotheses (default) keeps the reference's behaviour.
    void SetIterativeProposal(int hypotheses, int max_new) { iter_hypotheses = hypotheses; iter_max_new = max_new; }
    // r05: every winner of the greedy selection is refitted to the correspondences it explains — the loop's per-label HAF
    // least squares with one label (M/MultiH.cpp:913-989) — before it claims them, and the refit takes its place when it
    // explains at least as many (mh_set_tuning key 30).  A hypothesis fitted to four matches explains 60-70 % of its plane;
    // what it leaves behind used to feed models that sit between two planes.  Default on.
    void SetProposalRefit(bool on) { proposal_refit = on; }
    // The re-estimator of Process() with affinities (the point-only Process() always takes ESTIMATOR_3PT): the HAF
    // non-minimal fit (M/MultiH.cpp:913-989, the reference's; default) or the 3-point least squares from the points alone.
    // ESTIMATOR_DLT: the normalised N-point DLT over each label's members (MH_ESTIMATOR_DLT), which reads neither F nor the
    // affinities; the point-only Process() honours it (the two other values give ESTIMATOR_3PT there).
    enum { ESTIMATOR_HAF = 0, ESTIMATOR_3PT = 1, ESTIMATOR_DLT = 2 };
    void SetEstimator(int e) { estimator = e; }
    // The route without epipolar geometry (default off), for pairs no single F describes: independently moving planes, a
    // rotating camera in front of moving planes, a plane-dominated pair whose F is unstable.  With it on, both Process()
    // forms estimate no F and refine or drop no correspondence (GetFrontStages() reports the input count four times; a
    // caller's SetEpipolarGeometry is ignored with one log line), run the engine under ESTIMATOR_DLT without mh_set_epipolar
    // (affinities are uploaded if given and never read), take the medoid of each mean-shift mode as MergingStep's candidate
    // (multih::MergeCandidatesMedoid) and, under COMPAT_FIT_3PT only, skip HomographyCompatibilityCheck, whose trials are then
    // 3-point fits with F (one log line); under COMPAT_FIT_DLT the check runs here too (SetCompatibilityFit).
    // INIT_STABLE_SETS, PROPOSAL_SOURCE_HAF and PROPOSAL_SOURCE_3PT need F: Process() refuses them with a message.
    void SetEpipolarFree(bool on) { epipolar_free = on; }
    // The data term of the labeling (mh_set_data_term, include/multih_hip.h): DATA_TERM_REFERENCE is dataEnergy
    // (M/MultiH.cpp:473-504), whose cost inside the truncation threshold FALLS as the fit gets worse (default);
    // DATA_TERM_RISING drops its `1.0 -`, so the cost rises with the error.  Process() applies it to its engine on every
    // call, on both initialisation routes and the point-only route; nothing on the host evaluates the data term itself
    // (the loop's energy is the engine's).  Any other value makes Process() fail with a message.
    enum { DATA_TERM_REFERENCE = 0, DATA_TERM_RISING = 1 };
    void SetDataTerm(int t) { data_term = t; }
    // The weight of a neighbour pair in the smoothness term (mh_set_smoothness_weights, include/multih_hip.h, which defines the
    // rule): SMOOTHNESS_UNIFORM pays the Potts price round(100 lambda) times the pair's hit multiplicity whatever the distance
    // (the reference's smoothnessEnergy; default; rho_px and q_max are not looked at).  SMOOTHNESS_CAUCHY multiplies that by
    // q = max(1, round(q_max rho^2 / (rho^2 + d))), d the squared distance of the two correspondences in (x1,y1,x2,y2): q_max
    // for coincident sites, q_max / 2 at distance rho_px, 1 far away — PEARL's distance-weighted smoothness with a profile
    // that has an exact definition.  A near pair then costs q_max times what it cost; lambda scales both terms of the energy,
    // so SetSmoothnessWeights(CAUCHY, rho, q) with lambda / sqrt(q) keeps the short-range balance.  Nothing is rescaled here.
    // Process() applies it to its engine on every call — every rank of a sharded run does, the labeling is replicated —, with
    // explicit neighbours (SetNeighbours) and under all three neighbourhood modes.  Nothing on the host evaluates the term:
    // the LabelingStep, and the merges and drops of MERGE_ENERGY and SetLabelCost (mh_labeling_energy, mh_merge_deltas,
    // mh_drop_deltas), pick the weights up through the engine.  CAUCHY with rho_px not finite or <= 0, q_max outside
    // [1, 256], or another rule makes Process() fail with a message.
    enum { SMOOTHNESS_UNIFORM = 0, SMOOTHNESS_CAUCHY = 1 };
    void SetSmoothnessWeights(int rule, double rho_px, int q_max = 16) { smoothness_rule = rule; smoothness_rho = rho_px; smoothness_q_max = q_max; }
    // The error the whole route measures (mh_set_residual_mode with mh_set_residual_scope(MH_RESIDUAL_SCOPE_ROUTE),
    // include/multih_hip.h): RESIDUAL_FORWARD is the reference's one-way transfer error |H p1 - p2|^2 (default);
    // RESIDUAL_SYMMETRIC adds the backward term |adj(H) p2 - p1|^2.  Under it the route scores and selects its proposals,
    // merges (the moments' inliers), labels (the data term's table) and finishes (the one-cluster exit, the degenerate tail)
    // by the symmetric error at the caller's thr_hom, unscaled — the symmetric error of a well-fitted pair is about twice
    // the forward one, so a caller who wants the same inlier band passes thr_hom * sqrt(2).  Process() applies mode and
    // scope to its engine on every call, both ways, on every route (point-only, epipolar-free, sharded: the ranks' records
    // carry the mode).  TAIL_SCORE_MSAC and SELECTION_SCORE_MSAC are forward-only: together with RESIDUAL_SYMMETRIC
    // Process() refuses them up front with a message.  The refit, polish, reweight and compatibility modes (SetTailRefit,
    // SetTailPolish, SetModelPolish, SetModelReweight*, SetEstimatorReweight*, SetCompatibilityFit) combine with it and keep
    // measuring the forward error inside.  Any other value makes Process() fail with a message.
    enum { RESIDUAL_FORWARD = 0, RESIDUAL_SYMMETRIC = 1 };
    void SetResidual(int r) { residual = r; }
    // How the degenerate tail (HandleDegenerateCase) ranks its DLT hypotheses: TAIL_SCORE_COUNT by the inlier count (mh_score
    // and the first maximum; default), TAIL_SCORE_MSAC by the MSAC weight of include/multih_hip.h (mh_score_msac +
    // mh_select_best_msac: among hypotheses the one whose inliers fit best, the lowest index on ties; only the winning H is
    // fetched).  Everything else in the tail is the same: the original points, the uniform batch, the inliers at thr^2, label 0.
    // Any other value makes Process() fail with a message.
    enum { TAIL_SCORE_COUNT = 0, TAIL_SCORE_MSAC = 1 };
    void SetTailScore(int t) { tail_score = t; }
    // Refit of the degenerate tail's winner: 0 (default) returns the 4-point hypothesis as it was proposed; n in [1, 16] hands
    // the winner — picked exactly as above, by count or by weight — to mh_refit_homography (include/multih_hip.h: the normalised
    // N-point DLT on all its inliers, at most n rounds, a refit kept only while it explains at least as many points), labels the
    // refit's inliers 0 and returns the refit.  What cv::findHomography(CV_RANSAC) does behind its winning sample, without its
    // LM polish.  Works on the point-only route and on every rank of a sharded run alike.  Any other value makes Process() fail
    // with a message.
    void SetTailRefit(int iterations) { tail_refit = iterations; }
    // Levenberg-Marquardt polish of the degenerate tail's result: 0 (default) off; n in [1, 32] hands the tail's model — the
    // winner, refitted when SetTailRefit says so — with its inliers on the original points as label 0 to
    // mh_polish_homographies (include/multih_hip.h: at most n iterations of OpenCV's LM schedule on the forward transfer error)
    // and returns the polished model.  The labels stay those of the model in front of the polish, as OpenCV's mask does.
    // SetTailRefit(1) with SetTailPolish(10) is cv::findHomography's sequence.  Any other value makes Process() fail with a
    // message.
    void SetTailPolish(int iterations) { tail_polish = iterations; }
    // The same polish at the very end of Process() on the normal path (more than one cluster left, after the compatibility
    // check): every cluster's homography over the correspondences that carry its label, in one call.  Labels, energy and
    // iteration count are unchanged.  0 (default) off; n in [1, 32]; works on the point-only route and on every rank of a
    // sharded run alike.  Any other value makes Process() fail with a message.
    void SetModelPolish(int iterations) { model_polish = iterations; }
    // Reweighted refit of the final models (mh_reweight_homographies, include/multih_hip.h): where SetModelPolish runs, and in
    // front of it when both are set, every cluster's homography is refitted over the correspondences that carry its label by
    // at most `rounds` reweighted N-point DLT rounds, weights 1 - d2 / scale_px^2 under the model that stands (scale_px = 0:
    // the homography threshold).  Labels, energy and iteration count are unchanged.  0 (default) off; rounds in [1, 16]; reads
    // the points alone, so every route can use it.  Any other value makes Process() fail with a message.
    void SetModelReweight(int rounds, double scale_px = 0) { model_reweight = rounds; model_reweight_scale = scale_px; }
    // The same rounds inside the loop: under ESTIMATOR_DLT (SetEpipolarFree(true) included) every re-estimation starts from the
    // label's standing model and runs `rounds` reweighted rounds instead of the plain fit (mh_set_estimator_reweighting).  The
    // other estimators ignore it.  0 (default) off; rounds in [1, 16]; any other value makes Process() fail with a message.
    void SetEstimatorReweight(int rounds, double scale_px = 0) { estimator_reweight = rounds; estimator_reweight_scale = scale_px; }
    // The same two with the scale taken from the data (mh_reweight_homographies_auto, mh_set_estimator_reweighting_auto): in every
    // round c2 = kappa^2 * the lower median of the label's squared transfer errors under the model that stands, kept inside
    // [DBL_MIN, the labeling's truncation threshold thr_hom^2 * 81 / 16 — beyond it the labeling would not have assigned the member].
    // kappa = 0: kappa^2 = log2(100) — for two-dimensional Gaussian residuals d2 / sigma^2 is chi-squared with two degrees of
    // freedom, median 2 ln 2 and 0.99 quantile 2 ln 100, so the default cuts where 1 % of a clean label's members lie.  With
    // c2_min = DBL_MIN a label whose median error is 0 weighs only its exact fits, and keeps its model when they are fewer than
    // four or reproduce it.  0 (default) off; rounds in [1, 16]; kappa finite and >= 0.  Asking for a fixed and a self-scaled
    // final refit, or for both estimator settings, makes Process() fail with a message, as any other value does.
    void SetModelReweightAuto(int rounds, double kappa = 0) { model_reweight_auto = rounds; model_reweight_kappa = kappa; }
    void SetEstimatorReweightAuto(int rounds, double kappa = 0) { estimator_reweight_auto = rounds; estimator_reweight_kappa = kappa; }
    // How ProposeModels ranks the hypotheses of a batch — the initial batch, the iterative ones and the sharded route alike:
    // SELECTION_SCORE_COUNT (default) by inlier count (mh_select_greedy), SELECTION_SCORE_MSAC by the MSAC weight among the
    // hypotheses with at least min_inliers-or-8 inliers (mh_select_greedy_msac, include/multih_hip.h: the count makes a hypothesis
    // eligible, the fit decides; a refit replaces its hypothesis when it weighs at least as much).  INIT_STABLE_SETS proposes
    // nothing and ignores it; independent of SetTailScore.  Any other value makes Process() fail with a message.
    enum { SELECTION_SCORE_COUNT = 0, SELECTION_SCORE_MSAC = 1 };
    void SetSelectionScore(int s) { selection_score = s; }
    // The sampler of the proposal batches (the initial one and the iterative ones): uniform 4-tuples (default), or
    // neighbourhood-guided ones (mh_set_sampler, MH_SAMPLER_LOCAL): the first index uniform, the other three from its `k`
    // nearest neighbours in (x1, y1, x2, y2), with `uniform_per_16` hypotheses of every 16 left uniform (a homography from a
    // small patch extrapolates poorly: DESIGN.md 3.3).  Process() builds the sampler's table once, on the refined
    // correspondences, after the front half.  The degenerate tail's batch stays uniform; INIT_STABLE_SETS ignores the setting.
    enum { PROPOSAL_UNIFORM = 0, PROPOSAL_LOCAL = 1 };
    void SetProposalSampler(int sampler, int k = 32, int uniform_per_16 = 4)
    {
        proposal_sampler = sampler; proposal_sampler_k = k; proposal_uniform_per_16 = uniform_per_16;
    }
    // Where the INITIAL batch of ProposeModels comes from: PROPOSAL_SOURCE_DLT (default) — `hypotheses` 4-point DLT hypotheses from
    // sampled tuples — or PROPOSAL_SOURCE_HAF (mh_propose_haf, include/multih_hip.h): one hypothesis per `stride`-th refined
    // correspondence from its affinity and F (the reference's minimal solver, GetHomographyHAF), refitted to the consistent ones
    // (within sqr_threshold_homography) among its `members` nearest neighbours; members = 0: the single correspondence.  The batch
    // has ceil(n / stride) hypotheses — SetProposal's count is ignored, and a log line says so — and is sharded, scored and selected
    // as a DLT batch is.  With members > 0 Process() builds the neighbour table once; if the local sampler is set as well the table
    // is the sampler's and members must not exceed its k.  The iterative batches and the degenerate tail stay DLT;
    // INIT_STABLE_SETS and SetInitialHomographies ignore the source; the point-only Process() refuses it (no affinities).
    // PROPOSAL_SOURCE_3PT (mh_propose_3pt): F-constrained 3-point hypotheses — the first three indices of the tuples the DLT route
    // would draw (the same counters, seeds and SetProposalSampler), fitted with F by GetHomography3PT without refinement.  The INITIAL
    // AND THE ITERATIVE batches come from it, with SetProposal's counts; members and stride are ignored.  It needs no affinities, so
    // the point-only Process() accepts it.  The degenerate tail stays DLT.
    enum { PROPOSAL_SOURCE_DLT = 0, PROPOSAL_SOURCE_HAF = 1, PROPOSAL_SOURCE_3PT = 2 };
    void SetProposalSource(int source, int members = 16, int stride = 1)
    {
        proposal_source = source; proposal_haf_members = members; proposal_haf_stride = stride;
    }
    // Multi-GPU propose stage (BASELINE configs[3] and [4]): one process per GPU, every rank holds all
    // correspondences and owns a contiguous shard of each hypothesis batch (the hypotheses are a pure function of
    // (seed, counter), so the union over ranks is the single-GPU batch).  In the first greedy round the ranks all-gather
    // their int32 inlier scores — north_star's exchange —, in every round one 88-byte record each (best score and its
    // position in the batch, that hypothesis' H), and run the same first-maximum selection on the device.  Labeling and re-estimation run replicated and deterministic, so the ranks stay
    // identical without a broadcast.  `fn` is the transport: it receives DEVICE pointers (the engine's resident score
    // buffer on the send side), so RCCL (`ncclAllGather`, or torch.distributed's all_gather_into_tensor as in
    // multi-h_amd/sharding.py) works on them in place: send `bytes_per_rank` bytes, receive world * bytes_per_rank in
    // rank order, return 0 once the result is complete in `recv_dev`.  The engine's stream is idle during the call.
    typedef int (*AllGatherFn)(void* ctx, const void* send_dev, void* recv_dev, unsigned long long bytes_per_rank);
    void SetSharding(int rank, int world, AllGatherFn fn, void* ctx);
    // The same with a STREAM-ORDERED transport: `fn` enqueues the all-gather on `hip_stream` (the engine's) and returns at
    // once — RCCL's ncclAllGather; include/multih_rccl.h + host/rccl_transport.cpp provide it (mhr_allgather) together with the communicator
    // bootstrap.  No host synchronisation and no Python in the exchange.  world == 1 with a transport runs the whole
    // sharded protocol on a one-rank communicator.
    typedef int (*StreamAllGatherFn)(void* ctx, const void* send_dev, void* recv_dev, unsigned long long bytes_per_rank,
                                     void* hip_stream);
    void SetShardingStream(int rank, int world, StreamAllGatherFn fn, void* ctx);
    // Number of 8-point hypotheses of the GPU F estimation used when SetEpipolarGeometry was not called.
    void SetFundamentalHypotheses(int n) { fundamental_hypotheses = n; }
    // r06: what the F estimation compares with threshold_fundamental_matrix — FUND_EPIPOLAR_MAX: the squared distance of a
    // point to the epipolar line of its partner, the larger of the two images, which is what the reference's
    // cv::findFundamentalMat(CV_FM_RANSAC, thr) thresholds (M/MultiH.cpp:775; OpenCV 3.1.0, restated); FUND_SAMPSON: the
    // Sampson distance (at most half of it at equal F — the build's definition until r05: at 2.6 px it let through what the
    // reference's call rejects from 1.84 px on).  include/multih_hip.h, mh_set_fundamental_metric.
    enum { FUND_SAMPSON = 0, FUND_EPIPOLAR_MAX = 1 };
    void SetFundamentalMetric(int m) { fundamental_metric = m; }
    // Which estimator the F estimation runs.  FUND_ESTIMATOR_LS8 (default): `fundamental_hypotheses` normalised 8-point
    // fits, the best-supported one refitted twice to its inliers (mh_estimate_fundamental).  FUND_ESTIMATOR_MINIMAL7: the
    // scheme of the reference's cv::findFundamentalMat(CV_FM_RANSAC, thr, 0.99) (M/MultiH.cpp:775, M/main.cpp:399-409): at
    // most max_samples minimal 7-point samples with up to three F each, the confidence stop, the best one returned WITHOUT
    // a refit (mh_estimate_fundamental_minimal; OpenCV's own draws and un-normalised arithmetic are not reproduced).
    // Any other mode makes Process() (and FilterCorrespondencesByEpipolarGeometry) fail with a message.
    enum { FUND_ESTIMATOR_LS8 = 0, FUND_ESTIMATOR_MINIMAL7 = 1 };
    struct FundEstimator { int mode = FUND_ESTIMATOR_LS8; int max_samples = 1000; double confidence = 0.99; };
    void SetFundamentalEstimator(int mode, int max_samples = 1000, double confidence = 0.99)
    {
        fundamental_estimator.mode = mode; fundamental_estimator.max_samples = max_samples; fundamental_estimator.confidence = confidence;
    }
    // r06: how many correspondences each stage of GetFundamentalMatrixAndRefineData (M/MultiH.cpp:770-848) let through in
    // the last Process(): the input, the RANSAC mask (:809), OptimalTriangulation (:815-817), distanceError <= 1 (:826).
    // All equal to the input when the caller supplied F (SetEpipolarGeometry): the points are then taken as they are.
    struct FrontStages { int input = 0, in_ransac_mask = 0, triangulated = 0, affine_consistent = 0; };
    FrontStages GetFrontStages() const { return front_stages; }
    // The post-filter of Process() (HomographyCompatibilityCheck, M/MultiH.cpp:78-86) can be switched off to look at
    // what the merge <-> label loop itself produced (parity tests against the oracle of that loop).
    void SetCompatibilityCheck(bool on) { run_compatibility_check = on; }
    // What the trials of the post-filter fit.  COMPAT_FIT_3PT (default): the reference's 3-point fits with F; nothing changes
    // anywhere, and the route without epipolar geometry skips the check.  COMPAT_FIT_DLT: multih::CompatibilityCheckDlt stands
    // where that check stood, on both routes: `trials` 4-point DLT trials per cluster on the engine (mh_compat_dlt_medians, seed
    // proposal_seed ^ 0xc0117a7), a cluster going when its statistic exceeds limit_scale * thr_hom^2.  limit_scale = 0 takes
    // COMPAT_DLT_LIMIT_SCALE, the measured statistic of a clean plane whose noise equals the inlier threshold.
    // SetCompatibilityCheck(false) switches either off; SetModelReweight* and SetModelPolish run on what the check kept.
    // Process() fails with a message for another mode, trials outside [1, 4096] or a limit_scale that is negative or not finite.
    enum { COMPAT_FIT_3PT = 0, COMPAT_FIT_DLT = 1 };
    static constexpr double COMPAT_DLT_LIMIT_SCALE = 256.0;
    void SetCompatibilityFit(int mode, int trials = 501, double limit_scale = 0.0)
    {
        compat_fit = mode; compat_trials = trials; compat_limit_scale = limit_scale;
    }
    // How MergingStep decides.  MERGE_MEAN_SHIFT (default): the reference's rule — mean shift over the models' 6-D features, a
    // rebuilt model per mode, the collinearity filter (M/MultiH.cpp:352-471); nothing changes anywhere.  MERGE_ENERGY: the PEARL
    // merge move.  While no LabelingStep has run in this Process() the models only pass the collinearity filter; afterwards the
    // step evaluates pairs of labels (all while there are at most 64 models, else each label's 8 nearest in the feature space)
    // with mh_merge_deltas, joins those whose union — with its own N-point DLT refit — LOWERS the labeling's energy
    // (multih::SelectMerges / ApplyMerges: best first, no label twice per step), runs the same filter (a filtered model's
    // members become outliers) and sets `changed` iff the model count changed.  The LabelingStep that follows starts warm from
    // that labeling.  Needs no F: it runs on the route with F and under SetEpipolarFree alike, replicated on every rank of a
    // sharded run.  Limits: the union's model is the N-point DLT whatever SetEstimator says (the next LabelingStep re-estimates
    // with the route's estimator); no joins of three labels at once; a cost per label only through SetLabelCost (default 0).  Any other value makes Process() fail.
    enum { MERGE_MEAN_SHIFT = 0, MERGE_ENERGY = 1 };
    void SetMergeMode(int m) { merge_mode = m; }
    // One record per MergingStep that evaluated merges in the last Process() (empty under MERGE_MEAN_SHIFT): E_before =
    // mh_labeling_energy in front of the merges, sum_delta the accepted deltas' sum, E_start = mh_labeling_energy of what the
    // LabelingStep starts from (= E_before + sum_delta when nothing was filtered), E_expansion the energy that step returned
    // (-1 when none followed).  Under SetLabelCost an accepted drop's delta is part of sum_delta (its details: GetDropLog).
    struct MergeLogRecord {
        long long iteration = 0, models_before = 0, pairs = 0, merges_accepted = 0, models_filtered = 0;
        long long E_before = 0, sum_delta = 0, E_start = 0, E_expansion = -1;
    };
    const std::vector<MergeLogRecord>& GetMergeLog() const { return merge_log; }
    // The cost of a label in use, for the moves of MergingStep under MERGE_ENERGY (PEARL's third term, beside data and
    // smoothness): beta = llround(points * round(lam * T)) energy units, i.e. stated in outliers' worth — a label must explain
    // about `points` correspondences better than the outlier label does to pay for itself.  Default 0: nothing changes.  With
    // beta > 0 a join is taken iff delta - beta < 0 (multih::SelectMergesWithLabelCost), and behind the joins, on the labeling and
    // models that result, mh_drop_deltas evaluates for every used label the move "give each member its best alternative among
    // the other used labels and the outlier label"; at most one drop per step, the one with the smallest (delta, label), iff
    // delta - beta < 0 (multih::SelectDrop / ApplyDrop).  The alpha-expansion itself stays without label costs.  A negative or
    // non-finite value, or a positive one without MERGE_ENERGY, makes Process() fail with a message.
    void SetLabelCost(double points) { label_cost_points = points; }
    // One record per MergingStep that evaluated drops in the last Process() (empty while the label cost is 0): the dropped
    // label in the numbering behind the joins (-1: none), its members and how many of them became outliers, delta and beta,
    // E_before = mh_labeling_energy in front of the drop, E_after a second mh_labeling_energy call behind it (= E_before + delta;
    // E_before when nothing was dropped).
    struct DropLogRecord {
        long long iteration = 0, candidates = 0, dropped = -1, members = 0, to_outlier = 0;
        long long delta = 0, beta = 0, E_before = 0, E_after = 0;
    };
    const std::vector<DropLogRecord>& GetDropLog() const { return drop_log; }
    void SetDevice(int d) { device = d; }
    // schedule knob of the engine (mh_set_tuning; results never depend on it), applied when the engine is created
    void SetEngineTuning(int key, int value) { engine_tuning.emplace_back(key, value); }
    void SetVerbose(bool v) { log_to_console = v; }
    double GetLastLoopSeconds() const { return loop_seconds; }
    // Which optional entry points the linked engine library has, one flag per mode that needs some (in brackets: the mh_*
    // functions behind it).  An engine library from before a mode lacks its flag: PlanRun refuses the mode with a message.
    struct EngineCaps {
        bool point_only = false;                  // (mh_set_estimator, mh_refine_points)
        bool fundamental_minimal = false;         // (mh_estimate_fundamental_minimal)
        bool set_sampler = false;                 // (mh_set_sampler)
        bool sample_neighbours = false;           // (mh_build_sample_neighbours)
        bool data_term = false;                   // (mh_set_data_term)
        bool residual_route = false;              // (mh_set_residual_mode, mh_set_residual_scope)
        bool msac_scores = false;                 // (mh_score_msac, mh_select_best_msac)
        bool get_model = false;                   // (mh_get_model)
        bool refit = false;                       // (mh_refit_homography)
        bool polish = false;                      // (mh_polish_homographies)
        bool reweight = false;                    // (mh_reweight_homographies)
        bool estimator_reweighting = false;       // (mh_set_estimator_reweighting)
        bool reweight_auto = false;               // (mh_reweight_homographies_auto)
        bool estimator_reweighting_auto = false;  // (mh_set_estimator_reweighting_auto)
        bool select_greedy_msac = false;          // (mh_select_greedy_msac)
        bool propose_haf = false;                 // (mh_propose_haf)
        bool propose_3pt = false;                 // (mh_propose_3pt)
        bool compat_dlt = false;                  // (mh_compat_dlt_medians)
        bool energy_merge = false;                // (mh_merge_deltas, mh_labeling_energy)
        bool drop_deltas = false;                 // (mh_drop_deltas)
        bool smoothness_weights = false;          // (mh_set_smoothness_weights)
    };
    // What one Process() call derives from the settings, made by PlanRun before anything touches an engine.
    struct RunPlan {
        bool points_only = false;                 // the point-only Process()
        int est = 0;                              // the engine's re-estimator, MH_ESTIMATOR_*
        // where the initial and the iterative batches of ProposeModels come from, PROPOSAL_SOURCE_*
        int initial_source = PROPOSAL_SOURCE_DLT, iterative_source = PROPOSAL_SOURCE_DLT;
        // known once the front half has said how many correspondences are left: the batches use the local sampler (its table
        // is on the engine); the members of a HAF hypothesis (reduced where there are fewer correspondences)
        bool proposal_local = false;
        int haf_members = 0;
        long long label_cost_beta = 0;            // SetLabelCost in energy units
        int residual_mode = 0, residual_scope = 0;          // MH_RESIDUAL_*, MH_RESIDUAL_SCOPE_*
        int smoothness_rule = 0, smoothness_q_max = 1;      // MH_SMOOTH_*; rho and q_max as the engine gets them (0 and 1 under UNIFORM)
        double smoothness_rho = 0.0;
        // the reweighted rounds of the loop's estimator: 0 unless est is the N-point DLT; c2 is the fixed rule's squared scale
        int estimator_reweight_rounds = 0;
        double estimator_reweight_c2 = 0.0;
        bool estimator_reweight_auto = false;     // the rounds are self-scaled ones
    };

protected:
    std::vector<cv::Point2d> src_points_original, dst_points_original;   // M/MultiH.h:78
    std::vector<cv::Point2d> src_points, dst_points;                     // :79
    std::vector<cv::Mat> affinities_original, affinities;                // :80
    double fundamental_matrix[9];
    double epipole_2[2];
    bool have_epipolar = false;
    bool log_to_console = false;
    bool degenerate_case = false;
    double final_energy = 0.0;
    std::vector<std::vector<int>> neighbours;                            // :86 (trainIdx only)
    std::vector<cv::Mat> cluster_homographies;                           // :87
    std::vector<int> labeling;                                           // :88
    int minimum_inlier_number;
    double threshold_fundamental_matrix;
    double threshold_homography, sqr_threshold_homography;
    double locality_lambda, energy_lambda;
    double affine_threshold, straightness_threshold;
    int final_iteration_number = 0;

    // engine state
    mh_engine* engine = nullptr;
    int device = 0;
    std::vector<std::pair<int, int>> engine_tuning;
    enum { NEIGHBOURS_KNN = 0, NEIGHBOURS_RADIUS = 1, NEIGHBOURS_APPROX = 2 };
    int approx_trees = 4, approx_checks = 32;
    uint64_t approx_seed = 0;
    int neighbour_mode = NEIGHBOURS_KNN;
    int knn = 16;
    double neighbour_radius = 0.0;
    long long neighbour_max_hits = 1ll << 28;
    uint64_t proposal_seed = 1234;
    int proposal_hypotheses = 10000;
    int proposal_max_models = 32;
    bool proposal_refit = true;
    int estimator = ESTIMATOR_HAF;
    bool epipolar_free = false;
    int data_term = DATA_TERM_REFERENCE;
    int residual = RESIDUAL_FORWARD;
    int smoothness_rule = SMOOTHNESS_UNIFORM, smoothness_q_max = 16;      // SetSmoothnessWeights
    double smoothness_rho = 0.0;
    int tail_score = TAIL_SCORE_COUNT;
    int tail_refit = 0;
    int tail_polish = 0, model_polish = 0;
    int model_reweight = 0, estimator_reweight = 0;
    double model_reweight_scale = 0.0, estimator_reweight_scale = 0.0;
    int model_reweight_auto = 0, estimator_reweight_auto = 0;
    double model_reweight_kappa = 0.0, estimator_reweight_kappa = 0.0;
    // the self-scaled rule's numbers: kappa^2 (kappa = 0: log2(100), the nearest double) and the upper bound of c2
    static double AutoKappa2(double kappa) { return kappa > 0.0 ? kappa * kappa : 6.643856189774724; }
    double AutoScaleMax() const { return threshold_homography * threshold_homography * 81.0 / 16.0; }
    int selection_score = SELECTION_SCORE_COUNT;
    int proposal_sampler = PROPOSAL_UNIFORM, proposal_sampler_k = 32, proposal_uniform_per_16 = 4;
    bool ApplyProposalSampler(bool local);
    int proposal_source = PROPOSAL_SOURCE_DLT, proposal_haf_members = 16, proposal_haf_stride = 1;
    RunPlan plan;                         // of the last Process()
    EngineCaps caps;                      // of the engine library that Process() ran against
    int fixed_iterations = 0;
    int iter_hypotheses = 0, iter_max_new = 4;
    int fundamental_hypotheses = 4000;
    int fundamental_metric = FUND_EPIPOLAR_MAX;
    FundEstimator fundamental_estimator;
    FrontStages front_stages;
    int init_mode = INIT_DLT;
    bool run_compatibility_check = true;
    int compat_fit = COMPAT_FIT_3PT, compat_trials = 501;      // SetCompatibilityFit
    double compat_limit_scale = 0.0;
    bool post_filter_failed = false;             // the engine's part of HomographyCompatibilityCheck returned an error
    uint64_t merge_rng_counter = 0;
    double loop_seconds = 0.0;
    int labeling_steps_run = 0;
    std::vector<cv::Mat> initial_homographies;
    int shard_rank = 0, shard_world = 1;
    AllGatherFn shard_allgather = nullptr;
    StreamAllGatherFn shard_stream_allgather = nullptr;
    void* shard_ctx = nullptr;

    // Process() with or without affinities, stage by stage: PlanRun, EnsureEngine, ConfigureEngine, UploadCorrespondences,
    // FrontHalf, BuildProposalTables, InitialModels, ClusterMergingAndLabeling, PostFilter, Finish
    bool Run(bool points_only);
    bool PlanRun(bool points_only, const EngineCaps& have, RunPlan& out, std::string& error) const;
    bool PlanFinishModes(const EngineCaps& have, RunPlan& out, std::string& error) const;      // PlanRun's second half
    bool EnsureEngine();
    bool ConfigureEngine(const RunPlan& p);                // the sticky settings of the engine, every one on every call
    bool UploadCorrespondences(const std::vector<cv::Point2d>& src, const std::vector<cv::Point2d>& dst, const std::vector<cv::Mat>& aff);
    struct StageClock;                                     // the "... done" lines under MULTIH_TIMING
    bool FrontHalf();                                      // M/MultiH.cpp:770-848; may end in degenerate_case
    bool RefineData(const std::vector<unsigned char>& mask);                                   // :807-838
    bool BuildProposalTables(const StageClock& stage);
    bool InitialModels();
    bool PostFilter();                                     // :78-86
    bool Finish();                                         // :88-94, or the final models' reweighted refit and polish
    std::vector<double> FlatModels() const;                // cluster_homographies, 9 doubles each
    bool UploadModels();
    bool DownloadModels(int count);
    bool ProposeInitialModels();          // north_star propose: DLT batch + greedy selection
    bool EstablishStablePointSets();      // M/MultiH.cpp:604-694 (with ComputeLocalHomographies :696-717)
    // `source`: what the batch is made of (PROPOSAL_SOURCE_*: RunPlan's initial_source or iterative_source)
    bool ProposeModels(int source, uint64_t seed, long long first, int hypotheses, int max_models,
                       std::vector<unsigned char>& mask);
    void ClusterMergingAndLabeling();     // M/MultiH.cpp:224-312
    bool BuildNeighbourhood();            // :233-253
    bool MergingStep(bool& changed);      // :352-471
    bool MergingStepEnergy(bool& changed);             // SetMergeMode(MERGE_ENERGY)
    int merge_mode = MERGE_MEAN_SHIFT;
    std::vector<MergeLogRecord> merge_log;
    double label_cost_points = 0.0;       // SetLabelCost
    std::vector<DropLogRecord> drop_log;
    bool labeling_is_current = false;     // a LabelingStep has run in this Process() and `labeling` is valid for cluster_homographies
    bool merge_log_open = false;          // the last record waits for its LabelingStep's energy
    int loop_iteration = 0;
    bool LabelingStep(double& energy, bool changed);   // :513-602
    void ComputeInliersOfHomography(int idx);          // :743-768
    void HandleDegenerateCase();                       // :719-741 (single best DLT model)
    bool PolishTailModel(double H[9]);                 // SetTailPolish: the tail's model over its labelled inliers
};

namespace multih {
// r06: the load-time filter of the reference's CALLER — LoadPointsFromFile, M/main.cpp:399-409:
//     findFundamentalMat(srcPoints, dstPoints, CV_FM_RANSAC, 2.0, 0.99, mask);   then every row with mask[i] == 0 is erased
// — through the engine's own estimator (mh_estimate_fundamental: `hypotheses` normalised 8-point fits from counter-RNG
// 8-tuples, the best-supported one refitted twice to its inliers; cv::findFundamentalMat itself — 7-point samples, at most
// 1 000 of them, its own RNG, no refit — is outside /root/reference and not reproduced).  `metric` as
// MultiH::SetFundamentalMetric.  Erases the rejected rows from all three vectors (order kept, as the reference's backward
// erase loop keeps it) and returns false — leaving them untouched — when there are fewer than 8 rows, the sizes differ or the
// engine fails.  mask_out (nullable): one flag per INPUT row.  `estimator` as MultiH::SetFundamentalEstimator: with
// FUND_ESTIMATOR_MINIMAL7 the filter runs the caller's own scheme (7-point samples, confidence stop, no refit) and
// `hypotheses` is not used.
bool FilterCorrespondencesByEpipolarGeometry(std::vector<cv::Point2d>& srcPoints, std::vector<cv::Point2d>& dstPoints,
                                             std::vector<cv::Mat>& affines, double threshold = 2.0,
                                             uint64_t seed = 1234, int hypotheses = 4000,
                                             int metric = MultiH::FUND_EPIPOLAR_MAX, int device = 0,
                                             std::vector<unsigned char>* mask_out = nullptr,
                                             const MultiH::FundEstimator& estimator = MultiH::FundEstimator());
}
