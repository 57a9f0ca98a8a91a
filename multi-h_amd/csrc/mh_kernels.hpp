// mh_kernels.hpp — private launch interface between the C-ABI layer (capi*.hip)
// and the gfx950 kernels.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mh {

// Correspondences resident in HBM as struct-of-arrays (coalesced 16-B loads).
struct Points {
    const double* x1;
    const double* y1;
    const double* x2;
    const double* y2;
    int n;
    // bounding box of the source points (x1, y1), taken when the correspondences were set; NaN when unknown.  The
    // residual sweep uses it to prove, per model, that the projective denominator stays away from zero.
    double xmin, xmax, ymin, ymax;
};

struct Affines {            // a11 a12 a21 a22, SoA
    const double* a11;
    const double* a12;
    const double* a21;
    const double* a22;
};

struct Epipolar {           // passed by value to kernels
    double F[9];
    double ex, ey;
};

// Leading dimension (in doubles) of the residual matrix rows: rows start 128-B aligned.
inline long long residual_ld(int n) { return ((long long)n + 15) & ~15ll; }

// --- residual.hip -----------------------------------------------------------
// How a sweep is laid out on the chip; the defaults are the launcher's own choices.
struct SweepLaunch {
    int slices = 0;                 // point slices; 0 = the launcher's rule
    bool contiguous = false;        // with slices > 0 (tuning): each slice a contiguous run of tiles instead of every slices-th tile
    int swapxy = 0;                 // tuning: the slice index as the fastest grid dimension
    bool counts_zeroed = false;     // the caller has cleared counts already
    int resident_grid = 0;          // > 0: that many workgroups walk the work items as a resident grid (needs resident_ctl) ...
    int* resident_ctl = nullptr;    // ... through these two ints, zero between launches
    int slice_major = 0;            // resident grid: consecutive items = the slices of one model block
};
// variant: 0 default; tuning knob for bench sweeps (see residual.hip).
hipError_t launch_residual(const Points& p, const double* H, int M, double thr2, double* R,
                           long long ldr, int* counts, int variant, hipStream_t s, const SweepLaunch& how);
// workgroups of the product's materialising sweep that one compute unit holds at a time (occupancy query)
int residual_workgroups_per_cu();
hipError_t launch_score(const Points& p, const double* H, int M, double thr2,
                        const unsigned char* mask, int* counts, int variant, hipStream_t s);
// --- score32.hip: the same counts through an FP32 pre-test with a rigorous error bound (pretest32.hpp; FP64 only for the pairs it cannot decide)
hipError_t launch_model32(const double* H, int M, double X, double Y, double Cmax, float* H32 /* M x 16 */, hipStream_t s);
// Cmax: the bound on |x2|, |y2| the table was made with; thr2 in [2^-40, 2^40]
hipError_t launch_score32(const Points& p, const double* H, const float* H32, int M, double thr2, double Cmax, const unsigned char* mask,
                          int* counts, unsigned long long* fallback_pairs, int tiling, hipStream_t s, int* resident_ctl = nullptr,
                          int cu_count = 256, int resident_slices = 0, int* occ_cache = nullptr);
// the materialised int32 cost matrix (launch_cost_matrix, datacost.hip) through the same pre-test; H32 made with the same Cmax
hipError_t launch_cost32(const Points& p, const double* H, const float* H32, int M, double lambda, double thr2, double Cmax,
                         int* C, long long ldc, int* counts, hipStream_t s, int* resident_ctl = nullptr, int cu_count = 256,
                         int psplit_override = 0, int slice_major = 0, int batched = 0, int* occ_cache = nullptr, int rising = 0);
// --- msac32.hip: per model the inlier count AND the sum of the inliers' MSAC gains (include/multih_hip.h, mh_score_msac) —
// launch_msac32 behind the same pre-test (same H32 / Cmax / thr2 preconditions as launch_score32; fp64_pairs, nullable:
// device counter of the pairs that went through the FP64 formula), launch_msac64 with every pair in FP64
hipError_t launch_msac32(const Points& p, const double* H, const float* H32, int M, double thr2, double Cmax, const unsigned char* mask,
                         int* counts, int* weights, unsigned long long* fp64_pairs, hipStream_t s);
hipError_t launch_msac64(const Points& p, const double* H, int M, double thr2, const unsigned char* mask, int* counts, int* weights,
                         hipStream_t s);
// occ_cache (both launchers): the caller's per-engine cache of the resident kernel's workgroups per compute unit (-1 = not asked yet)
// symmetric (both, and the two launchers of datacost.hip): 0 the forward transfer error, 1 the symmetric one — the engine's
// route_symmetric() (capi_engine.hpp, mh_set_residual_scope)
hipError_t launch_inliers_of_model(const Points& p, const double* H, int idx, double thr2,
                                   int label_value, int* labels, hipStream_t s, int symmetric = 0);
hipError_t launch_moments(const Points& p, const double* H, int M, double thr2, double* moments,
                          double* min_eig, hipStream_t s, int symmetric = 0);

// --- compat.hip: order statistics of the post-filter's trials (HomographyCompatibilityCheck, M/MultiH.cpp:128-196)
hipError_t launch_compat_select(const double* pts /* total x 4 */, const int* begin /* clusters + 1 */, int clusters,
                                const int* tri /* clusters x trials x 3 */, const double* H /* clusters x trials x 9 */,
                                const unsigned char* ok, int trials, double* out /* clusters x trials x 8 */, hipStream_t s);
// the trials' 3-point homographies (GetHomography3PT without refinement, M/MultiH.cpp:154) — H: 9 doubles per (cluster, trial), ok: 1 where finite
hipError_t launch_compat_fit(const double* pts, const int* begin, int clusters, const int* tri, const double F[9], int trials,
                             double* H, unsigned char* ok, hipStream_t s);
// the check without F (mh_compat_dlt_medians): per (cluster, trial) the key at rank (rest - 1) / 2 of the forward transfer errors
// of the cluster's points that are none of the trial's four (idx: positions in the packed structure-of-arrays points, as
// launch_dlt4_segments writes them), NaN -> +inf; then per cluster the value at rank (trials - 1) / 2 of its trial values
hipError_t launch_compat_median4(const double* x1, const double* y1, const double* x2, const double* y2, const int* begin /* clusters + 1 */,
                                 int clusters, const int* idx /* clusters x trials x 4 */, const double* H /* clusters x trials x 9 */,
                                 int trials, double* trial_out /* clusters x trials */, hipStream_t s);
hipError_t launch_compat_cluster_median(const double* trial /* clusters x trials */, int clusters, int trials,
                                        double* medians_out /* clusters */, hipStream_t s);

// --- dlt4.hip ---------------------------------------------------------------
// local.nbr != null: the neighbourhood-guided sampler (dlt4.hip, sample4_by) over the n x k table nbr, every entry in [0, n)
struct Dlt4Local { const int* nbr = nullptr; int k = 0; int uniform_per_16 = 0; };
hipError_t launch_dlt4(const Points& p, unsigned long long seed, long long first, int M,
                       int* idx_out, double* H_out, hipStream_t s, int variant = 0 /* 1: the LDS-staged form */,
                       Dlt4Local local = Dlt4Local{});
// the register form under the segment sampler (mh_sampler.hpp): M = segments x trials hypotheses over packed points, hypothesis m
// draws inside segment m / trials = [begin[m / trials], begin[m / trials + 1]); idx_out: M x 4 positions in the packed arrays
hipError_t launch_dlt4_segments(const double* x1, const double* y1, const double* x2, const double* y2, int total, const int* begin,
                                int trials, unsigned long long seed, long long first, int M, int* idx_out, double* H_out,
                                hipStream_t s);

hipError_t launch_fund8(const Points& p, unsigned long long seed, long long first, int M,
                        int* idx_out /* M x 8 */, double* F_out, hipStream_t s);

// 7-point minimal samples: up to three F per sample, F_out[(m*3 + j)*9 ..] (the finite ones first, then quiet NaNs)
hipError_t launch_fund7(const Points& p, unsigned long long seed, long long first, int M,
                        int* idx_out /* M x 7 */, double* F_out /* 3M x 9 */, int* nvalid_out /* M */, hipStream_t s);

// --- fund.hip ---------------------------------------------------------------
// The stop rule of a sequential RANSAC over 7-point samples, replayed on the counts of S samples scored whole (3 slots each,
// sample order; one workgroup).  out[4]: winning slot index, its count, samples used, valid slots among the samples used.
// F_win (nullable): receives the winning slot's nine doubles of F.
hipError_t launch_ransac_stop(const int* counts /* 3S */, const int* nvalid /* S */, int S, int n, double confidence,
                              const double* F /* 3S x 9 */, double* F_win, int* out, hipStream_t s);
// inlier flags (n bytes) and inlier count of one F on the device: pass 1 of launch_fund_refit without the refit
hipError_t launch_fund_mask(const Points& p, const double* F_in, double thr2, unsigned char* mask_out, int* count,
                            hipStream_t s, int metric);
// metric: MH_FUND_SAMPSON (0) or MH_FUND_EPIPOLAR_MAX (1), see fund.hip
hipError_t launch_sampson_score(const Points& p, const double* F, int M, double thr2, int* counts,
                                hipStream_t s, int metric);
// Least-squares 8-point refit of F on the inliers of F_in under `metric` (one workgroup).
hipError_t launch_fund_refit(const Points& p, const double* F_in, double thr2, double* F_out,
                             unsigned char* mask_out, int* count_out, hipStream_t s, int metric);

// --- refit_h.hip: one homography refitted to its inliers, every round inside one launch (mh_refit_homography) ---
// H_in, H_out: 9 doubles each on the device; mask_out: p.n bytes; out_i[2]: inliers of H_out, fits accepted
constexpr int REFIT_H_MAX_ITERATIONS = 16;
hipError_t launch_refit_h(const Points& p, const double* H_in, double thr2, int iterations, double* H_out,
                          unsigned char* mask_out, int* out_i, hipStream_t s);

// --- polish_h.hip: Levenberg-Marquardt polish of one homography per label, every iteration inside one launch of one workgroup
// per model (mh_polish_homographies) ---
// labels: p.n ints on the device; H_in, H_out: m x 9 doubles; cost: m x 2 doubles (S before, S after); info: m x 4 ints
// (members, iterations run, steps accepted, status), all on the device
constexpr int POLISH_H_MAX_ITERATIONS = 32;
constexpr int POLISH_H_MAX_MODELS = 65536;
hipError_t launch_polish_h(const Points& p, const int* labels, const double* H_in, int m, int max_iterations, double* H_out,
                           double* cost, int* info, hipStream_t s);

// --- reweight_h.hip: iteratively reweighted N-point DLT refits, one homography per label, every round inside one launch of one
// workgroup per model (mh_reweight_homographies; the MH_ESTIMATOR_DLT re-estimator under mh_set_estimator_reweighting) ---
// labels: p.n ints on the device; H_in, H_out: m x 9 doubles (may be the same array); gain: m x 2 doubles (W of H_in, W of
// H_out); info: m x 4 ints (members, support of H_out, rounds done, status); counts: m ints (members) — the last three nullable
constexpr int REWEIGHT_H_MAX_ROUNDS = 16;
constexpr int REWEIGHT_H_MAX_MODELS = 65536;     // of a call of mh_reweight_homographies
hipError_t launch_reweight_h(const Points& p, const int* labels, const double* H_in, int m, double c2, int rounds, double* H_out,
                             double* gain, int* info, int* counts, hipStream_t s);

// --- label_scale.hip: per label, one order statistic of its members' forward transfer errors (mh_label_residual_quantile), and
// the reweighted rounds of reweight_h.hip with c2 = clamp(kappa2 * that statistic under the model that stands) re-estimated in
// every round, all rounds in one launch (mh_reweight_homographies_auto; the MH_ESTIMATOR_DLT re-estimator under
// mh_set_estimator_reweighting_auto).  One workgroup per model ---
constexpr int LABEL_QUANTILE_MAX_DEN = 65536;
struct AutoScale { int num, den; double kappa2, c2_min, c2_max; };          // rank ((c - 1) * num) / den; c2 in [c2_min, c2_max]
bool autoscale_ok(const AutoScale& a);           // num / den in range, kappa2 finite and > 0, 0 < c2_min <= c2_max finite
// labels: p.n ints on the device; H: m x 9 doubles; d2_out: m doubles; info: m x 4 ints (members, rank, members strictly below
// the value, status), nullable
hipError_t launch_label_quantile(const Points& p, const int* labels, const double* H, int m, int num, int den, double* d2_out,
                                 int* info, hipStream_t s);
// as launch_reweight_h; scale: m x 2 doubles (c2 under H_in, c2 under H_out), nullable
hipError_t launch_autoscale_reweight_h(const Points& p, const int* labels, const double* H_in, int m, const AutoScale& a, int rounds,
                                       double* H_out, double* gain, double* scale, int* info, int* counts, hipStream_t s);

// --- datacost.hip -----------------------------------------------------------
// the data cost of every model against every point, int32, model-major with pitch ldc (datacost.hip)
inline long long cost_ld(int n) { return ((long long)n + 31) & ~31ll; }
// rising (here and in launch_cost32): 0 the reference's data term, 1 MH_DATA_TERM_RISING (include/multih_hip.h)
hipError_t launch_cost_matrix(const Points& p, const double* H, int M, double lambda, double thr2, int* C, long long ldc,
                              int* counts, hipStream_t s, int rising = 0, int symmetric = 0);
hipError_t launch_data_cost(const Points& p, const double* H, int Nh, double lambda, double thr2,
                            int* cost, hipStream_t s, int rising = 0, int symmetric = 0);

// --- reestimate.hip ---------------------------------------------------------
hipError_t launch_reestimate(const Points& p, const Affines& a, const int* labels, int Nh,
                             const Epipolar& ep, double* H, int* counts, hipStream_t s);

// --- reestimate3pt.hip: the point-only re-estimator (GetHomography3PT without refinement over every label's members) ---
// scratch: reestimate_3pt_scratch_ints(p.n, Nh) ints (member lists and their offsets); a label with < 3 members or a fit that
// is not finite keeps its H; counts (nullable): member count per label
size_t reestimate_3pt_scratch_ints(int n, int Nh);
// form: 0 by size (the product's rule), 1 the match loop over the whole label array (scratch unused), 2 the compacted member lists
hipError_t launch_reestimate_3pt(const Points& p, const int* labels, int Nh, const Epipolar& ep, double* H, int* counts,
                                 int* scratch, hipStream_t s, int form = 0);

// --- reestimate_dlt.hip: the re-estimator without epipolar geometry (the normalised N-point DLT over every label's members) ---
// H[k] = fit(S_k) of mh_refit_homography's rule, the members found by the match loop (part of the definition of the sums'
// order); a label with < 4 members or a fit that is not finite keeps its H; counts (nullable): member count per label
hipError_t launch_reestimate_dlt(const Points& p, const int* labels, int Nh, double* H, int* counts, hipStream_t s);

hipError_t launch_haf_point(const Points& p, const Affines& a, const Epipolar& ep, double locality,
                            double* H_out /* n x 9, nullable */, double* feat_out /* n x 10, nullable */,
                            hipStream_t s);

// --- haf_propose.hip: one hypothesis per affine correspondence (mh_propose_haf) ---
// hypothesis s: anchor (first + s) * stride, the caller has checked the range; nbr: the n x k sampling table (null with
// members == 0), of which the first `members` columns are read; used_out: per hypothesis the mask of consistent neighbours
hipError_t launch_haf_propose(const Points& p, const Affines& a, const Epipolar& ep, const int* nbr, int k, int members,
                              double thr2, long long first, int m, int stride, double* H_out, unsigned* used_out, hipStream_t s);

// --- propose3pt.hip: F-constrained 3-point hypotheses (mh_propose_3pt) ---
// hypothesis s: the first three indices of the sampler's 4-tuple for counter first + s (local as for launch_dlt4) and
// GetHomography3PT without refinement on them; idx_out: M x 4 (the fourth column is -1); a fit that fails stores nine quiet NaNs
hipError_t launch_propose_3pt(const Points& p, const double F[9], unsigned long long seed, long long first, int M,
                              int* idx_out, double* H_out, hipStream_t s, Dlt4Local local = Dlt4Local{});

// --- refine.hip -------------------------------------------------------------
// points_only: step 1 alone (no affinity is read, a may be null), out is n x 4 (x1 y1 x2 y2) and every triangulated row is kept
hipError_t launch_refine_points(const Points& p, const Affines& a, const double F[9], const double e1[2],
                                const double e2[2], const unsigned char* in_mask, unsigned char* keep,
                                double* out /* n x 8, points_only: n x 4 */, unsigned char* reason /* n: MH_REFINE_* */, hipStream_t s,
                                int points_only = 0);

// --- meanshift.hip ----------------------------------------------------------
constexpr int MS_BATCH = 256;   // climbs per batch: part of the definition of the seed order (meanshift.hip; the oracle draws alike)
struct MeanShiftWork {      // every per-climb array holds MS_BATCH slices
    const double* data;      // n x d row-major
    int n, d;
    double* mean;            // [climb] 16      current mean (in/out)
    int* votes;              // [climb] n       votes of the running climb (members get +1 per iteration)
    int* out;                // [climb] 4       [0] iterations, [1] converged, [2] list length, [3] dead end (no member)
    int* list;               // [climb] 2*n     (index, votes) pairs compacted when the climb has ended
    double* partial;         // [climb] MS_GROUPS x 16 member sums of the running iteration
    int* partial_cnt;        // [climb] MS_GROUPS
};
struct MeanShiftResultBlock { int out[4]; double mean[16]; };
struct MeanShiftActive { unsigned char climb[MS_BATCH]; };       // the climbs a round still works on, passed by value
// The climbs active[0..n_active) side by side without host round trips in between: seed the means with the rows
// starts_dev[climb] (null: continue the running climbs), `iterations` climb iterations (no-ops for a climb that has
// ended), compact the votes of the climbs that have ended into their lists, then publish
// every active climb's control words and mean to result_dev[climb] (mapped pinned).  Workgroups beyond the rows
// (n < 256 * MS_GROUPS) are not launched: their partial sums are +0, which the running sum never notices.
hipError_t launch_ms_climb(const MeanShiftWork& w, const MeanShiftActive& active, int n_active, const int* starts_dev, double band_sq,
                           double stop_thresh, int iterations, MeanShiftResultBlock* result_dev,
                           int* tickets /* MS_BATCH ints, zero */, hipStream_t s);
// r05: the same for the FEW climbs that are still running after the first rounds — to their end (or max_iters) in one
// launch, one workgroup per group of the definition with the thread's rows in registers and a barrier of the climb's own
// per iteration (meanshift.hip, k_ms_persist); a climb whose workgroups were not all resident within 250 ms leaves
// untouched with fell_back (ctl[2 * MS_BATCH + climb]) set.  ctl: 3 x MS_BATCH ints; partial2: MS_BATCH x 2 x 64 x 16
// doubles; partial_cnt2: MS_BATCH x 2 x 64 ints.  Needs n_active x min(64, ceil(n / 256)) workgroups resident at once.
hipError_t launch_ms_persist(const MeanShiftWork& w, const MeanShiftActive& active, int n_active, double band_sq, double stop_thresh,
                             int max_iters, int* ctl, double* partial2, int* partial_cnt2, MeanShiftResultBlock* result_dev,
                             hipStream_t s, unsigned long long* ticks = nullptr);
bool ms_persist_supported(int n, int d);
int ms_persist_occupancy(int d);
// r05: a climb per workgroup, from seed to published result in one launch; the rows reached through a one-coordinate index
// (meanshift.hip, k_ms_indexed).  The index is built once per call; cell width w >= bandWidth^2 (1 + 2^-20) is the caller's
// duty (the three-cell window is exact only then).
struct MeanShiftIndex {
    const double* rs;        // [d][n] the rows in cell order, component-major
    const int* order;        // [n] position in cell order -> row
    const int* cell_start;   // [cells + 1]
    int cells, coord;
    double lo, inv_w;        // cell(x) = clamp(floor((x - lo) * inv_w), 0, cells - 1)
};
bool ms_indexed_supported(int n, int d);
int ms_index_max_cells();
hipError_t launch_ms_index_build(const double* data, int n, int d, const MeanShiftIndex& ix, int* count, int* cursor, int* cell_start,
                                 int* order, double* rs, hipStream_t s);
hipError_t launch_ms_indexed(const MeanShiftWork& w, const MeanShiftActive& active, int n_active, const int* starts_dev,
                             const MeanShiftIndex& ix, double band_sq, double stop_thresh, int max_iters, int dense_limit,
                             int keep, int* running, MeanShiftResultBlock* result_dev, hipStream_t s,
                             unsigned long long* ticks = nullptr);
// the lists of climbs 0 .. climbs-1 packed one behind the other (lengths / offsets: `climbs` ints each, device-visible)
hipError_t launch_ms_pack(const MeanShiftWork& w, int climbs, int longest, const int* offsets_dev, const int* lengths_dev, int* packed,
                          hipStream_t s);
// compacts and clears the votes of all `climbs` climbs, ended or not
hipError_t launch_ms_collect(const MeanShiftWork& w, int climbs, hipStream_t s);

// --- expand.hip, expand_solve.hip ---------------------------------------------
struct Graph {              // symmetric weighted CSR in HBM
    const int* rowptr;      // n+1
    const int* col;         // nnz
    const int* w;           // nnz  multiplicity mult(i,j)
    const int* rev;         // nnz  index of the reverse arc
    int n, nnz;
    const int* order;       // n    a fixed pseudo-random permutation of the sites: the alpha-expansion's solver takes its
                            //      core sites in this order so that a workgroup never owns a spatial cluster (expand.hip)
    const int* wsum;        // n    sum of w over the site's row: bounds every n-link total of the site (expand.hip, k_move_setup)
};

// --- merge_energy.hip: the energy of a labeling, the energy change of joining two labels (mh_labeling_energy, mh_merge_deltas) ---
constexpr int MERGE_OK = 0, MERGE_EMPTY = 1, MERGE_NO_FIT = 2;       // MH_MERGE_*
// per pair: status; for an OK pair H_out (9 doubles) and out = { |S|, data_old, data_new, cut, delta }.  labels: n ints, any
// value; pairs: 0 <= a < b < Nh (the caller's check: they index H)
hipError_t launch_merge_pairs(const Points& p, const int* labels, const double* H, const int* pairs, int npairs, const Graph& g,
                              double lambda, double thr2, double* H_out, long long* out /* npairs x 5 */, int* status, hipStream_t s,
                              int rising, int symmetric);
// out[0] += data, out[1] += smooth (cleared by the caller).  labels: n ints in -1..Nh-1 (the caller's check: they index H)
hipError_t launch_labeling_energy(const Points& p, const int* labels, const double* H, const Graph& g, double lambda, double thr2,
                                  unsigned long long* out, hipStream_t s, int rising, int symmetric);

// --- label_cost.hip: every site's best alternative label, the energy change of dropping a label (mh_best_alternative, mh_drop_deltas) ---
constexpr int DROP_OK = 0, DROP_EMPTY = 1;       // MH_DROP_*
constexpr int BEST_ALT_TILE = 64;                // models per LDS tile of k_best_alternative
// per site: alt, alt_cost (nullable), own_cost (nullable).  labels: n ints in -1..Nh-1, used: Nh flags, used[labels[i]] != 0
// (the caller's check and count)
hipError_t launch_best_alternative(const Points& p, const int* labels, const double* H, int Nh, const int* used, double lambda,
                                   double thr2, int* alt, int* alt_cost, int* own_cost, hipStream_t s, int rising, int symmetric);
// per candidate: status; for an OK one out = { |S_k|, data_old, data_new, smooth_old, smooth_new }.  cand: labels in [0, Nh) (the
// caller's check: they index H); alt, alt_cost: launch_best_alternative's on the same labels
hipError_t launch_drop_labels(const Points& p, const int* labels, const double* H, const int* cand, int ncand, const int* alt,
                              const int* alt_cost, const Graph& g, double lambda, double thr2, long long* out /* ncand x 5 */,
                              int* status, hipStream_t s, int rising, int symmetric);

constexpr int EXPAND_MAX_CTX = 16;
constexpr int EXPAND_FLAG_WORDS = 896;     // device control block (expand_ctl.hpp)
constexpr int EXPAND_HOST_WORDS = 32;      // its head, mirrored to the host
constexpr int EXPAND_ACC_WORDS = 64 + 3 * 64 * 16;   // 16 scalars (mirrored to the host) + three striped sums
constexpr int EXPAND_CORE_SHARDS = 8;

// The schedule knobs of an expansion (see expand.hip and expand_solve.hip); do_expand sets every one.
struct ExpandTuning {
    // per-move solver: relaxation rounds per barrier interval, push cycles per push phase, push phases per global relabel,
    // workgroups of the solver launch
    int relax_rounds = 0, push_cycles = 0, push_phases = 0, solve_grid = 0, push_mult = 0;
    int reduce_rounds = 0;      // dominance-reduction rounds per launch; 0 switches the reduction off (A/B)
    int reduce_launches = 1;    // reduction launches per move in front of the solver: 2, or 1 (the compacting one alone)
    int cascade_iters = 0;      // barrier-separated passes of the dominance cascade inside the solver launch (0 = to its fixed point)
    // 100 MHz ticks a poll at a grid barrier may last before the launch gives up (a workgroup of it is not resident: a GPU
    // shared with other persistent launches); 0 = 3 s
    long long barrier_timeout_ticks = 0;
    long long barrier_first_timeout_ticks = 0;     // the launch's first barrier (residency of all its workgroups)
    int batch_min_labels = 0;   // batches from the first cycle on only when the label set has at least this many labels
    int batch_spw = 0;          // sites per wave in a batch's setup and reduction launches: 16 / 32 / 64, 0 = by the size of the launch (a move alone: 16)
};

// Test hook (mh_set_tuning key 40): the solve of context inject_ctx in the inject_group-th group of moves this expansion
// enqueues (a batch or a move alone, counted from 1) is marked failed (ERR_NO_CONVERGENCE) behind its k_solve; 0 = off
struct ExpandHooks { int inject_group = 0, inject_ctx = 0; };

// What the caller lends an expansion.  Everything optional is off (null) unless set.
struct ExpandWork {
    int* label = nullptr;       // n   current labeling (GCO numbering)
    int* cur_cost = nullptr;    // n   cost[i][label[i]]
    // The per-move state of one move in flight.  n_ctx >= 2: that many consecutive moves are solved together on the SAME
    // labeling, each in a context of its own, and committed in order by k_batch_commit (expand.hip, "batches").
    struct Ctx {
        int* cap;               // nnz capacities of the move's s-t graph
        int* sent;              // nnz cumulative flow per arc, written by the arc's tail only (expand_solve.hip)
        int* excess;            // n
        int* sink_cap;          // n
        int* height;            // n
        int* decided;           // n   0 undecided, 1 source side (takes alpha), 2 sink side (keeps its label), 3 not in the graph
        unsigned char* took;    // n   1 where the last solved move moves the site to alpha (applied lazily, see expand.hip)
        int* core;              // 8 x n  compacted list of the sites the dominance reduction left undecided, in 8 shards
        int* flags;             // device control words (EXPAND_FLAG_WORDS ints, expand_ctl.hpp)
        long long* acc;         // device 64-bit accumulators (EXPAND_ACC_WORDS)
        int* took_list;         // n   the sites the context's move takes (null: not kept; only batches walk it)
    };
    int n_ctx = 1;
    Ctx ctx[EXPAND_MAX_CTX] = {};
    int* h_flags = nullptr;         // pinned, device-mapped host mirror of context 0's flags (host address)
    long long* h_acc = nullptr;     // ... and of its accumulators
    int* h_flags_dev = nullptr;     // device addresses of the two mirrors
    long long* h_acc_dev = nullptr;
    int* bctl = nullptr;            // 8 + EXPAND_MAX_CTX   batch control words (device)
    int* h_batch = nullptr;         // 8   k_batch_commit's publication, pinned + device-mapped (host address) ...
    int* h_batch_dev = nullptr;     //     ... and its device address
    // flow recycling (expand_solve.hip): per label the net arc flows (L x nnz) and sink flows (L x n) its last
    // expansion ended with; null = every move starts from the zero flow
    int* saved_flow = nullptr;
    int* saved_sink = nullptr;
    int* trace = nullptr;           // 8 ints per move {core sites, workgroups, relabels, relax intervals, push phases,
    int trace_moves = 0;            //   barriers, ticks (100 MHz), ticks inside barriers}; moves beyond trace_moves are not traced
    int detail_move = -1;           // move whose global relabels are logged behind the trace (4 ints each, at most 2048): {active sites,
                                    //   largest finite height, relabel intervals so far, ticks so far}; -1 none
    // diagnostic (expand.hip, k_core_components): 16 ints per move for the first comp_moves moves; scratch 2 n ints
    int* comp_out = nullptr;
    int* comp_scratch = nullptr;
    int comp_moves = 0;
    ExpandTuning tune;
    ExpandHooks hooks;
};

struct ExpandStats {
    int cycles;
    long long energy;
    int moves, accepted;                      // moves enqueued; moves that lowered the energy
    long long push_phases, relax_intervals;   // summed over the moves that were solved
    long long host_syncs;
    long long reduce_launches, flow_moves;    // reduction launches; moves that still needed push-relabel
    long long launches;                       // kernel launches of the whole expansion
    long long moves_run;                      // moves not skipped as provably idempotent
    long long moves_solved;                   // of those, moves whose core was not empty (k_solve had work)
    long long core_sites, core_max;           // undecided sites handed to the solver: sum and maximum over moves
    long long barriers, outer_iterations;     // grid barriers / global relabels inside the solver launches
    double solve_ms;                          // time inside the solver launches (device clock of workgroup 0)
    double barrier_ms, relax_ms, push_ms;     // of which: inside grid barriers; global relabels; push phases (the last two include their barriers)
    double tail_ms;                           // of which: relabel/push rounds that began with fewer than 64 rows still holding excess
    long long tail_rounds;
    double max_barrier_wait_ms;               // longest single wait of the leader workgroup at a grid barrier
    // r06, concurrent moves: batches launched; moves committed out of a batch (solved beside others, results kept); batches that
    // ended at a move whose validation against its predecessors' changes failed (that move heads the next batch); moves the HOST
    // did not launch at all because they were provably idempotent; moves run alone (no batch)
    long long batches, batch_committed, batch_invalid, host_skipped, solo_moves;
    long long injected_discarded;             // test hook (key 40): injected failures whose move the commit threw away
};

// How an expansion ended.  `hip` means something for hip_error alone; the statistics' energy is an energy and nothing else.
enum class ExpandStatus { ok, hip_error, overflow, barrier_timeout, no_convergence, too_many_sites };
struct ExpandResult { ExpandStatus status = ExpandStatus::ok; hipError_t hip = hipSuccess; };

// resident workgroups of the solver launch per CU, as the occupancy query sees k_solve
hipError_t solver_blocks_per_cu(int* blocks);
ExpandResult run_expansion(const Graph& g, const int* cost /* n x L */, int L, int potts,
                           ExpandWork& w, int max_cycles, ExpandStats* st, hipStream_t s);
hipError_t launch_init_labeling(const int* cost, int L, int n, const int* init_or_null_dev,
                                int* label, int* cur_cost, hipStream_t s);
hipError_t launch_argmin_labels(const int* cost, int L, int n, int* label, long long* acc,
                                hipStream_t s);

// --- select.hip ------------------------------------------------------------
// packs the points with mask != 0 into cx1.. (any order); *count = their number
hipError_t launch_sel_pack_points(const Points& p, const unsigned char* mask, double* cx1, double* cy1, double* cx2, double* cy2,
                                  int* count, hipStream_t s);
// The greedy selection's round (select.hip): one set of kernels for mh_select_greedy and mh_select_greedy_msac.  Every candidate has
// a count on the support set — count >= need makes it eligible, and carries it to the next round — and a RANK VALUE: that count,
// or its MSAC weight when `weights` (with its next_ / carried_ / left_ companions) is given; null = ranked by count.  The key
// rank << 32 | ~position is built for eligible candidates only; the highest key wins.
// one rank's offer in a round: 88 bytes, the unit of the sharded exchange
struct SelRecord { unsigned long long key; double H[9]; int err; int mode; };
// SelRecord::mode, built by selection_mode_word (capi_select.hip): what the ranks of a sharded batch must agree on — the claim
// raises error 3 on any mismatch of the word.  Zero under the defaults.  This is the one table of its fields:
constexpr int SEL_MODE_SYMMETRIC = 1 << 0;             // the rank's residual mode is the symmetric transfer error (mh_set_residual_mode)
constexpr int SEL_MODE_REFIT = 1 << 1;                 // winners are refitted to their inliers (mh_set_tuning key 30)
constexpr int SEL_MODE_REFIT_3PT = 1 << 2;             // ... by the 3-point estimator (mh_set_estimator); only beside SEL_MODE_REFIT
constexpr int SEL_MODE_SAMPLER_LOCAL = 1 << 3;         // the proposer's sampler is the local one (mh_set_sampler), and then:
constexpr int SEL_MODE_SAMPLER_K_SHIFT = 4;            //   bits 4-9   k of its sampling table (3 .. 32)
constexpr int SEL_MODE_SAMPLER_UNIFORM_SHIFT = 10;     //   bits 10-14 its uniform_per_16 (0 .. 16)
constexpr int SEL_MODE_BY_WEIGHT = 1 << 15;            // ranked by MSAC weight: mh_select_greedy_msac
constexpr int SEL_MODE_HAF = 1 << 16;                  // the resident batch is mh_propose_haf's, and then:
constexpr int SEL_MODE_HAF_MEMBERS_SHIFT = 17;         //   bits 17-22 its `members` (0 .. 32)
constexpr int SEL_MODE_P3 = 1 << 23;                   // the resident batch is mh_propose_3pt's
constexpr int SEL_MODE_REFIT_DLT = 1 << 24;            // winners are refitted by the N-point DLT estimator (mh_set_estimator); only beside SEL_MODE_REFIT
static_assert(sizeof(SelRecord) == 88, "the exchanged record is 88 bytes");
// scores_full (nullable): the first round's vector for the all-gather — the rank value of an eligible candidate, -1 otherwise
hipError_t launch_sel_argmax(const int* counts, const int* weights, const int* orig, int Mc, int need, unsigned int my_off,
                             unsigned long long* key, int* scores_full, hipStream_t s);
hipError_t launch_sel_argmax_gathered(const int* gathered, int world, int longest, int base, int rem, unsigned long long* key,
                                      hipStream_t s);
hipError_t launch_sel_record(const int* counts, const int* weights, const int* orig, const double* Hs, int Mc, unsigned int my_off,
                             const unsigned long long* key_local, int err, int mode, SelRecord* record, hipStream_t s);
// next_counts / next_weights (nullable, key 36): what a kept candidate counted and weighed on this round's support set
hipError_t launch_sel_compact(const int* counts, const int* weights, const int* orig, const double* Hs, int Mc, int need,
                              const SelRecord* records, int world, unsigned int my_off, int* next_orig, double* next_H, int* rec,
                              int* next_counts, int* next_weights, hipStream_t s);
// counts[c] = carried_c[c] - left_c[c], weights likewise (r05: a round counts its candidates on the points the last claim took
// away and subtracts, instead of counting them again on everything that is left)
hipError_t launch_sel_subtract(const int* carried_c, const int* left_c, const int* carried_w, const int* left_w, int Mc, int* counts,
                               int* weights, hipStream_t s);
// rec: the seven control words (select.hip); cx1..cy2 (nullable): the points that leave, packed
hipError_t launch_sel_claim(const Points& p, const SelRecord* records, int world, const unsigned long long* key_check, double thr2,
                            unsigned char* mask, int* rec, double* sel_H, long long* sel_counter, int max_models, hipStream_t s,
                            bool by_weight, int symmetric, const double* refit, double* cx1, double* cy1, double* cx2, double* cy2);
// r05 (mh_set_tuning key 30): the round's winner refitted to its inliers in the support set by the per-label HAF least squares
// (one label); refit = 9 doubles + the refit's rank value on the support set; launch_sel_claim takes it in the winner's place when
// it is finite and that value is at least the hypothesis'.  labels: n ints, sum / label_count: one int each (scratch).
// scratch3 non-null: the point-only 3-point fit instead (launch_reestimate_3pt, reestimate_3pt_scratch_ints(n, 1) ints; a unused)
// dlt: the N-point DLT fit instead (launch_reestimate_dlt; a, ep and scratch3 unused)
hipError_t launch_sel_refit(const Points& p, const Affines& a, const Epipolar& ep, const SelRecord* records, int world, double thr2,
                            const unsigned char* mask, int* labels, double* refit, int* sum, int* label_count, hipStream_t s,
                            bool by_weight, int symmetric, int* scratch3, bool dlt = false);
hipError_t launch_sel_publish(int* rec, unsigned long long* keys, SelRecord* my_record, int* h_rec_dev, hipStream_t s);
hipError_t launch_best_fused(int* scores, int world, int longest, int base, int rem, int* h_best_dev, int* clear,
                             int clear_count, hipStream_t s);
hipError_t launch_pad_scores(const int* counts, int m, int longest, int* scores, hipStream_t s);

// --- knn.hip ----------------------------------------------------------------
constexpr int KNN_MAX_SPLITS = 16;      // slices of the candidate range (knn.hip)
hipError_t launch_knn(const Points& p, int k, int* nbr_out /* n x k */, int splits, float* part_d, int* part_i, hipStream_t s);
// r05: the same table through a grid over the source image (cells walked ring by ring until no unexamined point can enter the
// list).  scratch: cell_of n ints, count G*G ints, start G*G + 1 ints (G = knn_grid_cells(n) <= 256), P4 4n floats, orig n ints;
// hipErrorInvalidValue when the points' bounding box is not finite (the caller then takes the exhaustive pass).
int knn_grid_cells(int n);
hipError_t launch_knn_grid(const Points& p, int k, int* nbr_out, int* cell_of, int* count, int* start, float* P4, int* orig, hipStream_t s);
hipError_t launch_radius_count(const Points& p, float r2, int* counts /* n */, hipStream_t s);
hipError_t launch_radius_fill(const Points& p, float r2, const int* rowptr /* n+1 */, int* col /* nnz */, hipStream_t s);

// --- graph.hip ------------------------------------------------------------------
// Symmetric weighted CSR with reverse-arc index from directed hits on the device (a CSR, or rowptr == null: a dense
// n x stride table; column -1 = no hit).  info: 8 device ints the caller cleared —
//   [0] raw total exceeds int32, [1] longest raw row, [2] index error (1 out of range, 2 rowptr decreasing), [4..5] the same two for the folded rows.
constexpr int SYM_MAX_ROW = 1024;         // longest raw row (hits made + received) k_sym_fold sorts in LDS
hipError_t launch_hits_filter(const Points& p, int stride, float r2, int* col, int* err, hipStream_t s);
hipError_t launch_sym_count(int n, const int* rowptr, int stride, const int* col, int* deg, int* start /* n+1 */, int* info, hipStream_t s);
hipError_t launch_sym_build(int n, const int* rowptr, int stride, const int* col, const int* start, int* cursor, int* raw,
                            int* mult, int* uniq, int* out_rowptr /* n+1 */, int* info, hipStream_t s);
// wsum[i] = sum of w over row i
hipError_t launch_row_weight_sums(int n, const int* rowptr, const int* w, int* wsum, hipStream_t s);
// MH_SMOOTH_CAUCHY: w[k] = mult[k] * q(distance of the arc's sites) and wsum[i] = sum of w over row i in one pass;
// *overflow (cleared by the caller) is raised when a product or a row sum leaves int32
hipError_t launch_arc_weights(const Points& p, const int* rowptr, const int* col, const int* mult, double r2, int q_max, int* w,
                              int* wsum, int* overflow, hipStream_t s);
hipError_t launch_sym_finish(int n, const int* start, const int* raw, const int* mult, const int* rowptr, int* col, int* w,
                             int* rev, hipStream_t s);

} // namespace mh
