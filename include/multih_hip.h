/* multih_hip.h — C ABI of the MI355X-native Multi-H hot-path engine.
 *
 * This is the drop-in boundary: plain pointers and sizes, no
 * C++/torch types, status codes instead of exceptions.  The reference has no
 * FFI — its boundary is the C++ class `MultiH` (M/MultiH.h:20-149, "M/" =
 * /root/reference/MultiH/MultiH/).  `multi-h_amd/host/MultiH.{h,cpp}` re-creates
 * that class on top of these entry points; INTEGRATION.md shows the binding a
 * reference maintainer would add.  Each entry point cites the reference code
 * whose arithmetic it replaces.
 *
 * Conventions
 *   - all pointers are HOST pointers unless a name ends in `_dev`;
 *   - homographies are 9 doubles, row-major (cv::Mat 3x3 CV_64F `.data`);
 *   - labels at this boundary: -1 = outlier, 0..Nh-1 = plane (M/MultiH.cpp:547-568);
 *   - every function returns MH_OK (0) or a negative MH_ERR_*; mh_last_error()
 *     gives the message of the calling thread's last failure;
 *   - an engine is used from one thread at a time (as the reference class is);
 *   - the engine fails loudly (MH_ERR_NO_DEVICE) when no gfx950 device is
 *     usable: there is NO CPU fallback anywhere behind this header.
 */
#ifndef MULTIH_HIP_H
#define MULTIH_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MH_ABI_VERSION 2

/* exported even when the library is built with -fvisibility=hidden */
#if defined(__GNUC__) || defined(__clang__)
#define MH_API __attribute__((visibility("default")))
#else
#define MH_API
#endif

enum {
    MH_OK = 0,
    MH_ERR_NO_DEVICE = -1,   /* no HIP device / wrong arch */
    MH_ERR_INVALID = -2,     /* bad argument or call order */
    MH_ERR_HIP = -3,         /* a HIP runtime call failed */
    MH_ERR_NOT_SET = -4,     /* required input (points, F, neighbours, models) missing */
    MH_ERR_OVERFLOW = -5     /* an int32 energy of the reference's type would overflow */
};

typedef struct mh_engine mh_engine;

/* ---- library ---------------------------------------------------------- */
MH_API int mh_abi_version(void);
MH_API const char* mh_last_error(void);
MH_API int mh_device_count(void);              /* number of visible HIP devices (0 if none) */

/* ---- lifetime / parameters -------------------------------------------- */
/* MultiH::MultiH, M/MultiH.h:49-53 + M/MultiH.cpp:10-21.  One HIP stream per engine. */
MH_API int mh_create(mh_engine** out, int device);
MH_API void mh_destroy(mh_engine* e);
/* thr_F, thr_H, locality, lambda, min_inliers: the ctor arguments (defaults 3.0, 2.5, 0.002, 0.5, 0). */
MH_API int mh_set_params(mh_engine* e, double thr_fund_mat, double thr_hom, double locality,
                  double lambda, int min_inliers);
/* external != 0: launch on the caller's hipStream_t `hip_stream` (e.g. torch's current stream;
 * NULL is the HIP default stream).  external == 0: back to the engine's own stream. */
MH_API int mh_set_stream(mh_engine* e, void* hip_stream, int external);
MH_API int mh_synchronize(mh_engine* e);

/* ---- inputs ------------------------------------------------------------ */
/* Correspondences as the reference holds them after filtering: src_points, dst_points
 * (vector<cv::Point2d> -> n x 2 doubles each) and affinities (2x2 CV_64F -> n x 4 doubles,
 * order a11 a12 a21 a22, M/MultiH.cpp:928-931).  affines may be NULL if re-estimation is
 * not used.  Stored in HBM as struct-of-arrays. */
MH_API int mh_set_correspondences(mh_engine* e, const double* src_xy, const double* dst_xy,
                           const double* affines, int n);
/* fundamental_matrix (row-major 9) and epipole_2 (x, y with third coordinate 1),
 * the members GetFundamentalMatrixAndRefineData computes (M/MultiH.cpp:775-799). */
MH_API int mh_set_epipolar(mh_engine* e, const double F[9], const double e2[2]);
/* `neighbours` of ClusterMergingAndLabeling (M/MultiH.cpp:252-253) as a DIRECTED hit list in
 * CSR form: row i lists the trainIdx hits of query i (self hits allowed; skipped as in
 * M/MultiH.cpp:537).  Multiplicity semantics of setNeighbors are reproduced (SURVEY A-2). */
MH_API int mh_set_neighbors_csr(mh_engine* e, const int* rowptr, const int* col, int n);
/* Exact k-NN hit list built on the GPU in float32 (x1,y1,x2,y2) space — the engine's own
 * replacement for the FLANN radius search (deviation documented).
 * k in [1, 32], k < n.  Query i's hits are the first k candidates j != i by (d(i, j), j), d the float32
 * squared distance.  Only a finite d makes a hit: if some query has fewer than k candidates at finite
 * float32 distance (coordinates so far apart that d overflows), the call fails with MH_ERR_INVALID and
 * leaves the current graph untouched — through the grid as through the exhaustive pass. */
MH_API int mh_build_neighbors_knn(mh_engine* e, int k);
/* The same k nearest hits, but only those within `radius` of the query (radius <= 0: no cut): the reference's
 * radius (1/locality_lambda) with the list bounded the way FLANN's default search bounds it in practice
 * (32 checks: a few dozen approximate nearest neighbours, never the full ball). */
MH_API int mh_build_neighbors_knn_radius(mh_engine* e, int k, double radius);
/* The reference's neighbourhood rule itself (M/MultiH.cpp:252-253, radiusMatch with maxDistance =
 * 1/locality_lambda), answered exactly instead of by FLANN's randomised KD-trees: query i hits
 * every j (itself included) whose float32 squared distance in (x1,y1,x2,y2) is <= radius^2.
 * The hit count grows like n^2 * radius^4, so `max_hits` (0 = 2^31-1) bounds it: beyond the bound
 * the call fails with MH_ERR_OVERFLOW and leaves the current graph untouched.  hits_out
 * (nullable) receives the number of directed hits found. */
MH_API int mh_build_neighbors_radius(mh_engine* e, double radius, long long max_hits, long long* hits_out);
/* Copy the symmetric weighted graph the engine derived (rowptr n+1, col/w nnz).  Pass NULLs to
 * query nnz only.  The graph is built and kept on the device (csrc/graph.hip); the host copy is fetched by the
 * first call after a build.  w receives the weights IN FORCE — what the labeling pays per arc under the rule of
 * mh_set_smoothness_weights (the multiplicities under MH_SMOOTH_UNIFORM) —, read from the device after every change of the
 * graph or of the rule. */
MH_API int mh_get_sym_graph(mh_engine* e, int* rowptr, int* col, int* w, int* nnz);
/* The hit multiplicities mult(p,q) = #[p->q] + #[q->p] of the same arcs (nnz ints, the order of mh_get_sym_graph's col),
 * whatever rule is in force.  mult nullable.  MH_ERR_NOT_SET without a graph. */
MH_API int mh_get_sym_multiplicity(mh_engine* e, int* mult /* nnz */);
/* The weight of every arc (p,q) of the symmetric graph, i.e. what multiplies the Potts price round(100*lambda) of the pair
 * in mh_expand, mh_labeling_step, mh_labeling_energy, mh_merge_deltas and mh_drop_deltas (they read the graph's w and its
 * per-site totals and nothing else about an arc).
 *   MH_SMOOTH_UNIFORM (0, default)   w_pq = mult(p,q): the reference's smoothnessEnergy.  rho and q_max are not looked at.
 *   MH_SMOOTH_CAUCHY  (1)            w_pq = mult(p,q) * q, with
 *     1. d  the float32 squared distance of the two sites in (x1,y1,x2,y2), in mh_build_neighbors_knn's arithmetic:
 *           coordinates cast to float, dx = x1[p] - x1[q] (dy, dz, dw alike), d = ((dx*dx + dy*dy) + dz*dz) + dw*dw, every
 *           operation rounded once, no fused multiply-add;
 *     2. in double: r2 = rho*rho (once, on the host), t = r2 / (r2 + (double)d), qf = (double)q_max * t;
 *     3. q  = qf >= 1.0 ? (int)round(qf) : 1   (C round(): halves away from zero; an infinite d gives t = 0 and a NaN d
 *           fails the comparison: both give 1, and no NaN is ever converted to an int);
 *     4. the product in int64.
 *   So q == q_max at d == 0, q never rises with d, q >= 1 (no arc disappears, the reverse-arc index stays valid), the rule is
 *   symmetric bit for bit (dx and -dx square alike), and q_max == 1 is the uniform graph.  (A rho so small that rho*rho
 *   underflows to 0 gives q = 1 on every arc, d == 0 included: 0/0 is a NaN.)  This is PEARL's distance-weighted
 *   smoothness with a Cauchy profile in place of exp(-d/rho^2): an exponential has no definition that a device and a CPU twin
 *   share bit for bit, and is not offered.
 * A near arc now costs q_max * round(100*lambda) where it cost round(100*lambda).  lambda scales BOTH terms of the energy
 * (the data term by 100/lambda, the Potts price by 100*lambda), so lambda' = lambda / sqrt(q_max) keeps the short-range
 * balance between them; the engine rescales nothing itself.
 * q_max in [1, MH_SMOOTH_Q_MAX], rho finite and > 0; anything else, another rule, or a null engine: MH_ERR_INVALID, nothing
 * changed.  MH_ERR_OVERFLOW when a product mult * q or a site's weight total leaves int32: the rule, the weights and the
 * totals that were in force stay in force.
 * Sticky per engine, like mh_set_data_term.  It applies at once to a resident graph (one kernel, csrc/graph.hip
 * k_arc_weights, writing spare buffers that are swapped in on success; back to UNIFORM restores the multiplicities bit for
 * bit, no rebuild) and to every graph that arrives later — mh_set_neighbors_csr and the three builders, on the device or
 * through the host fallback for very long rows; a graph that arrives under CAUCHY and overflows is refused
 * (MH_ERR_OVERFLOW) and the engine then holds no graph.  mh_set_correspondences drops the graph, not the setting.  Nothing
 * else goes stale: the data cost does not depend on the weights. */
#define MH_SMOOTH_UNIFORM 0
#define MH_SMOOTH_CAUCHY 1
#define MH_SMOOTH_Q_MAX 256
MH_API int mh_set_smoothness_weights(mh_engine* e, int rule, double rho, int q_max);

/* ---- epipolar front half --------------------------- */
/* The reference estimates F inside Process() with cv::findFundamentalMat(RANSAC)
 * (M/MultiH.cpp:775) and takes the epipole from F F^T (:786-793).  These entry points are the
 * engine's own GPU version of that step (normalised 8-point hypotheses from counter-RNG 8-tuples,
 * Sampson-distance scoring, least-squares refit on the inliers); results are inputs for
 * mh_set_epipolar.  They do not touch the homography model set. */
/* What "distance to the epipolar geometry" means in mh_score_sampson / mh_refit_fundamental / mh_estimate_fundamental
 * (r06; part of the result's definition, so an entry point of its own and not an mh_set_tuning key):
 *   MH_FUND_SAMPSON       e^2 / (a^2 + b^2 + a'^2 + b'^2)            — the engine's default since r02
 *   MH_FUND_EPIPOLAR_MAX  max(e^2 / (a^2 + b^2), e^2 / (a'^2 + b'^2)) — the squared point-to-epipolar-line distance, the
 *                         larger of the two images: what cv::findFundamentalMat compares with its threshold (OpenCV 3.1.0
 *                         FMEstimatorCallback::computeError; the call sites are M/main.cpp:400 at 2.0 px and
 *                         M/MultiH.cpp:775 at threshold_fundamental_matrix).  At least twice the Sampson value at equal F (equal when both line normals have the same length).
 * Stays set until changed; mh_set_correspondences does not reset it. */
#define MH_FUND_SAMPSON 0
#define MH_FUND_EPIPOLAR_MAX 1
MH_API int mh_set_fundamental_metric(mh_engine* e, int metric);
MH_API int mh_propose_fund8(mh_engine* e, unsigned long long seed, long long first, int m);
MH_API int mh_get_fund_hypotheses(mh_engine* e, double* F /* m x 9 */, int* idx /* m x 8, nullable */);
MH_API int mh_score_sampson(mh_engine* e, double thr2, int* counts /* m */);
/* `iterations` rounds of {inliers of F (Sampson d < thr2) -> normalised LS 8-point -> rank 2}. */
MH_API int mh_refit_fundamental(mh_engine* e, const double F_in[9], double thr2, int iterations,
                         double F_out[9], unsigned char* inlier_mask /* n, nullable */, int* inliers);
/* propose(hypotheses) -> score -> best -> 2 refits -> epipole e2 = null(F^T), third coordinate 1. */
MH_API int mh_estimate_fundamental(mh_engine* e, unsigned long long seed, int hypotheses, double thr,
                            double F[9], double e2[2], unsigned char* inlier_mask /* n, nullable */,
                            int* inliers);

/* ---- the caller's estimator: minimal 7-point samples with a confidence stop and no refit — what
 * cv::findFundamentalMat(CV_FM_RANSAC, thr, confidence) does at M/main.cpp:399-409 and M/MultiH.cpp:775 (its draws and its
 * un-normalised arithmetic are not reproduced).  Additive: mh_estimate_fundamental above stays the default route. */
/* m samples from counter-RNG 7-tuples (n >= 7), up to three F each: fills the F-hypothesis set with 3 m slots, slot 3 s + j
 * = solution j of sample `first + s` in ascending order of its root; the finite ones first, the others nine NaNs (they
 * score 0).  mh_score_sampson and mh_get_fund_hypotheses(F, NULL) work on the set unchanged; mh_get_fund_hypotheses with a
 * non-NULL idx fails with MH_ERR_INVALID until the next mh_propose_fund8. */
MH_API int mh_propose_fund7(mh_engine* e, unsigned long long seed, long long first, int m);
MH_API int mh_get_fund7_samples(mh_engine* e, int* idx /* m x 7, nullable */, int* nvalid /* m, nullable: finite slots per sample */);
/* propose(max_samples) -> score under the engine's metric -> the sequential stop rule on the device: after sample s the
 * best count so far gives N = ceil(log(1 - confidence) / log(1 - (best / n)^7)) clamped to [1, max_samples], and the first s
 * with s + 1 >= N ends the run (samples_used = s + 1).  F is the best slot of the samples used, bit for bit (ties: the
 * lowest slot index), mask / inliers are those of F, e2 as mh_epipoles gives it.  MH_ERR_INVALID when no slot is finite,
 * the best count is 0, max_samples < 1 or confidence is outside (0, 1). */
MH_API int mh_estimate_fundamental_minimal(mh_engine* e, unsigned long long seed, int max_samples, double confidence, double thr,
                                    double F[9], double e2[2], unsigned char* inlier_mask /* n, nullable */,
                                    int* inliers, int* samples_used /* nullable */);

/* Epipoles of F with third coordinate 1: e1 = eigenvector of F^T F, e2 = eigenvector of F F^T with the
 * smallest eigenvalue (M/MultiH.cpp:786-799).  Host arithmetic only; e may be NULL. */
MH_API int mh_epipoles(mh_engine* e, const double F[9], double e1[2], double e2[2]);
/* Per-correspondence refinement of GetFundamentalMatrixAndRefineData (M/MultiH.cpp:807-838) on the
 * GPU: Hartley-Sturm correction (OptimalTriangulation :1116-1188), affine consistency filter
 * (distanceError > 1 drops the point, :824-827) and the optimal affinity (:1190-1223).
 * in_mask (n, nullable): only points with mask != 0 are processed (the F-RANSAC mask of :809).
 * keep (n): 1 where the point survives; refined (n x 8): x1 y1 x2 y2 a11 a12 a21 a22 of survivors. */
MH_API int mh_refine_correspondences(mh_engine* e, const double F[9], const double e1[2], const double e2[2],
                              const unsigned char* in_mask, unsigned char* keep, double* refined);
/* r06: at which stage of M/MultiH.cpp:807-838 each row of the LAST mh_refine_correspondences call left (n = its row count):
 * the stage table of the harness (rows after the RANSAC mask, after OptimalTriangulation, after distanceError > 1). */
#define MH_REFINE_KEPT 0
#define MH_REFINE_NOT_IN_MASK 1          /* :809  mask[i] == 0 */
#define MH_REFINE_TRIANGULATION 2        /* :815-817  OptimalTriangulation failed (optimum at infinity, :1170-1175) or its pair is not finite */
#define MH_REFINE_AFFINE_TEST 3          /* :826  distanceError > 1 (a NaN is dropped here too) */
MH_API int mh_get_refine_reasons(mh_engine* e, unsigned char* reason /* n */, int n);
/* The point-only form of mh_refine_correspondences: the Hartley-Sturm correction (step 1) alone, the same kernel and the same
 * bits as there; no affinity is read (they need not be set).  Every row that is triangulated is kept.  refined (n x 4):
 * x1 y1 x2 y2 of survivors.  mh_get_refine_reasons reports its rows (KEPT, NOT_IN_MASK, TRIANGULATION). */
MH_API int mh_refine_points(mh_engine* e, const double F[9], const double e1[2], const double e2[2],
                            const unsigned char* in_mask, unsigned char* keep, double* refined);

/* ---- reference-style initialisation ------------- */
/* ComputeLocalHomographies (M/MultiH.cpp:696-717, GetHomographyHAF :850-911): one homography per
 * correspondence from its affinity, F and e2; H_out (n x 9, nullable).  feat_out (n x 10, nullable)
 * receives the feature vectors EstablishStablePointSets clusters (:617-644) with `locality` as the
 * coordinate weight. */
MH_API int mh_local_homographies(mh_engine* e, double locality, double* H_out, double* feat_out);
/* MeanShiftClustering<double>::Cluster (MeanShiftClustering.h:23-157) on n rows of d <= 16 doubles:
 * every climb (:62-123) runs on the GPU, the sequential seed/merge/vote logic (:52-56,:100-146) on
 * the host; seeds come from the counter RNG instead of rand(), 256 at a time from the rows unvisited
 * at that moment (their climbs share the launches; a seed visited by an earlier climb of its batch
 * is dropped — HISTORY.md 3.8).  modes: up to max_modes x d;
 * assign: per row the index of its mode (-1 if none); n_modes: number of modes found. */
MH_API int mh_mean_shift(mh_engine* e, const double* data, int n, int d, double band_width,
                  unsigned long long seed, double* modes, int max_modes, int* assign, int* n_modes);

/* ---- propose: hypothesis batch ----------------------------------------- */
/* Sample `m` 4-tuples with the counter RNG (seed, first..first+m-1) and solve the normalised
 * 4-point DLT for each on the GPU (north_star; stands where the reference calls
 * cv::findHomography: M/MultiH.cpp:725, M/MultipleHomographies.h:144,339).  The batch stays
 * resident in HBM as the engine's current model set. */
MH_API int mh_propose_dlt4(mh_engine* e, unsigned long long seed, long long first, int m);
/* Upload an explicit model set (m x 9) as the current model set. */
MH_API int mh_set_models(mh_engine* e, const double* H, int m);
MH_API int mh_get_models(mh_engine* e, double* H /* m x 9 */);
MH_API int mh_get_model_count(mh_engine* e, int* m);
/* One model of the current set (9 doubles): what a caller who wants a single winner copies instead of all m. */
MH_API int mh_get_model(mh_engine* e, int idx, double H[9]);
MH_API int mh_get_samples(mh_engine* e, int* idx /* m x 4, valid after mh_propose_dlt4 and mh_propose_3pt (there the fourth column is -1) */);
/* The sampler of mh_propose_dlt4 and mh_prefetch_dlt4.  Sticky per engine; mh_set_correspondences does not reset it.
 *   MH_SAMPLER_UNIFORM  every index uniform over all correspondences (default; uniform_per_16 is ignored).
 *   MH_SAMPLER_LOCAL    neighbourhood-guided: needs the sampling table (mh_build_sample_neighbours); both entry points answer
 *                       MH_ERR_NOT_SET without one.  Hypothesis c = first + s, draws r_j = splitmix64(seed + (c << 8) + j)
 *                       (64-bit wrap-around) as under the uniform sampler:
 *                         (c & 15) < uniform_per_16: the uniform tuple of c, unchanged;
 *                         otherwise i0 = ((r_0 >> 32) n) >> 32 (the uniform tuple's first index), then for j = 1 .. 63 the
 *                         candidate nbr[i0 k + (((r_j >> 32) k) >> 32)] is taken unless it is already in the tuple, until there
 *                         are four; slots still empty after draw 63 take the first index.
 *                       uniform_per_16 in [0, 16]; with 16 the batch is the uniform batch.  The estimator is the same 4-point
 *                       DLT, bit for bit: only the tuple changes.  The ranks of a sharded mh_select_greedy must agree on the
 *                       sampler, k and uniform_per_16: their records carry the engine's SETTING at the time of the selection
 *                       (not what the resident batch was proposed with: a caller who changes the sampler between propose and
 *                       select, or loads models with mh_set_models, is compared on the setting alone). */
#define MH_SAMPLER_UNIFORM 0
#define MH_SAMPLER_LOCAL 1
MH_API int mh_set_sampler(mh_engine* e, int sampler, int uniform_per_16);
/* The local sampler's table: the dense n x k table of mh_build_neighbors_knn (same kernels, same rule: float32 distance in
 * (x1,y1,x2,y2), hits ordered by (d, j), j != i, grid or exhaustive pass by key 31, MH_ERR_INVALID when a query lacks k finite
 * hits), 3 <= k <= 32, k < n, kept in a device buffer of the sampler's own: the labeling graph is neither built, replaced nor
 * read.  mh_set_correspondences drops the table.  mh_get_sample_neighbours copies it out (MH_ERR_NOT_SET without one). */
MH_API int mh_build_sample_neighbours(mh_engine* e, int k);
MH_API int mh_get_sample_neighbours(mh_engine* e, int* nbr /* n x k, nullable */, int* k_out /* nullable */);
/* HAF proposals: one hypothesis per affine correspondence, from the reference's own minimal solver (GetHomographyHAF,
 * M/MultiH.cpp:850-911: a homography from ONE affine correspondence and F), optionally refitted to the anchor's consistent
 * neighbours (GetHomographyHAFNonminimal's least squares, :913-989, without the rescale of RefineHomographyHAF).  Such a hypothesis
 * lies on its anchor's plane and is compatible with F by construction, and a batch has n / stride of them.  Fills the engine's
 * current model set with m hypotheses, replacing it exactly as mh_propose_dlt4 / mh_set_models do: the data cost and the MSAC
 * weights go stale, mh_get_samples answers as after mh_set_models.  mh_score, mh_score_msac, mh_select_greedy,
 * mh_select_greedy_msac and mh_select_best work on the batch unchanged.
 * Hypothesis s has counter c = first + s and anchor i = c * stride.
 *   1. H0 is what mh_local_homographies writes for row i, the same bits: the six HAF rows r0 .. r5 (four columns) of the
 *      correspondence; the ten sums of A^T A (pairs a <= b of columns in the order 00 01 02 03 11 12 13 22 23 33), each
 *      s = r0a * r0b, then s = s + rqa * rqb for q = 1 .. 5; the cyclic Jacobi solve of the symmetric 4 x 4 (csrc/mh_device.hpp,
 *      jacobi_sym_dev(4)); the column of the smallest eigenvalue, the first index on ties; rows 1-2 of H from e2, F and lambda
 *      (:984-989); every entry times 1.0 / h33.
 *   2. members == 0: the hypothesis is H0.
 *   3. members > 0: for j = 0 .. members - 1, in the order of row i of the sampling table (mh_build_sample_neighbours, its first
 *      `members` columns), q = nbr[i k + j] is CONSISTENT iff the forward transfer error d2(H0 as stored, q) < thr2 — strictly; a
 *      NaN is not consistent; always the forward error (M/MultiH.cpp:434-441), whatever mh_set_residual_mode says.
 *   4. The ten sums start as the anchor's; every consistent q adds its own ten terms, formed like the anchor's, with one
 *      acc = acc + s each, in ascending j.  Then the same Jacobi solve, column choice, rows and 1.0 / h33 as in step 1.  With no
 *      consistent neighbour the result is H0, bit for bit.
 *   5. A result that is not finite stays as it is: it scores 0, as NaN models do everywhere.
 * stride >= 1, m >= 0, first >= 0, (first + m - 1) * stride < n; members is 0 or in [3, k of the table]; thr2 is not NaN.  m == 0
 * leaves an empty set, like mh_set_models(NULL, 0).  Affinities or the epipolar geometry missing: MH_ERR_NOT_SET; members > 0
 * without a table: MH_ERR_NOT_SET; everything else that is wrong: MH_ERR_INVALID.
 * The counters are global and the table is a function of the correspondences, so rank r of a sharded batch proposes its shard with
 * first + (its offset into the batch).  The ranks of a sharded selection must agree on "proposed by mh_propose_haf" and on
 * `members`: the records' mode word carries both (bit 16, bits 17-22; what the RESIDENT batch was proposed with — mh_set_models,
 * mh_propose_dlt4, mh_adopt_prefetched and mh_propose_3pt clear it), and ranks that disagree all return the mode-mismatch MH_ERR_INVALID. */
MH_API int mh_propose_haf(mh_engine* e, long long first, int m, int stride, int members, double thr2);
/* Per hypothesis of the resident batch, the bit mask of its consistent neighbours (bit j = column j of the anchor's table row).
 * MH_ERR_NOT_SET unless the resident model set came from mh_propose_haf. */
MH_API int mh_get_haf_support(mh_engine* e, unsigned* used /* m */);
/* 3-point proposals: with F a homography needs only THREE point correspondences, H = [e']x F + e' v^T (GetHomography3PT,
 * M/MultiH.cpp:995-1050).  Such a hypothesis is compatible with F by construction, needs one same-plane draw fewer than a 4-point
 * DLT and no affinities.  Fills the engine's current model set with m hypotheses, replacing it exactly as mh_propose_dlt4 does: the
 * data cost and the MSAC weights go stale, the HAF record is cleared (mh_get_haf_support answers MH_ERR_NOT_SET).  mh_score,
 * mh_score_msac, mh_select_best, mh_select_greedy and mh_select_greedy_msac work on the batch unchanged, refitted winners (key 30)
 * under both estimators included.
 *   1. Hypothesis s has counter c = first + s.  Its tuple t is the FIRST THREE indices of the 4-tuple the engine's sampler
 *      (mh_set_sampler) gives counter c under `seed` in mh_propose_dlt4:
 *        MH_SAMPLER_UNIFORM  draw j = 0, 1, .. gives r = splitmix64(seed + (c << 8) + j) (64-bit wrap-around) and the index
 *                            ((r >> 32) * n) >> 32; an index already in the tuple is rejected; at most 64 draws; slots still empty
 *                            then take the first index.
 *        MH_SAMPLER_LOCAL    counters with (c & 15) < uniform_per_16 as above; the others keep the uniform first index i0 and take
 *                            their second and third from row i0 of the sampling table, draws j = 1 .. 63, as mh_propose_dlt4 does.
 *   2. H is GetHomography3PT WITHOUT numerical refinement on (src[t], dst[t]) and the engine's F (mh_set_epipolar): Hartley
 *      normalisation of the three source and of the three destination points, Fn = T2^-T F T1^-1, the epipole of Fn from the
 *      eigenvector of Fn Fn^T with the smallest eigenvalue, the third row of the normalised H from the 6 x 3 system's normal
 *      equations by an eigen-decomposition (eigenvalues within 2 eps sum |w| of zero dropped), rows 1-2 from it, H = T2^-1 Hn T1 —
 *      operation for operation the host's Homography3PTLinear (what the post-filter's trials fit with).
 *   3. A fit with an entry that is not finite stores NINE QUIET NaNs (0x7ff8000000000000): it scores 0 everywhere.
 * mh_get_samples returns m x 4: the three indices and -1 in the fourth column.
 * m == 0 leaves an empty set, like mh_set_models(NULL, 0).  No correspondences or no epipolar geometry: MH_ERR_NOT_SET; the local
 * sampler without its table: MH_ERR_NOT_SET; fewer than 3 correspondences, m < 0, first < 0: MH_ERR_INVALID.
 * The counters are global, so rank r of a sharded batch proposes its shard with first + (its offset into the batch).  The ranks of
 * a sharded selection must agree on "proposed by mh_propose_3pt": bit 23 of the records' mode word says so of the RESIDENT batch
 * (mh_set_models, mh_propose_dlt4, mh_adopt_prefetched and mh_propose_haf clear it), and ranks that disagree all return the
 * mode-mismatch MH_ERR_INVALID.  The prefetch pipeline (mh_prefetch_dlt4) stays DLT-only. */
MH_API int mh_propose_3pt(mh_engine* e, unsigned long long seed, long long first, int m);

/* ---- score -------------------------------------------------------------- */
/* Residual definition used by mh_score / mh_residual_matrix / mh_get_residual_rows:
 *   MH_RESIDUAL_FORWARD   d2 = |H p1 - p2|^2 — the reference's formula (M/MultiH.cpp:434-441), default;
 *   MH_RESIDUAL_SYMMETRIC d2 = |H p1 - p2|^2 + |H^-1 p2 - p1|^2 — north_star's "symmetric transfer",
 *                         an extension with no reference counterpart (H^-1 = adjugate, same rounding
 *                         discipline; the definition is checked in exact rationals, tests/test_symmetric_exact.py).
 *                         Used by mh_score, mh_residual_matrix, mh_get_residual_rows and (r05) mh_select_greedy;
 *                         the data cost, the labeling, the moments and the single-model labelling follow it under
 *                         MH_RESIDUAL_SCOPE_ROUTE alone (mh_set_residual_scope below; forward by default).
 * The symmetric d2, stated once: fwd(H; p1, p2) + fwd(adj(H); p2, p1), where fwd is the forward formula above in the
 * reference's operation order, adj(H) entry by entry is (mul, mul, sub) with every operation rounded once, and the two
 * terms meet in one final rounded addition; no fused multiply-add anywhere.  A NaN d2 is neither an inlier nor inside
 * the data term's truncation T. */
enum { MH_RESIDUAL_FORWARD = 0, MH_RESIDUAL_SYMMETRIC = 1 };
MH_API int mh_set_residual_mode(mh_engine* e, int mode);
/* Which calls follow mh_set_residual_mode.
 *   MH_RESIDUAL_SCOPE_SCORE (default)  the score family listed above, and nothing else;
 *   MH_RESIDUAL_SCOPE_ROUTE            ... and the calls behind the selection: mh_data_cost, mh_labeling_step (its table, hence
 *                                      its labels and energy), mh_cost_matrix (costs and the fused counts; always the FP64
 *                                      kernel under the symmetric mode, whatever mh_set_tuning keys 15 and 23 say: the FP32
 *                                      pre-test is proved for the forward error only), mh_inlier_moments, mh_inliers_of_model
 *                                      and mh_inliers_of_homography.
 * Under SCOPE_SCORE, or under MH_RESIDUAL_FORWARD with either scope, those calls are the forward launches, bit for bit.
 * The data term's table (mh_set_data_term) is unchanged with the symmetric d2 in place of the forward one: both terms, label
 * 0, the truncation T = thr_hom^2 * 81 / 16 and C round().
 * What stays forward whatever mode and scope say: mh_score_msac and mh_select_greedy_msac (they refuse the symmetric mode),
 * mh_refit_homography, mh_polish_homographies, mh_reweight_homographies*, mh_label_residual_quantile, the compatibility
 * statistics and mh_propose_haf's consistency test.  The scope does not enter the selection records' mode word: the
 * selection never reads it.
 * Sticky per engine; mh_set_correspondences does not reset it.  Setting it (to any value) marks the data cost stale exactly as
 * mh_set_data_term does (mh_expand answers MH_ERR_NOT_SET until mh_data_cost has run); under SCOPE_ROUTE mh_set_residual_mode
 * marks it stale too, under SCOPE_SCORE it does not.  Another value, or a null engine: MH_ERR_INVALID, nothing changed. */
#define MH_RESIDUAL_SCOPE_SCORE 0
#define MH_RESIDUAL_SCOPE_ROUTE 1
MH_API int mh_set_residual_scope(mh_engine* e, int scope);
/* Inlier count of every current model over all points, forward transfer error, strict
 * d2 < thr2 (M/MultiH.cpp:430-443).  point_mask (n bytes, nullable) restricts the count to
 * points with mask != 0.  counts (m ints, nullable) receives a host copy; the counts also
 * stay resident (mh_device_buffer MH_BUF_COUNTS). */
MH_API int mh_score(mh_engine* e, double thr2, const unsigned char* point_mask, int* counts);
/* MSAC-weighted scores: per model the inlier count of mh_score AND a weight that says how well the inliers fit.  With d2 the
 * forward transfer error of the pair in the reference's operation order (M/MultiH.cpp:434-441, as under mh_set_data_term):
 *   d2 < thr2 (strictly; mh_score's decision)   the pair counts 1 and weighs (int)round(256.0 * (1.0 - (d2 / thr2)))
 *   otherwise (d2 >= thr2, inf, NaN)            the pair counts 0 and weighs 0
 * d2 / thr2 is one IEEE double division, 256.0 * (...) one rounded double multiplication (no fused multiply-add), round is C
 * round(): halves away from zero.  count[m] and weight[m] are the int32 sums over the points with mask != 0 (all points
 * without a mask): exact, independent of the order of summation, weight <= MH_MSAC_SCALE * count; an inlier just under the
 * threshold counts 1 and weighs 0.  Forward residual only: MH_ERR_INVALID under MH_RESIDUAL_SYMMETRIC.  MH_ERR_OVERFLOW,
 * before anything is launched, when n * MH_MSAC_SCALE exceeds 2^31 - 1.
 * counts / weights (m ints each, nullable) receive host copies.  The counts stay resident in MH_BUF_COUNTS exactly as after
 * mh_score (a following mh_select_best behaves as after mh_score), the weights in MH_BUF_WEIGHTS.  Most pairs are decided
 * "far" by the FP32 pre-test of mh_score (csrc/msac32.hip; mh_set_tuning key 15 = 0: every pair in FP64); the call adds n * m
 * to the pairs of mh_get_score_stats and the pairs that went through the FP64 formula to its pairs_fp64.  On an empty shard
 * (a transport is set, more ranks than hypotheses) a no-op that succeeds, as mh_score is. */
#define MH_MSAC_SCALE 256
MH_API int mh_score_msac(mh_engine* e, double thr2, const unsigned char* point_mask, int* counts, int* weights);
/* The model with the highest weight of the last mh_score_msac, the lowest index on ties (the one-workgroup arg-max of
 * mh_select_best on the weights), and that model's count.  Outputs nullable.  MH_ERR_NOT_SET unless mh_score_msac has run on
 * the current model set and correspondences: mh_set_models, mh_propose_dlt4, mh_adopt_prefetched and mh_set_correspondences
 * make the weights stale.  One rank only: MH_ERR_INVALID with a transport of world > 1. */
MH_API int mh_select_best_msac(mh_engine* e, long long* best_index, int* best_weight, int* best_count);
/* The N x M residual matrix of north_star, model-major: R[m*n + i] = d2(point i, model m),
 * written to HBM by one kernel that also produces the inlier counts.  R_host (nullable)
 * receives a host copy — leave NULL to keep the matrix on the device only. */
MH_API int mh_residual_matrix(mh_engine* e, double thr2, double* R_host, int* counts);
/* The s = 4 variant of the matrix: the int32 PEARL data cost (dataEnergy, M/MultiH.cpp:473-504, or the engine's
 * other data term: mh_set_data_term; label = model + 1) of every current model against every point, model-major C[m*n + i], written to HBM by one kernel that also
 * produces the inlier counts (strict d2 < thr_hom^2).  Uses the engine's lambda and thr_hom (mh_set_params).  C_host
 * (nullable) receives a host copy. */
MH_API int mh_cost_matrix(mh_engine* e, int* C_host, int* counts);
/* Copy rows [first, first+count) of the resident residual matrix (valid after
 * mh_residual_matrix) to the host, tightly packed count x n doubles. */
MH_API int mh_get_residual_rows(mh_engine* e, int first, int count, double* rows_host);
/* Label points with the single model idx where inlier (ComputeInliersOfHomography,
 * M/MultiH.cpp:743-768): labels[i] = label_value if d2 < thr2, else unchanged. */
MH_API int mh_inliers_of_model(mh_engine* e, int idx, double thr2, int label_value, int* labels /* in/out n */);
/* Same labelling for a homography that is NOT in the resident model set (row-major H[9]); the
 * model set is left untouched.  Used by the sharded propose stage, where the winning hypothesis
 * of a round may live on another rank. */
MH_API int mh_inliers_of_homography(mh_engine* e, const double* H, double thr2, int label_value, int* labels /* in/out n */);
/* One homography refitted to ALL its inliers over the resident correspondences: the step cv::findHomography(CV_RANSAC) runs
 * behind its winning minimal sample (M/MultiH.cpp:719-741), without OpenCV's Levenberg-Marquardt polish.  Like
 * mh_inliers_of_homography it touches neither the resident model set nor the counts, weights, data cost or graph.  One
 * launch of one workgroup whatever `iterations` is (csrc/refit_h.hip, k_refit_h).
 *   Inlier set  S(H) = { i : d2(H, i) < thr2 }, strictly; d2 the forward transfer error in the reference's operation order
 *               (M/MultiH.cpp:434-441); a NaN is not an inlier; always the forward error, whatever mh_set_residual_mode says.
 *   Sums        every FP64 sum below in the engine's order: thread t of 256 starts at 0.0 and adds the terms of the members of
 *               S with index = t (mod 256) in ascending index, each as acc = acc + term; then the binary tree s = 128 .. 1,
 *               v[t] = v[t] + v[t + s].  No fused multiply-add anywhere.
 *   fit(S)      with c = |S|; fails when c < 4.
 *     1. the centroids of both images, sum * (1.0 / c);
 *     2. the mean distances d = sum of sqrt(ax * ax + ay * ay), (ax, ay) = point - centroid, and the scales
 *        s = sqrt(2.0) / (d / c); fails when a scale is not finite;
 *     3. x, y, u, v = (coordinate - centroid) * scale, (x, y) from the first image, (u, v) from the second; p = (x, y, 1.0);
 *     4. for the six pairs a <= b in the order 00 01 02 11 12 22, t = p_a * p_b and the 24 sums
 *          G0 += t    G1 += u * t    G2 += v * t    G3 += (u * u + v * v) * t
 *        the normal matrix of the two DLT rows [-p, 0, u p] and [0, -p, v p] (symmetric 9 x 9):
 *          M[a][b] = M[3+a][3+b] = G0    M[a][6+b] = M[6+b][a] = -G1    M[3+a][6+b] = M[6+b][3+a] = -G2    M[6+a][6+b] = G3
 *        every other entry 0;
 *     5. the cyclic Jacobi solve (csrc/mh_device.hpp, jacobi_sym_dev(9)); the column of the smallest eigenvalue, the first index
 *        on ties, as the row-major Hn;
 *     6. T2^-1 Hn T1 by the 4-point DLT proposer's steps (csrc/dlt4.hip): per row (a, b, c) of Hn
 *          (a * s1, b * s1, (c - (a * s1) * cx1) - (b * s1) * cy1),
 *        then rows 1 and 2 times 1.0 / s2 plus cx2 resp. cy2 times row 3; the sum of the nine squares in index order from 0.0,
 *        every entry times 1.0 / sqrt(sum), negated when h33 < 0;
 *     7. fails when an entry of the result is not finite.
 *   Rounds      cur = H_in, n_cur = |S(cur)|, accepted = 0; for r = 1 .. iterations:
 *     1. cand = fit(S(cur)); stop when it fails;
 *     2. stop when cand equals cur bit for bit;
 *     3. n_cand = |S(cand)|; stop when n_cand < n_cur (a refit must explain at least as many points: the rule of mh_set_tuning key 30);
 *     4. cur = cand, n_cur = n_cand, ++accepted.
 *   Outputs     H_out = cur; inlier_mask (n bytes, 1 = inlier) and inliers are those of H_out; fits_accepted = accepted.  With
 *               nothing accepted H_out is H_in's nine doubles unchanged (not renormalised), so iterations = 0 gives the mask
 *               and count of H_in.
 * MH_ERR_INVALID for a null engine, H_in or H_out, iterations outside [0, 16], a NaN thr2; MH_ERR_NOT_SET without
 * correspondences.  Affinities and the epipolar geometry are not read: the point-only route can call it.  Deterministic, so
 * every rank of a sharded run (all hold all points) gets the same result without an exchange. */
MH_API int mh_refit_homography(mh_engine* e, const double H_in[9], double thr2, int iterations, double H_out[9],
                               unsigned char* inlier_mask /* n, nullable */, int* inliers /* nullable */,
                               int* fits_accepted /* nullable */);
/* Levenberg-Marquardt polish of m homographies, each over the resident correspondences that carry its label: the minimiser of
 * the forward transfer error itself — what the route scores, thresholds and labels by (M/MultiH.cpp:434-441) — where every
 * other estimate of the engine is a linear fit to an algebraic error.  It is the step cv::findHomography runs behind its
 * re-estimated winner (ten rounds there; M/MultiH.cpp:725 calls it).  The loop is LMSolverImpl::run (M/Utilities.hpp:762-869;
 * host/merge_step.cpp restates it for three parameters, lm_run3); compute() is OpenCV 3.1.0's HomographyRefineCallback, which
 * is not in the reference tree, so this comment is the definition (tests/polish_h_numpy.py restates it).  One launch of one
 * 256-thread workgroup per model whatever max_iterations is (csrc/polish_h.hip, k_polish_h).  It reads the points only —
 * not the affinities, F, the resident model set, counts, weights, data cost or graph — and leaves all of them untouched.
 *   Members     S_k = { i : labels[i] == k }, k = 0 .. m - 1; every other value (-1, >= m) belongs to nobody.
 *   Parameters  x_j = H_in[k][j] / H_in[k][8], j = 0 .. 7.
 *   compute(x)  per member (X, Y) -> (u, v):
 *                 ww = (x6 * X + x7 * Y) + 1.0;  ww = |ww| > DBL_EPSILON ? 1.0 / ww : 0.0
 *                 xi = ((x0 * X + x1 * Y) + x2) * ww      yi = ((x3 * X + x4 * Y) + x5) * ww      r = (rx, ry) = (xi - u, yi - v)
 *               and, with a = (X * ww, Y * ww, ww), bx = (-(a0 * xi), -(a1 * xi)), by = (-(a0 * yi), -(a1 * yi)), the Jacobian rows
 *                 [a0 a1 a2 0 0 0 bx0 bx1]      [0 0 0 a0 a1 a2 by0 by1]
 *   Sums        every FP64 sum below in the engine's order (that of mh_refit_homography): thread t of 256 starts at 0.0 and adds
 *               the terms of the members with index = t (mod 256) in ascending index, each as acc = acc + term; then the binary
 *               tree s = 128 .. 1, v[t] = v[t] + v[t + s].  No fused multiply-add anywhere.  The 30 terms of a member:
 *                 S         rx * rx + ry * ry
 *                 v = J^T r a_i * rx (i = 0 1 2), a_i * ry (i = 0 1 2), bx0 * rx + by0 * ry, bx1 * rx + by1 * ry
 *                 A = J^T J a_i * a_j for the pairs 00 01 02 11 12 22 (both 3 x 3 diagonal blocks; the block between them is 0),
 *                           a_i * bx_j (A[i][6+j]) and a_i * by_j (A[3+i][6+j]), i = 0 1 2, j = 0 1,
 *                           bx0 * bx0 + by0 * by0, bx0 * bx1 + by0 * by1, bx1 * bx1 + by1 * by1 (the last 2 x 2 block)
 *               max |r| is the largest |rx| or |ry| of a member (a NaN is never the largest).  A candidate's Sd is the sum S alone.
 *   pinv        of a symmetric 8 x 8 M: the cyclic Jacobi (csrc/mh_device.hpp, jacobi_sym_dev(8)) gives w and the columns V;
 *               cut = (sum of |w_k| in index order from 0.0) * (2.0 * DBL_EPSILON); eigenvalues with |w_k| <= cut are dropped
 *               (sym_eig_solve3's cut).  pinv(M) b: from 0.0, for the kept k in index order, proj = (sum_i V[i][k] * b[i] from
 *               0.0) / w_k, out[i] = out[i] + proj * V[i][k].  Its diagonal: out[i] = out[i] + V[i][k] * V[i][k] / w_k.
 *   The loop    S, A, v, max |r| = compute(x); D = diag(A), once; lambda = 1, lc = 0.75, iter = 0, accepted = 0.  Repeat:
 *     1. Ap = A with Ap[i][i] = A[i][i] + lambda * D[i];  d = pinv(Ap) v;  xd[i] = x[i] - d[i];  Sd from compute(xd);
 *     2. temp[i] = -(sum_j A[i][j] * d[j] from 0.0) + 2.0 * v[i];  dS = sum_i d[i] * temp[i] from 0.0;
 *        R = (S - Sd) / (|dS| > DBL_EPSILON ? dS : 1.0);
 *     3. R > 0.75: lambda = lambda * 0.5, then lambda = 0 when lambda < lc.
 *        R < 0.25: t = sum_i d[i] * v[i] from 0.0;  nu = (Sd - S) / (|t| > DBL_EPSILON ? t : 1.0) + 2.0, raised to 2.0 when
 *        nu < 2.0, lowered to 10.0 when nu > 10.0; when lambda == 0: p = the diagonal of pinv(A), maxval = the largest of
 *        DBL_EPSILON and |p_i|, lambda = lc = 1.0 / maxval, nu = nu * 0.5; then lambda = lambda * nu;
 *     4. Sd < S: the step is accepted — S = Sd, x = xd, ++accepted;
 *     5. ++iter; stop when iter >= max_iterations, or max_i |d_i| < FLT_EPSILON, or an entry of d is not finite (this stop is
 *        not in LMSolverImpl::run: there the loop would go on with x standing still);
 *     6. after an accepted step A, v and max |r| are those of compute(x) (D stays); stop when max |r| < FLT_EPSILON.
 *     max_iterations = 0 runs compute(x) once and reports S.
 *   Outputs     H_out[k] = (x0 .. x7, 1.0) — the form cv::findHomography returns — when a step was accepted, otherwise H_in[k]'s
 *               nine doubles unchanged; cost[k] = (S of H_in, S of H_out); info[k] = (|S_k|, iter, accepted, status).
 *               status 1: |S_k| < 4; status 2 (looked at after status 1): an x_j is not finite (H_in[k][8] == 0, a NaN).  With
 *               status 1 or 2 H_out[k] is H_in[k]'s nine doubles, cost[k] = (0, 0) and iter = accepted = 0.
 * MH_ERR_INVALID for a null engine, labels, H_in or H_out, m outside [1, 65536], max_iterations outside
 * [0, MH_POLISH_MAX_ITERATIONS]; MH_ERR_NOT_SET without correspondences.  H_out may be H_in.  The point-only route can call
 * it.  Deterministic, so every rank of a sharded run (all hold all points) gets the same result without an exchange. */
#define MH_POLISH_MAX_ITERATIONS 32
MH_API int mh_polish_homographies(mh_engine* e, const int* labels /* n */, const double* H_in /* m x 9 */, int m,
                                  int max_iterations, double* H_out /* m x 9 */,
                                  double* cost /* m x 2: S before, S after; nullable */,
                                  int* info /* m x 4: members, iterations run, steps accepted, status; nullable */);
/* Iteratively reweighted N-point DLT refits of m homographies, each over the resident correspondences that carry its label.
 * Every other per-label estimate of the engine (the HAF fit, the 3-point fit, MH_ESTIMATOR_DLT, mh_polish_homographies) is a
 * plain least-squares fit over whatever the labeling handed it, contaminated or not; this one weighs each member by its MSAC
 * gain under the model that stands, so members that model explains badly pull less and members beyond c2 not at all.  There
 * is no counterpart in the reference, so this comment is the definition (tests/reweight_h_numpy.py restates it).  One launch
 * of one 256-thread workgroup per model whatever `rounds` is (csrc/reweight_h.hip, k_reweight_h).  It reads the points only —
 * not the affinities, F, the resident model set, counts, weights, data cost or graph — and leaves all of them untouched.
 *   Members     S_k = { i : labels[i] == k }, k = 0 .. m - 1; every other value (-1, >= m) belongs to nobody.
 *   Weight      of member i under H: d2 the forward transfer error in the reference's operation order (M/MultiH.cpp:434-441),
 *               always the forward error, whatever mh_set_residual_mode says;
 *                 w = d2 < c2 ? 1.0 - (d2 / c2) : 0.0
 *               strictly; a NaN gives 0.  One IEEE division and one subtraction: mh_score_msac's expression in front of its
 *               256.0 *.  The support of H is the set of members with d2 < c2; each of them has w > 0.
 *   Sums        every FP64 sum below in the engine's order (that of mh_refit_homography): thread t of 256 starts at 0.0 and adds
 *               the terms of the members with index = t (mod 256) in ascending index, each as acc = acc + term; then the binary
 *               tree s = 128 .. 1, v[t] = v[t] + v[t + s].  No fused multiply-add anywhere.  Members with w == 0 contribute no
 *               term: they are skipped, not added as zeros.
 *   wfit(H)     fit(S) of mh_refit_homography with every member's terms weighted by its w under H:
 *     1. W = sum of w and c = |support|; fails when c < 4;
 *     2. the centroids of both images, (sum of w * coordinate) * (1.0 / W);
 *     3. d = sum of w * sqrt(ax * ax + ay * ay), (ax, ay) = point - centroid, and the scales s = sqrt(2.0) / (d / W); fails when
 *        a scale is not finite;
 *     4. x, y, u, v and p = (x, y, 1.0) exactly as in fit(S) step 3;
 *     5. for the six pairs a <= b in the order 00 01 02 11 12 22, t = p_a * p_b, wt = w * t and the 24 sums
 *          G0 += wt    G1 += u * wt    G2 += v * wt    G3 += (u * u + v * v) * wt
 *     6. the normal matrix, the Jacobi solve, the de-normalisation and the finiteness test of fit(S) steps 4 (layout) to 7.
 *               With every weight 1.0 wfit is fit(S) bit for bit.
 *   Rounds      cur = H_in[k], done = 0; for r = 1 .. rounds:
 *     1. cand = wfit(cur); stop when it fails;
 *     2. stop when cand equals cur bit for bit;
 *     3. cur = cand, ++done.
 *               There is no acceptance test: the caller gets the gains and judges.
 *   Outputs     H_out[k] = cur — with done == 0 H_in[k]'s nine doubles unchanged (not renormalised); gain[k] = (W under H_in[k],
 *               W under H_out[k]) over the members; info[k] = (|S_k|, support of H_out[k], done, status).  status 1: |S_k| < 4;
 *               status 2 (looked at after status 1): an entry of H_in[k] is not finite.  With status 1 or 2 H_out[k] is H_in[k]'s
 *               nine doubles, gain[k] = (0, 0), the support 0 and done 0.  rounds = 0 reports W and the support of H_in.
 * MH_ERR_INVALID for a null engine, labels, H_in or H_out, m outside [1, 65536], rounds outside [0, MH_REWEIGHT_MAX_ROUNDS], a
 * c2 that is not finite or <= 0; MH_ERR_NOT_SET without correspondences.  H_out may be H_in.  The scale is the caller's: at c2
 * near the noise floor the weights cut into the noise and cost accuracy on clean sets.  The point-only and
 * epipolar-free routes can call it.  Deterministic, so every rank of a sharded run (all hold all points) gets the same result
 * without an exchange. */
#define MH_REWEIGHT_MAX_ROUNDS 16
MH_API int mh_reweight_homographies(mh_engine* e, const int* labels /* n */, const double* H_in /* m x 9 */, int m,
                                    double c2, int rounds, double* H_out /* m x 9 */,
                                    double* gain /* m x 2: W of H_in, W of H_out; nullable */,
                                    int* info /* m x 4: members, support of H_out, rounds done, status; nullable */);
/* Per label, one order statistic of its members' transfer errors under a model: the robust scale estimate the reweighted fit
 * lacks (a median of a label's own residuals follows that label's noise, whatever the caller knows about it).  There is no
 * counterpart in the reference, so this comment is the definition (tests/label_scale_numpy.py restates it).  One launch of one
 * 256-thread workgroup per model (csrc/label_scale.hip, k_label_quantile): a radix select on the 64-bit pattern of the key.
 *   Members     S_k = { i : labels[i] == k }, c = |S_k|; every other value (-1, >= m) belongs to nobody.
 *   Key         of member i: d2, the forward transfer error under H[k] in the reference's operation order (M/MultiH.cpp:434-441),
 *               always the forward error, whatever mh_set_residual_mode says; a NaN counts as +inf.  d2 is a sum of two squares:
 *               never negative, never -0, so its 64-bit pattern orders like the number.
 *   Rank        r = ((long long)(c - 1) * num) / den, integer division: num / den = 1/2 the lower median, 0/1 the minimum, 1/1
 *               the maximum.
 *   Result      d2_out[k] = the element at 0-based rank r of the ascending multiset of the keys: exact, and independent of any
 *               evaluation order.  info[k] = (c, r, the number of members whose key is strictly smaller than d2_out[k], status).
 *               status 1: c == 0 — d2_out[k] is the quiet NaN 0x7ff8000000000000, rank and below are 0.  There is no other
 *               status: a model with entries that are not finite simply produces NaN keys, which count as +inf.
 * MH_ERR_INVALID for a null engine, labels, H or d2_out, m outside [1, 65536], den outside [1, MH_QUANTILE_MAX_DEN], num outside
 * [0, den]; MH_ERR_NOT_SET without correspondences.  It reads the points only and leaves the engine's state untouched, like
 * mh_polish_homographies (its launch is timed in the MH_K_REESTIMATE slot).  Deterministic, so every rank of a sharded run gets the
 * same result without an exchange. */
#define MH_QUANTILE_MAX_DEN 65536
MH_API int mh_label_residual_quantile(mh_engine* e, const int* labels /* n */, const double* H /* m x 9 */, int m,
                                      int num, int den, double* d2_out /* m */,
                                      int* info /* m x 4: members, rank, members strictly below the value, status; nullable */);
/* mh_reweight_homographies with the scale taken from the data in every round (csrc/label_scale.hip, k_autoscale_reweight_h: all
 * rounds in one launch of one workgroup per model; per round the selection passes of mh_label_residual_quantile, then wfit's
 * three passes and solve as they stand).  Members, weight, sums and wfit are those of mh_reweight_homographies.
 *   scale(H)    q = the order statistic of mh_label_residual_quantile (num, den) over the label's members under H; s = kappa2 * q
 *               (one multiplication); c2 = s < c2_min ? c2_min : (s > c2_max ? c2_max : s).  s is never a NaN (q is not, and
 *               kappa2 > 0 is finite); q = +inf or an overflow gives c2_max.
 *   Rounds      cur = H_in[k], done = 0; for r = 1 .. rounds:
 *     1. c2 = scale(cur);
 *     2. cand = wfit(cur) with the weights d2 < c2 ? 1.0 - (d2 / c2) : 0.0; stop when it fails;
 *     3. stop when cand equals cur bit for bit;
 *     4. cur = cand, ++done.
 *   Outputs     H_out[k] = cur — with done == 0 H_in[k]'s nine doubles unchanged; scale[k] = (scale(H_in[k]), scale(H_out[k]));
 *               gain[k] = (W under H_in[k] at scale(H_in[k]), W under H_out[k] at scale(H_out[k])): the two W belong to DIFFERENT
 *               scales and are NOT comparable as an objective (a model with a smaller median error gets a smaller c2 and may
 *               get a smaller W); info[k] = (|S_k|, support of H_out[k] at its scale, done, status), statuses 1 (|S_k| < 4) and
 *               2 (an entry of H_in[k] not finite) as in mh_reweight_homographies: with either, gain[k] = scale[k] = (0, 0), the
 *               support and done 0 and H_out[k] H_in[k]'s bits.  rounds = 0 reports the scale, W and support of H_in.
 *   Degenerate  with c2_min == c2_max == c2 the call is mh_reweight_homographies(.., c2, rounds, ..) bit for bit in H_out, gain
 *               and info.
 * MH_ERR_INVALID under the conditions of mh_reweight_homographies (without its c2), for num / den as in
 * mh_label_residual_quantile, a kappa2 that is not finite or <= 0, bounds that are not finite or violate 0 < c2_min <= c2_max;
 * MH_ERR_NOT_SET without correspondences.  H_out may be H_in.  Reads the points only; deterministic. */
MH_API int mh_reweight_homographies_auto(mh_engine* e, const int* labels /* n */, const double* H_in /* m x 9 */, int m,
                                         int num, int den, double kappa2, double c2_min, double c2_max, int rounds,
                                         double* H_out /* m x 9 */,
                                         double* gain  /* m x 2: W of H_in at its scale, W of H_out at its scale; nullable */,
                                         double* scale /* m x 2: c2 under H_in, c2 under H_out; nullable */,
                                         int* info     /* m x 4: members, support of H_out at its scale, rounds done, status; nullable */);
/* Trial statistics of HomographyCompatibilityCheck (M/MultiH.cpp:128-196; host/merge_step.cpp ClusterMedian) for
 * `clusters` clusters of at least 19 points each.  pts_xyxy: the clusters' points back to back in cluster order, 4 doubles
 * each (x1 y1 x2 y2); cluster_begin[c] .. cluster_begin[c+1] (cluster_begin[0] = 0); per (cluster, trial): tri = the
 * positions inside the cluster of the 3 points the trial drew (:140-151), H = the trial's 3-point homography (:154,
 * row-major 9), ok = 0 when that fit failed (all distances then count as NaN -> 1e300).  stats_out: 8 doubles per
 * (cluster, trial): the order statistics of the N-3 squared transfer errors (:158-173) at ranks k-3 .. k+1, k = (N-3)/2,
 * then their three largest values ascending — all a trial's "median" (:175-176) can depend on, bit-identical to sorting
 * on the host.  Independent of the resident correspondences. */
MH_API int mh_compat_trial_stats(mh_engine* e, const double* pts_xyxy, const int* cluster_begin, int clusters, const int* tri,
                                 const double* H, const unsigned char* ok, int trials, double* stats_out);
/* r06: the same with the trials' 3-point homographies fitted ON THE DEVICE (GetHomography3PT without refinement, M/MultiH.cpp:154,
 * :995-1050) from F — until r05 the host fitted the 501 x clusters of them.  Bit-identical to the host's fits
 * (host/merge_step.cpp, Homography3PTLinear).  H_out (clusters x trials x 9) / ok_out (clusters x trials): nullable, the fits. */
MH_API int mh_compat_trial_stats_fit(mh_engine* e, const double* pts_xyxy, const int* cluster_begin, int clusters, const int* tri,
                              const double F[9], int trials, double* stats_out, double* H_out, unsigned char* ok_out);
/* The compatibility check WITHOUT F: per cluster the median over `trials` trials of the median forward transfer error of the
 * cluster's other points under a 4-point DLT fit to four random members.  There is no reference counterpart (the reference's
 * trials are 3-point fits with F, above); this comment is the definition.
 *   Input       pts_xyxy and cluster_begin as in mh_compat_trial_stats: the clusters' points back to back, four doubles each;
 *               cluster c = [begin[c], begin[c+1]), begin[0] == 0.  nc = its size, b0 = begin[c].  Independent of the resident
 *               correspondences.
 *   Tuple       trial t of cluster c is hypothesis m = c * trials + t of the call, with the counter first + m.  Its four local
 *               positions follow the uniform rule of mh_propose_dlt4 over nc indices: draw j = 0, 1, .. gives
 *               r = splitmix64(seed + (counter << 8) + j) and the position ((r >> 32) * nc) >> 32; a position already in the
 *               tuple is rejected; at most 64 draws; slots still empty then take the first position.  idx_out holds
 *               b0 + position (positions in the concatenated array).
 *   Fit         mh_propose_dlt4's normalised 4-point DLT on those four points, the same operations in the same order: unit
 *               Frobenius norm, h33 >= 0.  A result that is not finite stays as it is.
 *   Trial value a member is left out if and only if its local position equals one of the four tuple entries; rest = the number
 *               of the others (nc - 4 unless the tuple holds repeats).  The key of a member is its forward transfer error d2
 *               under the trial's H, in the reference's operation order (M/MultiH.cpp:434-441: the engine's residual); a NaN key
 *               counts as +inf (0x7ff0000000000000), as in mh_label_residual_quantile.  trial_out[c][t] = the key at 0-based
 *               rank (rest - 1) / 2 of the ascending multiset (the lower median): exact, independent of any evaluation order.
 *   Cluster     medians_out[c] = the element at 0-based rank (trials - 1) / 2 of the ascending multiset of the cluster's trial
 *               values.
 * MH_ERR_INVALID for a null engine, pts_xyxy, cluster_begin or medians_out; clusters < 1; a cluster_begin that does not start at
 * 0 or is not non-decreasing; a cluster of fewer than MH_COMPAT_DLT_MIN_POINTS points; trials outside
 * [1, MH_COMPAT_DLT_MAX_TRIALS]; first < 0; clusters * trials > 2^22.
 * The call reads nothing of the engine's state and changes none of it: the resident model set, samples, counts, weights, data
 * cost, graph and prefetch queue stay untouched.  Deterministic, so the ranks of a sharded run need no exchange.  Three launches
 * on the engine's stream, timed in the slots MH_K_DLT4 (the fits), MH_K_SCORE (the trial values) and MH_K_REESTIMATE (the
 * cluster values). */
enum { MH_COMPAT_DLT_MIN_POINTS = 5, MH_COMPAT_DLT_MAX_TRIALS = 4096 };
MH_API int mh_compat_dlt_medians(mh_engine* e, const double* pts_xyxy, const int* cluster_begin, int clusters,
                                 unsigned long long seed, long long first, int trials,
                                 double* medians_out   /* clusters */,
                                 double* trial_out     /* clusters x trials, nullable */,
                                 double* H_out         /* clusters x trials x 9, nullable */,
                                 int* idx_out          /* clusters x trials x 4, nullable */);
/* ---- multi-GPU transport (one process per GPU, hypotheses sharded, correspondences replicated) ------
 * The reference is a single process; the one exchange north_star adds is an all-gather of per-model inlier scores.
 * The engine calls the transport with DEVICE pointers: send `bytes_per_rank` bytes, receive world * bytes_per_rank in
 * rank order.  Two kinds (give exactly one; both NULL with world = 1 clears the transport):
 *   stream_fn  enqueues the collective on `hip_stream` (the engine's stream) and returns at once — ncclAllGather of
 *              RCCL; multi-h_amd/host/rccl_transport.cpp is that function.  No host synchronisation, no Python.
 *   host_fn    is called with the engine's stream idle and returns once recv_dev is complete (the torch.distributed
 *              hook of multi-h_amd/sharding.py, used to rehearse several ranks on one GPU over gloo).
 * Rank r owns the hypotheses [r * base + min(r, rem), ...) of a batch of total_m (base = total_m / world, rem = total_m
 * % world, the first rem shards one longer) as its resident model set. */
typedef int (*mh_allgather_stream_fn)(void* ctx, const void* send_dev, void* recv_dev, unsigned long long bytes_per_rank,
                                      void* hip_stream);
typedef int (*mh_allgather_dev_fn)(void* ctx, const void* send_dev, void* recv_dev, unsigned long long bytes_per_rank);
MH_API int mh_set_transport(mh_engine* e, int rank, int world, mh_allgather_stream_fn stream_fn, mh_allgather_dev_fn host_fn,
                            void* ctx);
/* Greedy model selection over the resident hypothesis batch, on the device (csrc/select.hip): up to `max_models`
 * rounds of {score the candidates over the points still in the support mask, take the best — highest count, lowest
 * position in the WHOLE batch on ties —, stop if it has fewer than `need` inliers, take its inliers out of the mask}.
 * This is the sequential-RANSAC scheme of the dead M/MultipleHomographies.h:146-175 behind MultiH::ProposeModels.
 * point_mask (n bytes, nullable = all ones): in = points that may support a model, out = points no selected model
 * explains.  H_out: max_models x 9; counters_out / counts_out (nullable): position of each selected hypothesis in the
 * whole batch and its inlier count when selected.  Per round the host reads five control words from mapped memory; no
 * host<->device copy is issued inside the loop (mh_get_copy_stats).  Scores AND claims on the engine's residual mode
 * (r05: the symmetric transfer error too; until r04 the mode was refused).
 * Sharded batch (a transport is set; total_m = size of the whole batch, 0 = the resident set is the whole batch): in the
 * first round the ranks all-gather their int32 score vectors (north_star's exchange); in every round they all-gather
 * one 88-byte record each — {best score and its position, that hypothesis' H, an error word} — and pick the same
 * winner.  Outputs do not depend on the number of ranks.  A rank-local failure (the state of that rank's engine: wrong
 * shard size, a failing scoring launch) does not keep the rank out of the round's collectives: it offers
 * nothing, sets the record's error word, and after the exchange every rank leaves the loop — the failing one with its
 * own error, the others with MH_ERR_HIP "a rank reported an error".  Arguments (thr2, need, max_models, total_m) must be
 * the same on every rank, and so must the settings the records' mode word carries: the residual mode, refitted winners and their
 * estimator (bits 2 and 24), the sampler, (bit 15) whether the rank ranks by count — this entry point — or by weight
 * (mh_select_greedy_msac), (bit 16, bits 17-22) whether the resident batch is mh_propose_haf's and with how many members, and
 * (bit 23) whether it is mh_propose_3pt's;
 * ranks that disagree all return MH_ERR_INVALID after the first exchange. */
MH_API int mh_select_greedy(mh_engine* e, double thr2, int need, int max_models, unsigned char* point_mask,
                            double* H_out, long long* counters_out, int* counts_out, int* selected_out, long long total_m);
/* The same selection RANKED BY MSAC WEIGHT — a mode beside mh_select_greedy, which is unchanged.  The arguments are those of
 * mh_select_greedy plus weights_out (nullable, max_models ints).  Each round works on the support set S: the points with
 * mask != 0 (all points when no mask is given).
 *   1. Score.        Every candidate c gets count_c and weight_c over S exactly as mh_score_msac defines them: a pair with
 *                    d2 < thr2 counts 1 and weighs (int)round(256.0 * (1.0 - (d2 / thr2))), every other pair counts 0 and weighs
 *                    0; d2 is the forward error in the reference's operation order.
 *   2. Eligibility.  A candidate is eligible when count_c >= need.  A weight never makes up for a missing count.
 *   3. Winner.       The eligible candidate with the highest weight, the lowest position in the WHOLE batch on ties.  If no
 *                    candidate is eligible the selection ends.  An eligible candidate of weight 0 can still win (every inlier
 *                    may sit just under the threshold).
 *   4. Claim.        The winner's inliers on S leave S (d2 < thr2, strictly).  H_out, counters_out, counts_out and weights_out
 *                    take the hypothesis' H, batch position, count and weight at the moment it was selected.
 *   5. Compaction.   Candidates with count_c >= need move on to the next round, the winner does not (counts and weights only
 *                    fall as S shrinks).
 *   6. Refit (mh_set_tuning key 30; HAF, MH_ESTIMATOR_3PT or MH_ESTIMATOR_DLT as for mh_select_greedy).  The winner is refitted to its inliers on S;
 *                    the refit takes its place in the claim and in H_out when it is finite and its WEIGHT on S is at least the
 *                    hypothesis' weight (mh_select_greedy: "explains at least as many points").  counts_out and weights_out
 *                    stay the hypothesis' own.
 * MH_ERR_INVALID under MH_RESIDUAL_SYMMETRIC (as mh_score_msac); MH_ERR_OVERFLOW, before anything is launched, when
 * n * MH_MSAC_SCALE exceeds 2^31 - 1; the argument checks of mh_select_greedy.  mh_set_tuning keys 15 (every pair in FP64) and
 * 36 (rounds by subtraction or by recount) are schedules here too: same outputs.  The pairs scored go into mh_get_score_stats as
 * under mh_score_msac.
 * Sharded batch: the collectives of mh_select_greedy, with the same sizes — in the first round one all-gather of the int32 score
 * vectors (here: the weight of every eligible hypothesis, -1 for the others), in every round one 88-byte record per rank (the
 * key's high word is the weight).  "Ranked by weight" travels in the records' mode word: if one rank calls mh_select_greedy and
 * another this entry point, every rank returns the mode-mismatch MH_ERR_INVALID after the first round's exchange; nobody waits
 * in a collective the others do not run.  Rank-local failures as in mh_select_greedy.  Outputs do not depend on the number of
 * ranks. */
MH_API int mh_select_greedy_msac(mh_engine* e, double thr2, int need, int max_models, unsigned char* point_mask,
                                 double* H_out, long long* counters_out, int* counts_out, int* weights_out, int* selected_out,
                                 long long total_m);
/* Pipelined propose: mh_prefetch_dlt4 prepares the batch (seed, first .. first+m-1) in one of the engine's spare model buffers
 * on a second stream, concurrently with whatever the main stream is doing (csrc/dlt4.hip); mh_adopt_prefetched makes the OLDEST
 * prepared batch the current model set — the main stream waits for the side stream's event, the host does not wait at all.
 * Up to TWO batches may be prepared ahead (a third mh_prefetch_dlt4 answers MH_ERR_INVALID until one is adopted).  With the
 * batch after next prepared too — adopt i, prefetch i+2, sweep i — the DLT a sweep waits for was dispatched a whole sweep
 * earlier and nothing is handed from stream to stream between two sweeps; with one batch ahead the sweep is held until the
 * second stream has reached the DLT's dispatch (a sweep that reaches the chip first leaves the DLT no room until it ends).
 * Same hypotheses, bit for bit, as mh_propose_dlt4.  mh_set_correspondences drops whatever is queued. */
MH_API int mh_prefetch_dlt4(mh_engine* e, unsigned long long seed, long long first, int m);
MH_API int mh_adopt_prefetched(mh_engine* e);
/* Best-supported model of the scored batch (highest resident inlier count, lowest position in the whole batch on ties) by
 * the engine's own arg-max kernel.  With a transport the ranks first all-gather their int32 score vectors (BASELINE
 * configs[3]; the gathered vector stays resident: MH_BUF_GATHERED_SCORES) and every rank finds the same winner; a rank
 * whose shard is empty (more ranks than hypotheses) takes part with nothing to offer.
 * best_index / best_count both NULL: ENQUEUE ONLY.  With a stream-ordered transport (or none) the all-gather, the arg-max
 * and the publication then run on a stream of their own behind an event of the sweep, OFF the main stream's critical
 * path: the next sweep starts at once and writes the engine's other counts buffer (after such a call MH_BUF_COUNTS is
 * undefined until the next scoring call).  A later call with outputs — before anything else has been scored — or
 * mh_synchronize completes it; the ranks' send buffer is the batch's own counts buffer (no padding kernel).  The
 * host-synchronised transport runs the same steps on the main stream.
 * Whether a call is a NEW exchange is decided from state that is the same on every rank (r05): the model-set generation
 * the last exchange belongs to and whether a scoring call has been made since — on an empty shard the scoring entry points
 * are no-ops that succeed and count.  The ranks make the same calls; a rank-local failure (a model set that is not the
 * rank's shard, an unscored batch) travels through the collective as an error marker: that rank returns its own error,
 * every other rank's next fetch fails with MH_ERR_HIP "a rank reported an error", none is left waiting. */
MH_API int mh_select_best(mh_engine* e, long long total_m, long long* best_index, int* best_count);
/* mh_score and mh_select_greedy decide most (point, model) pairs in FP32 with a rigorous error bound and only the pairs
 * within that bound of the threshold in FP64 (csrc/score32.hip; the counts are the FP64 formula's, bit for bit).  pairs:
 * pairs scored that way since the last reset; pairs_fp64: how many of them needed the FP64 formula. */
MH_API int mh_get_score_stats(mh_engine* e, long long* pairs, long long* pairs_fp64, int reset);
/* Number of explicit host<->device copies mh_select_greedy has issued since the last reset. */
MH_API int mh_get_copy_stats(mh_engine* e, long long* h2d, long long* d2h, int reset);
/* Per-model inlier moments {n, Sx, Sy, Sxx, Sxy, Syy} and smallest eigenvalue of the 3x3
 * scatter — the collinearity test of MergingStep (M/MultiH.cpp:446-463). */
MH_API int mh_inlier_moments(mh_engine* e, double thr2, double* moments /* m x 6 */, double* min_eig /* m */);

/* ---- label --------------------------------------------------------------- */
/* The data term of mh_data_cost, mh_cost_matrix and mh_labeling_step.  With lam = 100 / lambda and T = thr_hom^2 * 81 / 16
 * (both computed in double, in that order of operations), B = (int)round(lam * T), and d2 the forward transfer error of the
 * pair in the reference's operation order (M/MultiH.cpp:434-441: s = h6 x + h7 y + h8; u = (h0 x + h1 y + h2) / s;
 * v = (h3 x + h4 y + h5) / s; d2 = (x2 - u)^2 + (y2 - v)^2, every operation rounded once) — or, under MH_RESIDUAL_SYMMETRIC
 * with MH_RESIDUAL_SCOPE_ROUTE, the symmetric d2 as stated at mh_set_residual_mode —, the int32 cost of (point, label) is
 *                               MH_DATA_TERM_REFERENCE (default)             MH_DATA_TERM_RISING
 *   label 0 (outlier)           B                                            B
 *   d2 < T (strictly)           (int)round(lam * (1.0 - (d2 / T)))           (int)round(lam * (d2 / T))
 *   otherwise (d2 >= T, NaN)    2 * B                                        2 * B
 * d2 / T is one IEEE double division, lam * (...) one rounded double multiplication (no fused multiply-add anywhere), round
 * is C round(): halves away from zero.  REFERENCE is dataEnergy (M/MultiH.cpp:473-504): 100 / lambda at a perfect fit falling
 * to 0 at the threshold.  RISING is the same expression without the `1.0 -`: 0 at a perfect fit rising to round(lam) just
 * below the threshold; the outlier cost, the truncation, the scales and the Potts term are the same.
 * Sticky per engine; mh_set_correspondences does not reset it.  Setting it (to any value) marks the data cost stale, as
 * mh_set_params does: mh_expand answers MH_ERR_NOT_SET until mh_data_cost has run.  The inlier counts fused into
 * mh_cost_matrix do not depend on it, and mh_select_greedy never reads it.  Another value, or a null engine: MH_ERR_INVALID. */
#define MH_DATA_TERM_REFERENCE 0
#define MH_DATA_TERM_RISING 1
MH_API int mh_set_data_term(mh_engine* e, int term);
/* The engine's data term (dataEnergy, M/MultiH.cpp:473-504, by default) for every (site, label): cost[i*(Nh+1)+l], int32,
 * label 0 = outlier, l>=1 = current model l-1.  cost (nullable) receives a host copy. */
MH_API int mh_data_cost(mh_engine* e, int* cost);
/* alpha-expansion over the current data cost and neighbour graph with the Potts term
 * round(100*lambda) (M/MultiH.cpp:506-511; GCoptimization.cpp:975-1058,1212-1289).
 * labels: in = initial labeling in GCO numbering 0..Nh (NULL = all zero), out = result in GCO
 * numbering.  energy: final int32 energy; cycles: executed cycles.
 * Contract: any non-negative int32 cost table (mh_data_cost's, or a table written into MH_BUF_COST behind it) and any graph.
 * Overflow bound: the call returns MH_ERR_OVERFLOW when the energy of the initial labeling exceeds 2^31 - 1, or when one
 * n-link potts * w_pq (w_pq = hit multiplicity) does — there GCO's int EnergyType / EnergyTermType wrap and its result is
 * not defined.  Below that bound every t-link and every move's total flow fit int32 (each is at most the energy of the
 * labeling the move starts from, which never increases) and the result is GCO's.  Deviation: the push-relabel solver holds
 * a site's excess and an arc's cumulative flow counter to 2^30 and refuses the call (MH_ERR_OVERFLOW) beyond, where GCO's
 * int max-flow would still be exact; with an initial energy of at most 2^30 no excess can reach that, a flow counter could
 * in principle (pushes back and forth over one arc).  The engine never returns MH_OK with a wrapped result. */
MH_API int mh_expand(mh_engine* e, const int* init_labels, int* labels_out, int* energy, int* cycles);
/* Counters of the last alpha-expansion: {0 cycles, 1 moves, 2 accepted moves, 3 push phases, 4 relaxation
 * intervals, 5 host synchronisations, 6 dominance-reduction launches, 7 moves that still needed
 * push-relabel after the reduction, 8 kernel launches, 9 moves actually run (the others were skipped on the
 * device as provably idempotent), 10 moves whose undecided core was not empty, 11 sum and 12 maximum of the
 * core sizes, 13 grid barriers, 14 global relabels, 15 microseconds spent inside the solver launches, of which
 * 16 inside grid barriers, 17 in global relabels and 18 in push phases (both including their barriers), 19 in
 * relabel/push rounds that began with fewer than 64 solver rows still holding excess (the tail of a move), 20 restarts of
 * the expansion after a grid-barrier timeout (a GPU shared with other persistent launches: each restart halves the
 * solver's workgroups; results never depend on their number), 21 workgroups of the solver launch in the attempt that
 * completed, 22 restarts of all expansions of this engine so far, 23 the longest single wait at a grid barrier in microseconds (the give-up time of
 * the next expansion's first attempts is max(20 ms, 50 x the longest such wait the engine has seen); r05: the FIRST barrier of a
 * launch — the one that waits for every workgroup to be dispatched — gets max(250 ms, ten times that), a timed-out attempt is
 * repeated once with the same grid before the grid is halved, word 22 = restarts of all expansions of this engine so far; only
 * the last attempt waits 3 s)}. */
MH_API int mh_get_expand_stats(mh_engine* e, long long stats[24]);
/* r06: the concurrent alpha-moves of the last expansion (csrc/expand.hip, k_commit): [0] batches launched, [1] moves kept out of a
 * batch (solved beside others on the same labeling and validated), [2] batches that ended at a move whose test failed (it heads the
 * next batch), [3] moves the host never launched because they were provably idempotent, [4] moves run alone, [5] failures injected by the test hook of key 40 whose move
 * its batch threw away,
 * [6] moves per batch (mh_set_tuning key 37), [7] label count from which the first cycle is batched too (key 38). */
MH_API int mh_get_expand_batch_stats(mh_engine* e, long long stats[8]);
/* Per-move log of the last alpha-expansion's solver launches (diagnostic; enabled with mh_set_tuning key 8 = number of
 * moves to log): 8 ints per move {undecided core sites, workgroups, global relabels, relabel intervals, push phases, grid
 * barriers, 100 MHz ticks inside the launch, of which inside barriers}; all zero for moves that were skipped or had an empty core. */
MH_API int mh_get_expand_trace(mh_engine* e, int* trace /* moves x 8 */, int moves);
/* Diagnostic (mh_set_tuning key 21 = number of moves): connected components of each move's undecided core, 16 ints per move
 * {core sites, components, largest, second largest, sites in components of <= 64 / 256 / 1024 / 2048 / 8192 sites, components of
 * those sizes, propagation rounds, 0}; zeros for skipped moves.  Never changes a result. */
MH_API int mh_get_core_components(mh_engine* e, int* out /* moves x 16 */, int moves);
/* The re-estimator of mh_reestimate, mh_labeling_step and the refitted winners of mh_select_greedy (mh_set_tuning key 30).
 *   MH_ESTIMATOR_HAF  GetHomographyHAFNonminimal (M/MultiH.cpp:913-989): needs the affinities and the epipolar geometry (default)
 *   MH_ESTIMATOR_3PT  GetHomography3PT without LM refinement (M/MultiH.cpp:995-1050) over each label's members: H = [e']x F + e' v^T
 *                     by least squares from the points alone; needs the epipolar geometry, not the affinities.  A label with
 *                     fewer than 3 members keeps its H (as does one whose fit is not finite).
 *   MH_ESTIMATOR_DLT  the normalised N-point DLT over each label's members, from the points alone: needs neither the epipolar
 *                     geometry nor the affinities (csrc/reestimate_dlt.hip, k_dlt_reestimate).  For label k = 0 .. Nh-1,
 *                     S_k = { i : labels[i] == k } (labels of -1 or >= Nh belong to nobody) and H[k] = fit(S_k), with fit(S)
 *                     exactly as defined under mh_refit_homography: its steps 1-7, every FP64 sum in the engine's order (thread
 *                     t of 256 adds the members with index = t (mod 256) in ascending index from 0.0, then the binary tree
 *                     128 .. 1), no fused multiply-add, jacobi_sym_dev(9) and the column of the smallest eigenvalue (the first
 *                     index on ties), k_dlt4's de-normalisation, unit Frobenius norm, h33 >= 0.  When the fit fails (|S_k| < 4,
 *                     a scale that is not finite, an entry of the result that is not finite) the label keeps its H's nine
 *                     doubles unchanged.  (Members that are all one point fail through the scale only where the centroid comes
 *                     out as that point exactly; where it rounds away from it the scales are finite and the fit is what the
 *                     steps give.)  There is no acceptance test against inlier counts: the loop's re-estimators replace
 *                     unconditionally, and under key 30 the selection's own rule decides.  MH_BUF_LABEL_COUNTS receives |S_k|.
 * Sticky per engine; mh_set_correspondences does not reset it.  The ranks of a sharded mh_select_greedy must agree on it.
 * Another value: MH_ERR_INVALID. */
#define MH_ESTIMATOR_HAF 0
#define MH_ESTIMATOR_3PT 1
#define MH_ESTIMATOR_DLT 2
MH_API int mh_set_estimator(mh_engine* e, int estimator);
/* Reweighted rounds for the MH_ESTIMATOR_DLT re-estimator of mh_reestimate and mh_labeling_step.  rounds = 0 (default): nothing
 * anywhere changes, k_dlt_reestimate runs.  rounds in [1, MH_REWEIGHT_MAX_ROUNDS]: the re-estimator is
 * mh_reweight_homographies(labels, H, Nh, c2, rounds) in place on the resident models — each label starts from its standing
 * model, the one the labeling was made with; a label whose first round fails (or with fewer than 4 members, or a standing model
 * that is not finite) keeps its H; MH_BUF_LABEL_COUNTS receives |S_k| as before.  The other estimators ignore the setting, and
 * so does the refit of the greedy selections (mh_set_tuning key 30): the selections and their mode word stay as they are.
 * Sticky per engine; mh_set_correspondences does not reset it.  MH_ERR_INVALID for a null engine, rounds outside
 * [0, MH_REWEIGHT_MAX_ROUNDS], or with rounds > 0 a c2 that is not finite or <= 0 (with rounds = 0 c2 is not looked at). */
MH_API int mh_set_estimator_reweighting(mh_engine* e, int rounds, double c2);
/* The same with the scale taken from the data: with rounds in [1, MH_REWEIGHT_MAX_ROUNDS] the MH_ESTIMATOR_DLT re-estimator is
 * mh_reweight_homographies_auto(labels, H, Nh, num, den, kappa2, c2_min, c2_max, rounds) in place on the resident models;
 * MH_BUF_LABEL_COUNTS receives |S_k|.  Of the two setters the last call decides which rule runs: mh_set_estimator_reweighting
 * switches this rule off (whatever its rounds), this call replaces the fixed one; rounds = 0 switches reweighting off altogether.
 * The other estimators, the key-30 refit of the greedy selections and their mode word ignore it, as they ignore the fixed setting.
 * Sticky per engine.  MH_ERR_INVALID for a null engine, rounds outside [0, MH_REWEIGHT_MAX_ROUNDS], or with rounds > 0 the
 * argument conditions of mh_reweight_homographies_auto (with rounds = 0 the other arguments are not looked at). */
MH_API int mh_set_estimator_reweighting_auto(mh_engine* e, int rounds, int num, int den, double kappa2, double c2_min, double c2_max);
/* GetHomographyHAFNonminimal for every label (M/MultiH.cpp:913-989 + the 1/lambda rescale of
 * Homography_RefineHAFCallback.h:33-34), or the 3-point fit under MH_ESTIMATOR_3PT, or the N-point DLT under MH_ESTIMATOR_DLT.
 * labels: -1..Nh-1 per point.  Updates the current model set in place (the data cost goes stale); H_out (nullable) receives a
 * host copy.  Needs: HAF the affinities and mh_set_epipolar, 3PT mh_set_epipolar, DLT correspondences and models only (a
 * missing mh_set_epipolar or missing affinities is no error there). */
MH_API int mh_reestimate(mh_engine* e, const int* labels, double* H_out);
/* LabelingStep (M/MultiH.cpp:513-602): data cost -> expansion (warm start iff warm != 0, from
 * `labeling` + 1) -> labels - 1 -> re-estimation (the engine's estimator).  labeling: in/out n ints (-1..Nh-1).
 * Needs the neighbour graph and what the estimator needs (see mh_reestimate): under MH_ESTIMATOR_DLT neither affinities nor
 * mh_set_epipolar. */
MH_API int mh_labeling_step(mh_engine* e, int warm, int* labeling, double* energy, int* cycles);

/* ---- the energy of a given labeling, and what joining two labels would do to it (csrc/merge_energy.hip) ----
 * Notation of mh_data_cost / mh_expand: lam = 100 / lambda, T = thr_hom^2 * 81 / 16, potts = round(100 * lambda);
 * cost(i, H) the engine's data term (mh_set_data_term) of the forward error — of the symmetric error under
 * MH_RESIDUAL_SYMMETRIC with MH_RESIDUAL_SCOPE_ROUTE —, the arithmetic of mh_data_cost; w_pq the symmetric graph's
 * multiplicity; an undirected neighbour pair counts once.  All sums are int64.  Neither call needs F or affinities.
 *
 * mh_labeling_energy: labels in -1..Nh-1 (anything else: MH_ERR_INVALID).
 *     data   = sum_i (labels[i] < 0 ? round(lam * T) : cost(i, H[labels[i]]))
 *     smooth = potts * sum w_pq [labels[p] != labels[q]]
 *     energy = data + smooth;  parts (nullable) = { data, smooth }.
 * On the labels mh_expand returns (minus one) this is mh_expand's energy.
 *
 * mh_merge_deltas: per pair (a, b), 0 <= a < b < Nh, with S_a = { i : labels[i] == a }, S_b likewise, S = S_a u S_b
 * (a label outside 0..Nh-1 belongs to nobody):
 *     H_ab     = fit(S), the N-point DLT stated under mh_refit_homography (the summation order of the per-label fits)
 *     data_old = sum_{i in S} cost(i, H[labels[i]])        (the resident models)
 *     data_new = sum_{i in S} cost(i, H_ab)
 *     cut      = potts * sum w_pq over the undirected pairs with one end in S_a and the other in S_b
 *     delta    = data_new - data_old - cut;   parts (nullable) = { |S|, data_old, data_new, cut } per pair
 * status: MH_MERGE_OK, MH_MERGE_EMPTY (S_a or S_b has no member) or MH_MERGE_NO_FIT (fewer than 4 members, a scale or an entry
 * of the fit not finite); not OK: delta = LLONG_MAX, the pair's H_out row and parts stay as the caller passed them.
 * The contract: relabelling b -> a and replacing model a by H_ab changes mh_labeling_energy by exactly delta; the deltas of
 * pairs that share no label add.  The call changes nothing in the engine: models, data-cost freshness, labels, counts and
 * mode words stay.  The union's model is the N-point DLT whatever mh_set_estimator says.
 * MH_ERR_INVALID: null engine; null labels / pairs / delta / status with npairs > 0; npairs < 0 or > 2^20; a pair with
 * a >= b or a label outside [0, Nh).  MH_ERR_NOT_SET without correspondences, models or a neighbour graph.  npairs == 0:
 * MH_OK, nothing is launched. */
#define MH_MERGE_OK      0
#define MH_MERGE_EMPTY   1
#define MH_MERGE_NO_FIT  2
#define MH_MERGE_MAX_PAIRS (1 << 20)
MH_API int mh_merge_deltas(mh_engine* e, const int* labels /* n */, const int* pairs /* npairs x 2 */, int npairs,
                           double* H_out /* npairs x 9, nullable */, long long* delta /* npairs */,
                           long long* parts /* npairs x 4, nullable */, int* status /* npairs */);
MH_API int mh_labeling_energy(mh_engine* e, const int* labels /* n */, long long* energy, long long* parts /* 2, nullable */);

/* ---- every site's best alternative label, and what dropping a label would do to the energy (csrc/label_cost.hip) ----
 * The notation above: lam, T, potts, cost(i, H) in the arithmetic of mh_data_cost, w_pq; cost(i, -1) = round(lam * T), the
 * outlier cost.  The graph has no self arcs and both directions carry the same w.  All sums are int64.  labels in -1..Nh-1.
 *
 * Used labels: U = { k in 0..Nh-1 : some labels[i] == k }.
 *
 * mh_best_alternative: per site i, with C_i = ({-1} u U) \ {labels[i]}:
 *     alt[i]      = the first minimum of cost(i, l) over l in C_i in the order -1, 0, 1, ... (the outlier first, then the lowest
 *                   index)
 *     alt_cost[i] = that minimum;   own_cost[i] = cost(i, labels[i])
 * C_i empty (the site is an outlier and no label is used): alt[i] = -1, alt_cost[i] = round(lam * T).
 * The N x Nh table is never written: alt and alt_cost are the arg-min over the rows of mh_data_cost's table, restricted to C_i.
 *
 * mh_drop_deltas: the arg-min once, then per candidate label k with members S_k = { i : labels[i] == k } and
 * labels' = labels with alt[i] in place of k on S_k:
 *     data_old   = sum_{S_k} cost(i, H[k])                  data_new   = sum_{S_k} alt_cost[i]
 *     smooth_old = potts * sum w_pq [labels[p] != labels[q]]    smooth_new = potts * sum w_pq [labels'[p] != labels'[q]]
 *                  both over the undirected pairs with at least one end in S_k, each pair once
 *     delta      = data_new - data_old + smooth_new - smooth_old
 *     parts (nullable) = { |S_k|, data_old, data_new, smooth_old, smooth_new } per candidate
 * status: MH_DROP_OK or MH_DROP_EMPTY (no member); not OK: delta = LLONG_MAX, the candidate's parts row stays as the caller
 * passed it.  alt_out (nullable): the n best alternatives the deltas were computed with.
 * The contract: with the models as they stand, mh_labeling_energy(labels') - mh_labeling_energy(labels) == delta, exactly.
 * With a cost beta >= 0 per used label, E_beta = mh_labeling_energy + beta |U|, a drop — like a join of mh_merge_deltas —
 * removes one used label: it lowers E_beta iff delta - beta < 0.
 * Both calls need correspondences and models (mh_drop_deltas: and the neighbour graph), no F and no affinities, and change
 * nothing in the engine: models, data-cost freshness, labels, counts and mode words stay.
 * MH_ERR_INVALID: null engine; null labels / alt; null cand / delta / status with ncand > 0; a label outside -1..Nh-1; a
 * candidate outside [0, Nh); ncand outside [0, Nh].  MH_ERR_NOT_SET without correspondences, models or (mh_drop_deltas) a
 * neighbour graph.  ncand == 0: MH_OK, nothing is launched. */
#define MH_DROP_OK     0
#define MH_DROP_EMPTY  1
MH_API int mh_best_alternative(mh_engine* e, const int* labels /* n */, int* alt /* n */, int* alt_cost /* n, nullable */,
                               int* own_cost /* n, nullable */);
MH_API int mh_drop_deltas(mh_engine* e, const int* labels /* n */, const int* cand /* ncand labels */, int ncand,
                          long long* delta /* ncand */, long long* parts /* ncand x 5, nullable */, int* status /* ncand */,
                          int* alt_out /* n, nullable */);

/* ---- device-side access (bench / multi-GPU plumbing) --------------------- */
enum { MH_BUF_COUNTS = 0, MH_BUF_MODELS = 1, MH_BUF_RESIDUALS = 2, MH_BUF_LABELS = 3, MH_BUF_COST = 4, MH_BUF_GATHERED_SCORES = 5,
       MH_BUF_LABEL_COUNTS = 6 /* per label, its member count in the last re-estimation (mh_reestimate / mh_labeling_step) */,
       MH_BUF_WEIGHTS = 7 /* per model, the weight of the last mh_score_msac (m ints) */ };
/* Device pointer and size in bytes of a resident buffer (valid until the next call that
 * re-allocates it).  Used to wrap the per-model scores in a tensor for the RCCL all-gather. */
MH_API int mh_device_buffer(mh_engine* e, int which, void** ptr_dev, unsigned long long* bytes);

/* Per-kernel HIP-event timing on the engine's stream.  When enabled every launch of the
 * instrumented kernels is bracketed by events; stats are resolved at the next synchronize. */
enum { MH_K_DLT4 = 0, MH_K_RESIDUAL = 1, MH_K_SCORE = 2, MH_K_DATACOST = 3, MH_K_EXPAND = 4,
       MH_K_REESTIMATE = 5, MH_K_COSTMATRIX = 6,
       /* r06: what mh_select_best enqueues on the exchange stream — the all-gather of the scores (when a transport is set)
        * and the arg-max launch behind it — from the moment the batch's sweep has ended to the end of that launch: a rank's
        * wait for its peers plus the wire time, per exchange */
       MH_K_EXCHANGE = 7, MH_K_COUNT_ = 8 };
MH_API int mh_profile_enable(mh_engine* e, int on);
MH_API int mh_profile_reset(mh_engine* e);
MH_API int mh_profile_get(mh_engine* e, int kernel, int* launches, double* total_ms);
/* mh_set_tuning — every key in one table (r06).  Class:
 *   S  product switch, SCHEDULE ONLY: accepted by the product library, never changes a result (defaults are the measured optima)
 *   R  product switch that CHANGES RESULTS — key 30 alone
 *   D  diagnostic: what is logged / read back, never a result
 *   T  test hook: injects a failure
 *   X  experiment of a measurement build: accepted only by a library compiled with -DMH_TUNING (python multi-h_amd/build.py
 *      --tuning); the product library takes the value 0 and answers MH_ERR_INVALID to anything else
 *
 *  key class default  what
 *   0   X     0       residual kernel variant (other tilings, nt stores, compiler division, store-only calibration, fused multiply-adds: one not bit-exact)
 *   1   X     0       score kernel variant
 *   2   S     128     alpha-expansion solver: frontier (relax) rounds per barrier interval
 *   3   S     512     ... most push cycles per phase
 *   4   S     1       ... push phases per global relabel
 *   5   S     256     ... workgroups of the solver launch
 *   6   S     2       dominance-reduction rounds per launch (0 = off)
 *   7   S     6       mean shift: climb iterations per host round trip (launched schedule)
 *   8   D     0       moves logged by mh_get_expand_trace (0 = off)
 *   9   D     -1      the move whose relabels are logged one by one
 *  10   S     6       push cycles per phase as a multiple of the last relabel's depth
 *  11   S     1       flow recycling between the cycles of an expansion (0: every move from the zero flow)
 *  12   S     1       dominance-reduction launches per move (1 or 2)
 *  13   X     0       row pitch of R in doubles (0 = the product's)
 *  14   T     0       the first attempts of the next n expansions count as barrier time-outs (restart with fewer workgroups)
 *  15   S     1       FP32 pre-test of the score kernels (0: the FP64 sweep for every pair; counts equal by construction)
 *  16   X     0       tiling of that pre-test kernel
 *  17   S     2       passes of the dominance cascade inside the solver launch (0 = to its fixed point)
 *  18   T     0       the n-th scoring round of the coming greedy selections fails on this rank (collective exit of mh_select_greedy)
 *  19   S     0       residual sweep as a resident grid: workgroup slots left free beyond its own occupancy (-1: one hardware-dispatched workgroup per item)
 *  20   S     1       the sweep is held until the second stream has reached a pending DLT prefetch's dispatch
 *  21   D     0       moves whose core components are diagnosed (mh_get_core_components)
 *  22   S     0       dummy streams created in front of the engine's second stream, before its first use (placement experiment kept in the product: no effect on results)
 *  23   S     8       int32 cost matrix as a resident grid: point slices (0: one workgroup per item; -1: about 37 500 items)
 *  24   S     12      the same for the FP32 pre-test score
 *  25   S     0       DLT proposer's form: 0 by context (registers + DPP for mh_propose_dlt4, LDS-staged for mh_prefetch_dlt4), 1 LDS everywhere, 2 registers everywhere — same bits
 *  26   X     0       resident residual sweep takes its items slice-major with this many point slices
 *  27   X     0       the same order for the resident cost-matrix kernel
 *  28   X     0       cost-matrix kernel evaluates the near pairs of several models together (same matrix; slower)
 *  29   S     12      mean shift: at most this many running climbs of a batch finish in one persistent launch (0 = a launch per iteration)
 *  30   R     0       mh_select_greedy refits every round's winner to the correspondences of the support set it explains (the loop's
 *                     per-label HAF least squares, M/MultiH.cpp:913-989, one label; needs affinities and the epipolar geometry; under
 *                     MH_ESTIMATOR_3PT the 3-point least squares, which needs the epipolar geometry alone; under MH_ESTIMATOR_DLT
 *                     the N-point DLT fit over the winner's inliers on the support set, which needs the points alone) before it
 *                     claims them; the refit takes the hypothesis' place when it is finite and explains at least as many.  Sticky per engine;
 *                     class MultiH sets it on every call (SetProposalRefit, default on).  The ranks of a sharded batch must agree on it
 *                     (their records carry it; r06).
 *  31   S     1       k-NN table through a grid over the source image (0: the exhaustive pass) — the same table
 *  32   S     1       mean shift: a workgroup per climb through a one-coordinate index, one launch per batch (0: keys 7 / 29's schedule)
 *  33   S     8       ... members per iteration beyond which an indexed climb counts as dense and is handed to the persistent kernel
 *  36   S     1       greedy selection: rounds after the first count on the points the last claim took out and subtract (0: count again on what is left)
 *  37   S     16      alpha-expansion: this many consecutive moves are solved together on the same labeling and committed in order, each
 *                     validated against what its predecessors changed (1: one move after the other, the form until r05) — same labels,
 *                     energies and cycle counts
 *  38   S     16      ... from the first cycle on for label sets of at least this many labels (smaller sets from the second cycle)
 *  39   S     0       ... sites per wavefront in the setup and reduction launches of a batch of moves: 16 / 32 / 64, 0 = by the size of the
 *                     launch (moves x sites); a move alone takes 16, a batch's energy-difference launch 64
 *  40   T     0       (g << 4) | k, g >= 1: in the NEXT expansion, the solve of context k (0..15) of the g-th group of moves it enqueues
 *                     (a batch or a move alone, counted from 1) is marked as not converged.  A move that is kept reports it ("push-relabel
 *                     did not converge", MH_ERR_HIP); a move its batch throws away (solved on a labeling an accepted predecessor has
 *                     changed) is solved again, and mh_get_expand_batch_stats word 5 counts it
 *  34   X     0       the 3-point re-estimator's member form (measurement libraries): 0 by size, 1 the match loop, 2 the compacted lists
 * (35 is not assigned.) */
MH_API int mh_set_tuning(mh_engine* e, int key, int value);

#ifdef __cplusplus
}
#endif
#endif /* MULTIH_HIP_H */
