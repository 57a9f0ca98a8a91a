// multih_internal.h — what the sources of the host layer share and no caller sees: the engine's C ABI with its optional
// entry points referenced weakly, and the helpers MultiH.cpp and hooks.cpp both use.  Every host source that calls an mh_*
// function includes this header and none includes multih_hip.h on its own: one strong reference to an optional entry point
// would make the layer unlinkable against an engine library without it.
#pragma once

#include <cstdint>
#include <vector>

#include "MultiH.h"
#include "multih_hip.h"

// The optional entry points are referenced weakly because the class is also linked against the suite's stand-in engine
// (tests/fake_engine.cpp, the host-boundary test under AddressSanitizer), which defines the ABI up to mh_set_tuning and none
// of these.  Against libmultih_hip.so they always resolve; where they do not, the default route runs unchanged and the mode
// that needs one fails with a message instead of a link error (multih::detail::LinkedEngineCaps, MultiH::PlanRun).
// the point-only route, the N-point estimator (SetEstimator) and the minimal-sample F estimator (SetFundamentalEstimator)
#pragma weak mh_set_estimator
#pragma weak mh_refine_points
#pragma weak mh_estimate_fundamental_minimal
// the proposal sampler (SetProposalSampler)
#pragma weak mh_set_sampler
#pragma weak mh_build_sample_neighbours
// the data term (SetDataTerm)
#pragma weak mh_set_data_term
// the error of the route (SetResidual)
#pragma weak mh_set_residual_mode
#pragma weak mh_set_residual_scope
// the MSAC tail (SetTailScore)
#pragma weak mh_score_msac
#pragma weak mh_select_best_msac
#pragma weak mh_get_model
// the refit of the tail's winner (SetTailRefit)
#pragma weak mh_refit_homography
// the LM polish of the results (SetTailPolish, SetModelPolish)
#pragma weak mh_polish_homographies
// the reweighted refits (SetModelReweight*, SetEstimatorReweight*)
#pragma weak mh_reweight_homographies
#pragma weak mh_set_estimator_reweighting
#pragma weak mh_reweight_homographies_auto
#pragma weak mh_set_estimator_reweighting_auto
// the selection ranked by weight (SetSelectionScore)
#pragma weak mh_select_greedy_msac
// the HAF and the 3-point proposals (SetProposalSource)
#pragma weak mh_propose_haf
#pragma weak mh_propose_3pt
// the compatibility check without F (SetCompatibilityFit(COMPAT_FIT_DLT))
#pragma weak mh_compat_dlt_medians
// the energy-tested merge (SetMergeMode(MERGE_ENERGY)) and the label cost (SetLabelCost)
#pragma weak mh_merge_deltas
#pragma weak mh_labeling_energy
#pragma weak mh_drop_deltas
// the distance-weighted smoothness (SetSmoothnessWeights)
#pragma weak mh_set_smoothness_weights

namespace multih {
namespace detail {

// Which of the optional entry points the linked engine library has: the one place that looks at the weak symbols' addresses
// to fill a MultiH::EngineCaps.
MultiH::EngineCaps LinkedEngineCaps();

// false, with the engine's message on stderr, unless rc is MH_OK
bool Check(int rc, const char* what);

// a 3 x 3 matrix that OWNS its storage, filled from nine doubles
cv::Mat MatFrom9(const double* h);

// MergingStep (M/MultiH.cpp:352-471) on a given engine: host candidates (merge_step.cpp MergeCandidates), then the N x
// candidates scoring and the collinearity filter on the GPU (mh_inlier_moments; :430-463).  kept: the surviving
// candidates, 9 doubles each.  Returns an MH_* status.  The correspondences must be resident in the engine; its model
// set is replaced by the candidates.
// F == nullptr: the epipolar-free route, whose candidate of a mode is its medoid (merge_step.cpp MergeCandidatesMedoid).
int MergingStepOnEngine(mh_engine* engine, const double* H, int nh, const double F[9], double thr_h, double straightness,
                        uint64_t seed, std::vector<double>& kept, uint64_t* draws);

// An engine for a helper outside any MultiH object: from the pool when one is idle on `device`, and back to it.
mh_engine* BorrowEngine(int device);
void ReturnEngine(int device, mh_engine* e);

} // namespace detail
} // namespace multih
