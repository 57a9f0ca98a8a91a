// process_plan_caller.cpp — TEST: MultiH::PlanRun, the part of Process() that checks the settings against what the engine
// library offers and derives the run's plan from them, called directly: no engine is created, nothing is printed by the class.
// Every expected message is the text Process() has always written for that setting, copied literally.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "MultiH.h"
#include "multih_hip.h"

namespace {

struct Probe : MultiH {
    Probe() : MultiH(2.6, 2.2, 0.005, 0.5, 20)
    {
        for (int i = 0; i < 8; ++i) {
            src_points_original.push_back(cv::Point2d(10.0 * i, 3.0 * i * i));
            dst_points_original.push_back(cv::Point2d(10.0 * i + 1.0, 3.0 * i * i - 2.0));
            affinities_original.push_back(cv::Mat(2, 2, CV_64F));
        }
    }
    void DropFeatures() { dst_points_original.clear(); }
    bool Plan(bool points_only, const EngineCaps& caps, RunPlan& plan, std::string& error)
    {
        if (points_only) affinities_original.clear();
        return PlanRun(points_only, caps, plan, error);
    }
};

typedef std::function<void(Probe&)> Setup;
typedef bool MultiH::EngineCaps::*Cap;

const Cap ALL_CAPS[] = { &MultiH::EngineCaps::point_only, &MultiH::EngineCaps::fundamental_minimal, &MultiH::EngineCaps::set_sampler,
                         &MultiH::EngineCaps::sample_neighbours, &MultiH::EngineCaps::data_term, &MultiH::EngineCaps::residual_route,
                         &MultiH::EngineCaps::msac_scores, &MultiH::EngineCaps::get_model, &MultiH::EngineCaps::refit,
                         &MultiH::EngineCaps::polish, &MultiH::EngineCaps::reweight, &MultiH::EngineCaps::estimator_reweighting,
                         &MultiH::EngineCaps::reweight_auto, &MultiH::EngineCaps::estimator_reweighting_auto,
                         &MultiH::EngineCaps::select_greedy_msac, &MultiH::EngineCaps::propose_haf, &MultiH::EngineCaps::propose_3pt,
                         &MultiH::EngineCaps::compat_dlt, &MultiH::EngineCaps::energy_merge, &MultiH::EngineCaps::drop_deltas };

MultiH::EngineCaps Everything()
{
    MultiH::EngineCaps c;
    for (Cap cap : ALL_CAPS) c.*cap = true;
    return c;
}

MultiH::EngineCaps AllBut(Cap cap)
{
    MultiH::EngineCaps c = Everything();
    c.*cap = false;
    return c;
}

int failures = 0, checks = 0;

// the plan is refused with exactly `message` (and a line feed)
void Refused(const char* name, const MultiH::EngineCaps& caps, bool points_only, const Setup& setup, const std::string& message)
{
    Probe p;
    setup(p);
    MultiH::RunPlan plan;
    std::string error;
    ++checks;
    if (p.Plan(points_only, caps, plan, error)) { std::printf("FAILED %s: planned\n", name); ++failures; }
    else if (error != message + "\n") { std::printf("FAILED %s: \"%s\"\n", name, error.c_str()); ++failures; }
}

bool Planned(const char* name, const MultiH::EngineCaps& caps, bool points_only, const Setup& setup, MultiH::RunPlan& plan)
{
    Probe p;
    setup(p);
    std::string error;
    ++checks;
    if (p.Plan(points_only, caps, plan, error) && error.empty()) return true;
    std::printf("FAILED %s: \"%s\"\n", name, error.c_str());
    ++failures;
    return false;
}

void Expect(const char* name, bool ok)
{
    ++checks;
    if (!ok) { std::printf("FAILED %s\n", name); ++failures; }
}

const char* const NO_FINAL_ROUNDS = "Error: reweighting rounds 17 (final) / 0 (estimator) outside [0, 16]";
const char* const COMPAT_RANGE = "Error: SetCompatibilityFit: trials outside [1, 4096] or a limit scale that is negative or not finite";
const char* const LABEL_COST_VALUE = "Error: the label cost must be finite and not negative (SetLabelCost)";
const char* const MSAC_FORWARD_ONLY =
    "Error: the MSAC weights (TAIL_SCORE_MSAC, SELECTION_SCORE_MSAC) measure the forward error only; they do not combine with RESIDUAL_SYMMETRIC";
const char* const NO_POINT_ONLY = "Error: the engine library has no point-only entry points (mh_set_estimator, mh_refine_points)";

void OneWrongSetting()
{
    const MultiH::EngineCaps all = Everything();
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Refused("estimator 7", all, false, [](Probe& p) { p.SetEstimator(7); }, "Error: unknown estimator 7 (ESTIMATOR_HAF, ESTIMATOR_3PT or ESTIMATOR_DLT)");
    Refused("compat fit 7", all, false, [](Probe& p) { p.SetCompatibilityFit(7); }, "Error: unknown compatibility fit 7 (COMPAT_FIT_3PT or COMPAT_FIT_DLT)");
    Refused("merge mode 7", all, false, [](Probe& p) { p.SetMergeMode(7); }, "Error: unknown merge mode (SetMergeMode)");
    Refused("residual 7", all, false, [](Probe& p) { p.SetResidual(7); }, "Error: unknown residual 7 (RESIDUAL_FORWARD or RESIDUAL_SYMMETRIC)");
    Refused("tail score 7", all, false, [](Probe& p) { p.SetTailScore(7); }, "Error: unknown tail score 7 (TAIL_SCORE_COUNT or TAIL_SCORE_MSAC)");
    Refused("selection score 7", all, false, [](Probe& p) { p.SetSelectionScore(7); },
            "Error: unknown selection score 7 (SELECTION_SCORE_COUNT or SELECTION_SCORE_MSAC)");
    Refused("proposal source 7", all, false, [](Probe& p) { p.SetProposalSource(7); },
            "Error: unknown proposal source 7 (PROPOSAL_SOURCE_DLT or PROPOSAL_SOURCE_HAF)");
    Refused("compat trials 0", all, false, [](Probe& p) { p.SetCompatibilityFit(MultiH::COMPAT_FIT_DLT, 0); }, COMPAT_RANGE);
    Refused("compat trials 4097", all, false, [](Probe& p) { p.SetCompatibilityFit(MultiH::COMPAT_FIT_DLT, 4097); }, COMPAT_RANGE);
    Refused("compat limit -1", all, false, [](Probe& p) { p.SetCompatibilityFit(MultiH::COMPAT_FIT_DLT, 501, -1.0); }, COMPAT_RANGE);
    Refused("compat limit inf", all, false, [inf](Probe& p) { p.SetCompatibilityFit(MultiH::COMPAT_FIT_DLT, 501, inf); }, COMPAT_RANGE);
    for (int members : { 1, 2, 33 })
        Refused("HAF members", all, false, [members](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_HAF, members); },
                "Error: SetProposalSource: members = " + std::to_string(members) + ", stride = 1 (members 0 or in [3, 32], stride >= 1)");
    Refused("HAF stride 0", all, false, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_HAF, 16, 0); },
            "Error: SetProposalSource: members = 16, stride = 0 (members 0 or in [3, 32], stride >= 1)");
    Refused("HAF members above k", all, false,
            [](Probe& p) { p.SetProposalSampler(MultiH::PROPOSAL_LOCAL, 8); p.SetProposalSource(MultiH::PROPOSAL_SOURCE_HAF, 16); },
            "Error: SetProposalSource: members = 16 exceeds k = 8 of the local sampler, whose table the HAF proposals share");
    Refused("tail refit 17", all, false, [](Probe& p) { p.SetTailRefit(17); }, "Error: tail refit iterations 17 outside [0, 16]");
    Refused("tail polish 33", all, false, [](Probe& p) { p.SetTailPolish(33); }, "Error: tail polish iterations 33 outside [0, 32]");
    Refused("model polish 33", all, false, [](Probe& p) { p.SetModelPolish(33); }, "Error: model polish iterations 33 outside [0, 32]");
    Refused("reweighting rounds 17", all, false, [](Probe& p) { p.SetModelReweight(17); }, NO_FINAL_ROUNDS);
    Refused("reweighting scale -1", all, false, [](Probe& p) { p.SetModelReweight(2, -1.0); },
            "Error: reweighting scale -1 (final) / 0 (estimator) is not a finite number >= 0");
    Refused("kappa NaN", all, false, [nan](Probe& p) { p.SetModelReweightAuto(2, nan); },
            "Error: self-scaled reweighting kappa nan (final) / 0 (estimator) is not a finite number >= 0");
    Refused("fixed and self-scaled, final", all, false, [](Probe& p) { p.SetModelReweight(2); p.SetModelReweightAuto(2); },
            "Error: both the fixed and the self-scaled reweighting are set for the final refit; choose one");
    Refused("fixed and self-scaled, estimator", all, false, [](Probe& p) { p.SetEstimatorReweight(2); p.SetEstimatorReweightAuto(2); },
            "Error: both the fixed and the self-scaled reweighting are set for the estimator; choose one");
    Refused("label cost -1", all, false, [](Probe& p) { p.SetMergeMode(MultiH::MERGE_ENERGY); p.SetLabelCost(-1.0); }, LABEL_COST_VALUE);
    Refused("label cost NaN", all, false, [nan](Probe& p) { p.SetMergeMode(MultiH::MERGE_ENERGY); p.SetLabelCost(nan); }, LABEL_COST_VALUE);
    Refused("label cost without MERGE_ENERGY", all, false, [](Probe& p) { p.SetLabelCost(40.0); },
            "Error: a label cost needs the energy-tested merge (SetLabelCost with SetMergeMode(MERGE_ENERGY))");
    Refused("label cost too large", all, false, [](Probe& p) { p.SetMergeMode(MultiH::MERGE_ENERGY); p.SetLabelCost(1e300); },
            "Error: the label cost is too large (SetLabelCost)");
    Refused("symmetric with the MSAC tail", all, false,
            [](Probe& p) { p.SetResidual(MultiH::RESIDUAL_SYMMETRIC); p.SetTailScore(MultiH::TAIL_SCORE_MSAC); }, MSAC_FORWARD_ONLY);
    Refused("symmetric with MSAC selection", all, false,
            [](Probe& p) { p.SetResidual(MultiH::RESIDUAL_SYMMETRIC); p.SetSelectionScore(MultiH::SELECTION_SCORE_MSAC); }, MSAC_FORWARD_ONLY);
    Refused("stable sets, point-only", all, true, [](Probe& p) { p.SetInitialisation(MultiH::INIT_STABLE_SETS); },
            "Error: the stable point sets (INIT_STABLE_SETS) need affinities; the point-only Process() cannot use them");
    Refused("stable sets, epipolar-free", all, false, [](Probe& p) { p.SetInitialisation(MultiH::INIT_STABLE_SETS); p.SetEpipolarFree(true); },
            "Error: the stable point sets (INIT_STABLE_SETS) need the fundamental matrix; the epipolar-free route (SetEpipolarFree) cannot use them");
    Refused("HAF proposals, point-only", all, true, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_HAF); },
            "Error: HAF proposals (PROPOSAL_SOURCE_HAF) need affinities; the point-only Process() cannot use them");
    Refused("HAF proposals, epipolar-free", all, false, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_HAF); p.SetEpipolarFree(true); },
            "Error: HAF proposals (PROPOSAL_SOURCE_HAF) need the fundamental matrix; the epipolar-free route (SetEpipolarFree) cannot use them");
    Refused("3-point proposals, epipolar-free", all, false, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_3PT); p.SetEpipolarFree(true); },
            "Error: 3-point proposals (PROPOSAL_SOURCE_3PT) need the fundamental matrix; the epipolar-free route (SetEpipolarFree) cannot use them");
    Refused("no features", all, false, [](Probe& p) { p.DropFeatures(); }, "Error: Features are not set!");
}

// every mode whose entry points PlanRun looks for: refused by a library that lacks just those, and by one that has none at all
// where no other missing entry point comes first
void MissingEntryPoints()
{
    struct Mode { const char* name; Cap cap; bool points_only, alone_too; Setup setup; const char* message; };
    const Mode modes[] = {
        { "COMPAT_FIT_DLT", &MultiH::EngineCaps::compat_dlt, false, true, [](Probe& p) { p.SetCompatibilityFit(MultiH::COMPAT_FIT_DLT); },
          "Error: the engine library has no compatibility check with 4-point trials (mh_compat_dlt_medians)" },
        { "PROPOSAL_SOURCE_3PT", &MultiH::EngineCaps::propose_3pt, false, true, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_3PT); },
          "Error: the engine library has no 3-point proposals (mh_propose_3pt)" },
        { "PROPOSAL_SOURCE_HAF", &MultiH::EngineCaps::propose_haf, false, true, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_HAF); },
          "Error: the engine library has no HAF proposals (mh_propose_haf)" },
        { "point-only", &MultiH::EngineCaps::point_only, true, true, [](Probe&) {}, NO_POINT_ONLY },
        { "ESTIMATOR_3PT", &MultiH::EngineCaps::point_only, false, true, [](Probe& p) { p.SetEstimator(MultiH::ESTIMATOR_3PT); }, NO_POINT_ONLY },
        { "ESTIMATOR_DLT", &MultiH::EngineCaps::point_only, false, true, [](Probe& p) { p.SetEstimator(MultiH::ESTIMATOR_DLT); }, NO_POINT_ONLY },
        { "epipolar-free", &MultiH::EngineCaps::point_only, false, true, [](Probe& p) { p.SetEpipolarFree(true); }, NO_POINT_ONLY },
        { "MERGE_ENERGY", &MultiH::EngineCaps::energy_merge, false, true, [](Probe& p) { p.SetMergeMode(MultiH::MERGE_ENERGY); },
          "Error: the engine library has no energy-tested merge (mh_merge_deltas, mh_labeling_energy)" },
        { "label cost", &MultiH::EngineCaps::drop_deltas, false, false, [](Probe& p) { p.SetMergeMode(MultiH::MERGE_ENERGY); p.SetLabelCost(40.0); },
          "Error: the engine library has no label-drop evaluation (mh_drop_deltas)" },
        { "DATA_TERM_RISING", &MultiH::EngineCaps::data_term, false, true, [](Probe& p) { p.SetDataTerm(MultiH::DATA_TERM_RISING); },
          "Error: the engine library has no selectable data term (mh_set_data_term)" },
        { "RESIDUAL_SYMMETRIC", &MultiH::EngineCaps::residual_route, false, true, [](Probe& p) { p.SetResidual(MultiH::RESIDUAL_SYMMETRIC); },
          "Error: the engine library has no symmetric route (mh_set_residual_mode, mh_set_residual_scope)" },
        { "TAIL_SCORE_MSAC", &MultiH::EngineCaps::msac_scores, false, true, [](Probe& p) { p.SetTailScore(MultiH::TAIL_SCORE_MSAC); },
          "Error: the engine library has no MSAC scores (mh_score_msac, mh_select_best_msac, mh_get_model)" },
        { "TAIL_SCORE_MSAC, no read-back", &MultiH::EngineCaps::get_model, false, false, [](Probe& p) { p.SetTailScore(MultiH::TAIL_SCORE_MSAC); },
          "Error: the engine library has no MSAC scores (mh_score_msac, mh_select_best_msac, mh_get_model)" },
        { "tail refit", &MultiH::EngineCaps::refit, false, true, [](Probe& p) { p.SetTailRefit(1); },
          "Error: the engine library has no homography refit (mh_refit_homography, mh_get_model)" },
        { "tail refit, no read-back", &MultiH::EngineCaps::get_model, false, false, [](Probe& p) { p.SetTailRefit(1); },
          "Error: the engine library has no homography refit (mh_refit_homography, mh_get_model)" },
        { "tail polish", &MultiH::EngineCaps::polish, false, true, [](Probe& p) { p.SetTailPolish(10); },
          "Error: the engine library has no homography polish (mh_polish_homographies)" },
        { "model polish", &MultiH::EngineCaps::polish, false, true, [](Probe& p) { p.SetModelPolish(10); },
          "Error: the engine library has no homography polish (mh_polish_homographies)" },
        { "tail polish, no read-back", &MultiH::EngineCaps::get_model, false, false, [](Probe& p) { p.SetTailPolish(10); },
          "Error: the engine library has no single-model read-back for the tail's polish (mh_get_model)" },
        { "model reweight", &MultiH::EngineCaps::reweight, false, true, [](Probe& p) { p.SetModelReweight(2); },
          "Error: the engine library has no reweighted refit (mh_reweight_homographies)" },
        { "estimator reweight", &MultiH::EngineCaps::estimator_reweighting, false, false,
          [](Probe& p) { p.SetEstimator(MultiH::ESTIMATOR_DLT); p.SetEstimatorReweight(2); },
          "Error: the engine library has no reweighted estimator (mh_set_estimator_reweighting)" },
        { "model reweight, self-scaled", &MultiH::EngineCaps::reweight_auto, false, true, [](Probe& p) { p.SetModelReweightAuto(2); },
          "Error: the engine library has no self-scaled reweighted refit (mh_reweight_homographies_auto)" },
        { "estimator reweight, self-scaled", &MultiH::EngineCaps::estimator_reweighting_auto, false, false,
          [](Probe& p) { p.SetEstimator(MultiH::ESTIMATOR_DLT); p.SetEstimatorReweightAuto(2); },
          "Error: the engine library has no self-scaled reweighted estimator (mh_set_estimator_reweighting_auto)" },
        { "SELECTION_SCORE_MSAC", &MultiH::EngineCaps::select_greedy_msac, false, true, [](Probe& p) { p.SetSelectionScore(MultiH::SELECTION_SCORE_MSAC); },
          "Error: the engine library has no selection ranked by MSAC weight (mh_select_greedy_msac)" },
    };
    for (const Mode& m : modes) {
        Refused(m.name, AllBut(m.cap), m.points_only, m.setup, m.message);
        if (m.alone_too) Refused(m.name, MultiH::EngineCaps(), m.points_only, m.setup, m.message);
        MultiH::RunPlan plan;
        Planned(m.name, Everything(), m.points_only, m.setup, plan);
    }
    // nothing optional is needed by the defaults, and the estimator's rounds need no entry point while the estimator is not the DLT
    MultiH::RunPlan plan;
    if (Planned("defaults, no entry points", MultiH::EngineCaps(), false, [](Probe&) {}, plan)) Expect("defaults: HAF", plan.est == MH_ESTIMATOR_HAF);
    if (Planned("estimator rounds under HAF, no entry points", MultiH::EngineCaps(), false, [](Probe& p) { p.SetEstimatorReweight(3); }, plan))
        Expect("no rounds under HAF", plan.estimator_reweight_rounds == 0 && !plan.estimator_reweight_auto);
}

// two wrong settings: the message is that of the check that has always come first
void Order()
{
    const MultiH::EngineCaps all = Everything();
    Refused("estimator before compat fit", all, false, [](Probe& p) { p.SetCompatibilityFit(7); p.SetEstimator(7); },
            "Error: unknown estimator 7 (ESTIMATOR_HAF, ESTIMATOR_3PT or ESTIMATOR_DLT)");
    Refused("residual before tail score", all, false, [](Probe& p) { p.SetTailScore(7); p.SetResidual(7); },
            "Error: unknown residual 7 (RESIDUAL_FORWARD or RESIDUAL_SYMMETRIC)");
    Refused("tail refit before tail polish", all, false, [](Probe& p) { p.SetTailPolish(33); p.SetTailRefit(17); },
            "Error: tail refit iterations 17 outside [0, 16]");
    Refused("merge mode before label cost", all, false, [](Probe& p) { p.SetLabelCost(-1.0); p.SetMergeMode(7); }, "Error: unknown merge mode (SetMergeMode)");
    Refused("compat fit before proposal source", all, false, [](Probe& p) { p.SetProposalSource(7); p.SetCompatibilityFit(7); },
            "Error: unknown compatibility fit 7 (COMPAT_FIT_3PT or COMPAT_FIT_DLT)");
    Refused("label cost before data term's entry point", AllBut(&MultiH::EngineCaps::data_term), false,
            [](Probe& p) { p.SetDataTerm(MultiH::DATA_TERM_RISING); p.SetLabelCost(-1.0); }, LABEL_COST_VALUE);
    Refused("fixed rounds before self-scaled rounds", all, false, [](Probe& p) { p.SetModelReweightAuto(17); p.SetModelReweight(17); }, NO_FINAL_ROUNDS);
    Refused("self-scaled rounds before selection score", all, false, [](Probe& p) { p.SetSelectionScore(7); p.SetModelReweightAuto(17); },
            "Error: self-scaled reweighting rounds 17 (final) / 0 (estimator) outside [0, 16]");
}

void PlanValues()
{
    const MultiH::EngineCaps all = Everything();
    MultiH::RunPlan plan;
    if (Planned("HAF", all, false, [](Probe&) {}, plan))
        Expect("HAF: plan", plan.est == MH_ESTIMATOR_HAF && !plan.points_only && plan.initial_source == MultiH::PROPOSAL_SOURCE_DLT &&
                                plan.iterative_source == MultiH::PROPOSAL_SOURCE_DLT && plan.label_cost_beta == 0 &&
                                plan.residual_mode == MH_RESIDUAL_FORWARD && plan.residual_scope == MH_RESIDUAL_SCOPE_SCORE &&
                                plan.estimator_reweight_rounds == 0);
    if (Planned("point-only", all, true, [](Probe& p) { p.SetEstimatorReweight(3); }, plan))
        Expect("point-only: 3PT, no rounds", plan.est == MH_ESTIMATOR_3PT && plan.points_only && plan.estimator_reweight_rounds == 0);
    if (Planned("point-only with the DLT", all, true, [](Probe& p) { p.SetEstimator(MultiH::ESTIMATOR_DLT); }, plan))
        Expect("point-only with the DLT", plan.est == MH_ESTIMATOR_DLT);
    if (Planned("ESTIMATOR_3PT", all, false, [](Probe& p) { p.SetEstimator(MultiH::ESTIMATOR_3PT); p.SetEstimatorReweightAuto(3); }, plan))
        Expect("ESTIMATOR_3PT: no rounds", plan.est == MH_ESTIMATOR_3PT && plan.estimator_reweight_rounds == 0 && !plan.estimator_reweight_auto);
    if (Planned("epipolar-free", all, false, [](Probe& p) { p.SetEpipolarFree(true); p.SetEstimatorReweight(3, 1.5); }, plan))
        Expect("epipolar-free: DLT with fixed rounds", plan.est == MH_ESTIMATOR_DLT && plan.estimator_reweight_rounds == 3 &&
                                                       !plan.estimator_reweight_auto && plan.estimator_reweight_c2 == 1.5 * 1.5);
    if (Planned("ESTIMATOR_DLT, self-scaled", all, false, [](Probe& p) { p.SetEstimator(MultiH::ESTIMATOR_DLT); p.SetEstimatorReweightAuto(4); }, plan))
        Expect("ESTIMATOR_DLT: self-scaled rounds", plan.est == MH_ESTIMATOR_DLT && plan.estimator_reweight_rounds == 4 &&
                                                    plan.estimator_reweight_auto && plan.estimator_reweight_c2 == 2.2 * 2.2);
    if (Planned("symmetric", all, false, [](Probe& p) { p.SetResidual(MultiH::RESIDUAL_SYMMETRIC); }, plan))
        Expect("symmetric: mode and scope", plan.residual_mode == MH_RESIDUAL_SYMMETRIC && plan.residual_scope == MH_RESIDUAL_SCOPE_ROUTE);
    if (Planned("HAF proposals", all, false, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_HAF); }, plan))
        Expect("HAF proposals: the initial batch only", plan.initial_source == MultiH::PROPOSAL_SOURCE_HAF &&
                                                        plan.iterative_source == MultiH::PROPOSAL_SOURCE_DLT);
    if (Planned("3-point proposals, point-only", all, true, [](Probe& p) { p.SetProposalSource(MultiH::PROPOSAL_SOURCE_3PT); }, plan))
        Expect("3-point proposals: every batch", plan.initial_source == MultiH::PROPOSAL_SOURCE_3PT &&
                                                 plan.iterative_source == MultiH::PROPOSAL_SOURCE_3PT);
    if (Planned("given models ignore the source", all, false,
                [](Probe& p) { p.SetProposalSource(7); p.SetInitialHomographies(std::vector<cv::Mat>(1, cv::Mat(3, 3, CV_64F))); }, plan))
        Expect("given models: DLT batches", plan.initial_source == MultiH::PROPOSAL_SOURCE_DLT);
    // the label cost in energy units at lambda 0.5, thr_hom 2.2: printed for the test to compare with tests/label_cost_numpy.py
    for (double points : { 40.0, 0.5 })
        if (Planned("label cost", all, false, [points](Probe& p) { p.SetMergeMode(MultiH::MERGE_ENERGY); p.SetLabelCost(points); }, plan))
            std::printf("beta %.17g %lld\n", points, plan.label_cost_beta);
}

} // namespace

int main()
{
    OneWrongSetting();
    MissingEntryPoints();
    Order();
    PlanValues();
    if (failures) { std::printf("process_plan_caller: %d of %d checks FAILED\n", failures, checks); return 1; }
    std::printf("process_plan_caller ok: %d checks\n", checks);
    return 0;
}
