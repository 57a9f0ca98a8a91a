// smooth_plan_caller.cpp — TEST: what MultiH::PlanRun makes of SetSmoothnessWeights, called directly as
// tests/process_plan_caller.cpp calls it: no engine is created, nothing is printed by the class.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>

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
    bool Plan(const EngineCaps& caps, RunPlan& plan, std::string& error) { return PlanRun(false, caps, plan, error); }
};

typedef std::function<void(Probe&)> Setup;

int failures = 0, checks = 0;

void Expect(const char* name, bool ok)
{
    ++checks;
    if (!ok) { std::printf("FAILED %s\n", name); ++failures; }
}

void Refused(const char* name, const MultiH::EngineCaps& caps, const Setup& setup, const std::string& message)
{
    Probe p;
    setup(p);
    MultiH::RunPlan plan;
    std::string error;
    ++checks;
    if (p.Plan(caps, plan, error)) { std::printf("FAILED %s: planned\n", name); ++failures; }
    else if (error != message + "\n") { std::printf("FAILED %s: \"%s\"\n", name, error.c_str()); ++failures; }
}

bool Planned(const char* name, const MultiH::EngineCaps& caps, const Setup& setup, MultiH::RunPlan& plan)
{
    Probe p;
    setup(p);
    std::string error;
    ++checks;
    if (p.Plan(caps, plan, error) && error.empty()) return true;
    std::printf("FAILED %s: \"%s\"\n", name, error.c_str());
    ++failures;
    return false;
}

std::string Range(const char* rho, int q_max)
{
    return std::string("Error: SetSmoothnessWeights: rho = ") + rho + ", q_max = " + std::to_string(q_max) + " (rho finite and > 0, q_max in [1, 256])";
}

} // namespace

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    MultiH::EngineCaps with, without;                  // `without`: the stand-in engine's (no optional entry point at all)
    with.smoothness_weights = true;
    const int C = MultiH::SMOOTHNESS_CAUCHY, U = MultiH::SMOOTHNESS_UNIFORM;

    Refused("rho 0", with, [=](Probe& p) { p.SetSmoothnessWeights(C, 0.0, 8); }, Range("0", 8));
    Refused("rho -3", with, [=](Probe& p) { p.SetSmoothnessWeights(C, -3.0, 8); }, Range("-3", 8));
    Refused("rho nan", with, [=](Probe& p) { p.SetSmoothnessWeights(C, nan, 8); }, Range("nan", 8));
    Refused("rho inf", with, [=](Probe& p) { p.SetSmoothnessWeights(C, inf, 8); }, Range("inf", 8));
    Refused("rho -inf", with, [=](Probe& p) { p.SetSmoothnessWeights(C, -inf, 8); }, Range("-inf", 8));
    Refused("q_max 0", with, [=](Probe& p) { p.SetSmoothnessWeights(C, 40.0, 0); }, Range("40", 0));
    Refused("q_max -1", with, [=](Probe& p) { p.SetSmoothnessWeights(C, 40.0, -1); }, Range("40", -1));
    Refused("q_max 257", with, [=](Probe& p) { p.SetSmoothnessWeights(C, 40.0, 257); }, Range("40", 257));
    Refused("rule 7", with, [=](Probe& p) { p.SetSmoothnessWeights(7, 40.0, 8); },
            "Error: unknown smoothness rule 7 (SMOOTHNESS_UNIFORM or SMOOTHNESS_CAUCHY)");
    Refused("no entry point", without, [=](Probe& p) { p.SetSmoothnessWeights(C, 40.0, 8); },
            "Error: the engine library has no distance-weighted smoothness (mh_set_smoothness_weights)");
    // the range is checked before the library is asked
    Refused("rho 0, no entry point", without, [=](Probe& p) { p.SetSmoothnessWeights(C, 0.0, 8); }, Range("0", 8));

    MultiH::RunPlan untouched, plan;
    if (Planned("default", without, [](Probe&) {}, untouched))
        Expect("default plan", untouched.smoothness_rule == MH_SMOOTH_UNIFORM && untouched.smoothness_rho == 0.0 && untouched.smoothness_q_max == 1);
    // UNIFORM plans exactly as before, against either library, and does not look at rho and q_max
    for (const MultiH::EngineCaps& caps : { with, without }) {
        if (Planned("uniform", caps, [=](Probe& p) { p.SetSmoothnessWeights(U, nan, -5); }, plan))
            Expect("uniform plan", plan.smoothness_rule == MH_SMOOTH_UNIFORM && plan.smoothness_rho == 0.0 && plan.smoothness_q_max == 1 &&
                                       plan.est == untouched.est && plan.initial_source == untouched.initial_source &&
                                       plan.iterative_source == untouched.iterative_source && plan.label_cost_beta == untouched.label_cost_beta &&
                                       plan.residual_mode == untouched.residual_mode && plan.residual_scope == untouched.residual_scope &&
                                       plan.estimator_reweight_rounds == untouched.estimator_reweight_rounds);
    }
    if (Planned("cauchy 40 8", with, [=](Probe& p) { p.SetSmoothnessWeights(C, 40.0, 8); }, plan))
        Expect("cauchy plan", plan.smoothness_rule == MH_SMOOTH_CAUCHY && plan.smoothness_rho == 40.0 && plan.smoothness_q_max == 8);
    if (Planned("cauchy default q_max", with, [=](Probe& p) { p.SetSmoothnessWeights(C, 0.5); }, plan))
        Expect("cauchy default plan", plan.smoothness_rule == MH_SMOOTH_CAUCHY && plan.smoothness_rho == 0.5 && plan.smoothness_q_max == 16);
    for (int q : { 1, 256 })
        if (Planned("cauchy q_max edge", with, [=](Probe& p) { p.SetSmoothnessWeights(C, 1e-300, q); }, plan))
            Expect("cauchy edge plan", plan.smoothness_q_max == q && plan.smoothness_rho == 1e-300);

    if (failures) { std::printf("smooth_plan_caller: %d of %d checks FAILED\n", failures, checks); return 1; }
    std::printf("smooth_plan_caller ok: %d checks\n", checks);
    return 0;
}
