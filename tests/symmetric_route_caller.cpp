// symmetric_route_caller.cpp — TEST: MultiH::SetResidual against an engine library WITHOUT mh_set_residual_mode and
// mh_set_residual_scope (tests/fake_engine.cpp, built on the CPU): the host class references both weakly, so it links; a forward
// Process() runs as before, the symmetric route fails with a message, an unknown value and the forward-only MSAC modes are
// refused, and the default route runs afterwards as it did.
#include <cstdio>
#include <vector>

#include "MultiH.h"

extern "C" void fake_engine_set_mode(int mode);

static int run(int residual, int tail_score, int& clusters)
{
    const int n = 60;
    std::vector<cv::Point2d> src, dst;
    std::vector<cv::Mat> aff;
    for (int i = 0; i < n; ++i) {      // (the points of tests/apply_multih_caller.cpp: two models of the stand-in engine)
        const double x = 10.0 + 7 * i + 3 * (i % 5), y = 20.0 + 37 * (i % 11);
        src.push_back(cv::Point2d(x, y));
        dst.push_back((i % 2) ? cv::Point2d((x + 300.0) / 1.3, (y + 600.0) / 1.3) : cv::Point2d(x, y));
        cv::Mat A(2, 2, CV_64F);
        A.at<double>(0, 0) = 1.0 + i; A.at<double>(0, 1) = 0.1; A.at<double>(1, 0) = -0.1; A.at<double>(1, 1) = 2.0 + i;
        aff.push_back(A);
    }
    MultiH* multiH = new MultiH(2.6, 2.2, 0.005, 0.5, 20);
    const double F[9] = { 0, -1, 2000, 1, 0, -1000, -2000, 1000, 0 }, e2[2] = { 1000, 2000 };
    multiH->SetEpipolarGeometry(F, e2);
    if (residual != -100) multiH->SetResidual(residual);
    multiH->SetTailScore(tail_score);
    const bool ok = multiH->Process(src, dst, aff);
    clusters = ok ? multiH->GetClusterNumber() : -1;
    delete multiH;
    return ok ? 1 : 0;
}

int main()
{
    fake_engine_set_mode(0);
    int before = 0, fwd = 0, c = 0, after = 0;
    if (run(-100, MultiH::TAIL_SCORE_COUNT, before) != 1 || before < 1) { std::printf("FAILED default route\n"); return 10; }
    if (run(MultiH::RESIDUAL_FORWARD, MultiH::TAIL_SCORE_COUNT, fwd) != 1 || fwd != before) { std::printf("FAILED forward route\n"); return 11; }
    if (run(MultiH::RESIDUAL_SYMMETRIC, MultiH::TAIL_SCORE_COUNT, c) != 0) { std::printf("FAILED: the symmetric route ran without its entry points\n"); return 12; }
    if (run(7, MultiH::TAIL_SCORE_COUNT, c) != 0) { std::printf("FAILED: residual 7 accepted\n"); return 13; }
    if (run(MultiH::RESIDUAL_SYMMETRIC, MultiH::TAIL_SCORE_MSAC, c) != 0) { std::printf("FAILED: symmetric with the MSAC tail accepted\n"); return 14; }
    if (run(-100, MultiH::TAIL_SCORE_COUNT, after) != 1 || after != before) { std::printf("FAILED default route afterwards\n"); return 15; }
    std::printf("symmetric_route_caller ok: clusters %d\n", before);
    return 0;
}
