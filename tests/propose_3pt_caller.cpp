// propose_3pt_caller.cpp — TEST: MultiH::PROPOSAL_SOURCE_3PT against an engine library WITHOUT mh_propose_3pt
// (tests/fake_engine.cpp, built on the CPU): the host class references the entry point weakly, so it links; the 3-point source
// fails with a message, an unknown source is refused, and the default route runs before and after as it did.
#include <cstdio>
#include <vector>

#include "MultiH.h"

extern "C" void fake_engine_set_mode(int mode);

static int run(int source, bool points_only, int& clusters)
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
    multiH->SetProposalSource(source, 16, 1);
    const bool ok = points_only ? multiH->Process(src, dst) : multiH->Process(src, dst, aff);
    clusters = ok ? multiH->GetClusterNumber() : -1;
    delete multiH;
    return ok ? 1 : 0;
}

int main()
{
    fake_engine_set_mode(0);
    int before = 0, c = 0, after = 0;
    if (run(MultiH::PROPOSAL_SOURCE_DLT, false, before) != 1 || before < 1) { std::printf("FAILED default route\n"); return 10; }
    if (run(MultiH::PROPOSAL_SOURCE_3PT, false, c) != 0) { std::printf("FAILED: 3PT ran without its entry point\n"); return 11; }
    if (run(MultiH::PROPOSAL_SOURCE_3PT, true, c) != 0) { std::printf("FAILED: point-only 3PT ran without its entry point\n"); return 12; }
    if (run(7, false, c) != 0) { std::printf("FAILED: source 7 accepted\n"); return 13; }
    if (run(MultiH::PROPOSAL_SOURCE_DLT, false, after) != 1 || after != before) { std::printf("FAILED default route afterwards\n"); return 14; }
    std::printf("propose_3pt_caller ok: clusters %d\n", before);
    return 0;
}
