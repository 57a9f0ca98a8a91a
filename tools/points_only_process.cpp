// points_only_process.cpp — times MultiH::Process() on one scene, the point-only route (Process(src, dst)) next to the
// route with affinities (Process(src, dst, affines)), built and run by tools/points_only_bench.py.
//   points_only_process <x1 y1 x2 y2 a11 a12 a21 a22 per row> <calls> [F(9) e2(2) file]
// Routes: affine (Process with affinities, HAF refits), affine3pt (with affinities, SetEstimator(ESTIMATOR_3PT)), points
// (Process(src, dst)).  Prints one line per route and call: "<route> <call> <ms> <clusters> <labeling steps> <loop ms>
// <in RANSAC mask> <triangulated> <affine consistent>"; call 0 also pays for the HIP runtime.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "MultiH.h"

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: points_only_process <corr> <calls> [epipolar]\n"); return 2; }
    std::ifstream in(argv[1]);
    std::vector<cv::Point2d> src, dst;
    std::vector<cv::Mat> aff;
    double v[8];
    while (in >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> v[6] >> v[7]) {
        src.push_back(cv::Point2d(v[0], v[1]));
        dst.push_back(cv::Point2d(v[2], v[3]));
        cv::Mat A(2, 2, CV_64F);
        for (int q = 0; q < 4; ++q) A.at<double>(q / 2, q % 2) = v[4 + q];
        aff.push_back(A);
    }
    const int calls = std::atoi(argv[2]);
    double F[9], e2[2];
    bool have_epi = false;
    if (argc > 3) {
        std::ifstream ef(argv[3]);
        have_epi = true;
        for (double& x : F) have_epi = have_epi && static_cast<bool>(ef >> x);
        for (double& x : e2) have_epi = have_epi && static_cast<bool>(ef >> x);
    }
    const char* names[3] = { "affine", "affine3pt", "points" };
    for (int route = 0; route < 3; ++route) {
        for (int c = 0; c < calls; ++c) {
            MultiH mh(2.6, 2.2, 0.005, 0.5, 20);
            if (have_epi) mh.SetEpipolarGeometry(F, e2);
            mh.SetProposal(1234, 100000, 32);
            mh.SetFixedIterations(20);
            if (route == 1) mh.SetEstimator(MultiH::ESTIMATOR_3PT);
            const auto t0 = std::chrono::steady_clock::now();
            const bool ok = route < 2 ? mh.Process(src, dst, aff) : mh.Process(src, dst);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (!ok) { std::fprintf(stderr, "Process() failed\n"); return 1; }
            const MultiH::FrontStages st = mh.GetFrontStages();
            std::printf("%s %d %.3f %d %d %.3f %d %d %d\n", names[route], c, ms, mh.GetClusterNumber(), mh.GetLabelingStepsRun(),
                        1e3 * mh.GetLastLoopSeconds(), st.in_ransac_mask, st.triangulated, st.affine_consistent);
            mh.Release();
        }
    }
    return 0;
}
