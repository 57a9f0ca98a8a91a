// main.cpp — command-line harness around class MultiH, following the call order of the
// reference's ApplyMultiH (M/main.cpp:232-311): load correspondences (8 numbers per line,
// M/main.cpp:380-412) -> MultiH ctor -> Process -> GetLabels -> GetIterationNumber ->
// GetClusterNumber -> getters -> SavePointsToFile (9 numbers per line, :429-446).
// No imread / DrawClusters / imshow / waitKey (SURVEY A-11: the reference blocks on a key press).
//
//   multih_harness <in_corr.txt> <out_result.txt> [--epipolar <file with F(9) e2x e2y>]
//                  [--thrF 2.6] [--thrH 2.2] [--locality 0.005] [--lambda 0.5] [--min-inliers 20]
//                  [--hypotheses 10000] [--max-models 32] [--seed 1234] [--iterations 0]
//                  [--neighbourhood knn|radius|approx]   (knn, the default: the 16 nearest hits within 1/locality pixels; radius: every hit within
//                  it; approx: what FLANN's default search — 4 randomised KD-trees, 32 checks — finds of them, MultiH::SetNeighbourApprox)
//                  [--load-filter 2.0]   r06: the filter of the reference's LoadPointsFromFile (M/main.cpp:399-409:
//                                findFundamentalMat(CV_FM_RANSAC, 2.0, 0.99) and the erase loop) through the engine's own estimator
//                                (multih::FilterCorrespondencesByEpipolarGeometry); the value is the threshold in pixels, 0 switches
//                                the filter off (what the harness did until r05)
//                  [--f-metric opencv|sampson]   what the two F estimations compare with their thresholds (MultiH::SetFundamentalMetric)
//                  [--f-estimator ls8|minimal]   which estimator the two F estimations run (MultiH::SetFundamentalEstimator): ls8, the
//                                default, scores 8-point fits and refits the best twice; minimal is the scheme of the reference's
//                                findFundamentalMat call: at most 1 000 7-point samples, confidence 0.99, no refit
//                  [--stages <file>]   write the stage table as one JSON object: rows loaded, after the load filter, in
//                                Process()'s RANSAC mask, after OptimalTriangulation, after distanceError <= 1 (M/MultiH.cpp:807-838)
//                  [--points]   point-only correspondences: 4 numbers per input row (x1 y1 x2 y2, no affinity) and 5 per output
//                                row (x1 y1 x2 y2 label); runs MultiH::Process(src, dst), the point-only route (3-point refits)
//                  [--estimator haf|3pt|dlt]   the re-estimator of the route with affinities (MultiH::SetEstimator; haf, the default,
//                                is the reference's); --points takes 3pt unless dlt (the N-point DLT, which reads no F) is asked for
//                  [--no-epipolar]   the route without epipolar geometry (MultiH::SetEpipolarFree): no F is estimated, no row is
//                                filtered (the load filter included), DLT refits, medoid merge candidates, no compatibility check
//                                (unless --compat-fit dlt)
//                  [--compat-fit dlt[:trials[:limit_scale]]]   the post-filter's trials are 4-point DLT fits, which need no F
//                                (MultiH::SetCompatibilityFit): it then runs on either route, trials per cluster (default 501, at
//                                most 4096), a cluster going when its statistic exceeds limit_scale * thrH^2 (default: the
//                                measured 256); "Compatibility check (4-point trials) .. clusters removed" reports it
//                  [--data-term reference|rising]   the data term of the labeling (MultiH::SetDataTerm): reference, the default, is
//                                the reference's dataEnergy (the cost falls as the fit gets worse); rising drops its `1.0 -`
//                  [--smoothness uniform|cauchy:RHO[:QMAX]]   the weight of a neighbour pair in the smoothness term
//                                (MultiH::SetSmoothnessWeights): uniform, the default, is the reference's (hit multiplicity);
//                                cauchy multiplies it by max(1, round(QMAX RHO^2 / (RHO^2 + d))), d the pair's squared distance in
//                                (x1,y1,x2,y2), RHO in pixels, QMAX in [1, 256] (default 16)
//                  [--merge meanshift|energy]   how MergingStep decides (MultiH::SetMergeMode): meanshift, the default, is the
//                                reference's rule; energy joins two labels only where the union with its own N-point refit lowers
//                                the labeling's energy (mh_merge_deltas), and the LabelingStep behind it starts warm; "Energy merges:"
//                                reports the steps' totals
//                  [--label-cost P]   the cost of a label in use, in outliers' worth (MultiH::SetLabelCost; needs --merge energy):
//                                joins are taken iff delta - beta < 0, and behind them at most one label per step is dropped
//                                (mh_drop_deltas) where that lowers the energy with the cost; default 0; "Label cost:" reports
//                                the drops
//                  [--residual forward|symmetric]   the error of the whole route (MultiH::SetResidual): forward, the default, is the
//                                reference's one-way transfer error; symmetric adds the backward term through adj(H) — proposals
//                                are scored and selected, clusters merged, points labelled and the tail finished by it at thrH,
//                                unscaled; not together with --tail-score msac or --select-score msac
//                  [--tail-score count|msac]   how the degenerate tail ranks its DLT hypotheses (MultiH::SetTailScore): count, the
//                                default, by inlier count; msac by the fit-weighted score of mh_score_msac
//                  [--tail-refit N]   the degenerate tail refits its winner to all its inliers, at most N rounds (MultiH::SetTailRefit;
//                                0, the default, returns the 4-point hypothesis; N <= 16)
//                  [--tail-polish N]  the degenerate tail polishes its result — the winner, refitted when --tail-refit says so — by at
//                                most N Levenberg-Marquardt iterations on the transfer error of its inliers (MultiH::SetTailPolish;
//                                0, the default, off; N <= 32); --tail-refit 1 --tail-polish 10 is cv::findHomography's sequence
//                  [--polish N]       every final cluster's homography polished the same way over its labelled correspondences
//                                (MultiH::SetModelPolish; 0, the default, off; N <= 32)
//                  [--reweight n[:scale]]   every final cluster's homography refitted by n reweighted N-point DLT rounds over its
//                                labelled correspondences, weights 1 - d2 / scale^2 (MultiH::SetModelReweight; 0, the default, off;
//                                n <= 16; scale in pixels, default thrH); runs in front of --polish
//                  [--estimator-reweight n[:scale]]   the same rounds as the loop's re-estimator under --estimator dlt and
//                                --no-epipolar (MultiH::SetEstimatorReweight; 0, the default, off)
//                  [--reweight-auto n[:kappa]] [--estimator-reweight-auto n[:kappa]]   the same two with the scale of every round
//                                taken from the data: kappa^2 times the lower median of the label's squared transfer errors
//                                (MultiH::SetModelReweightAuto / SetEstimatorReweightAuto; default kappa^2 = log2(100)); an option
//                                and its -auto twin, both with n > 0, are refused
//                  [--select-score count|msac]   how the proposal batches are ranked (MultiH::SetSelectionScore): count, the default,
//                                by inlier count (mh_select_greedy); msac by the MSAC weight among the hypotheses with enough
//                                inliers (mh_select_greedy_msac)
//                  [--sampler uniform|local[:k[:u]]]   the sampler of the proposal batches (MultiH::SetProposalSampler): uniform
//                                4-tuples (default) or neighbourhood-guided ones from the k nearest neighbours (32) with u of
//                                every 16 hypotheses left uniform (4)
//                  [--proposals dlt|haf[:members[:stride]]|3pt]   where the initial hypotheses come from (MultiH::SetProposalSource): dlt,
//                                the default, 4-point DLT hypotheses from sampled tuples; haf one hypothesis per `stride`-th affine
//                                correspondence (1), refitted to its consistent ones among `members` nearest neighbours (16; 0 = none);
//                                3pt (no arguments) F-constrained 3-point hypotheses from the first three indices of the DLT route's
//                                tuples, for the initial and the iterative batches; works with --points
//                  [--ranks N]   one process per GPU (rank r on device r), the hypothesis batches sharded over the ranks and
//                                exchanged by RCCL (host/rccl_transport.cpp: ncclAllGather on the engine's stream); this
//                                process becomes rank 0 and starts the others before anything touches the GPU.  Every rank
//                                computes the same result; rank 0 writes <out_result.txt>, rank r > 0 <out_result.txt>.rank<r>.
//                                N = 1 runs the same protocol on a one-rank communicator.
// Defaults are the harness defaults of the reference (M/main.cpp:55-59).
#include <algorithm>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <sys/wait.h>
#include <poll.h>
#include <unistd.h>

#include "MultiH.h"
#include "multih_rccl.h"

// M/main.cpp:380-412.  filter_threshold > 0: the load-time F-RANSAC filter of :399-409 (see MultiH.h,
// multih::FilterCorrespondencesByEpipolarGeometry); *loaded = rows read from the file.
static bool LoadPointsFromFile(std::vector<cv::Point2d>& srcPoints, std::vector<cv::Point2d>& dstPoints,
                               std::vector<cv::Mat>& affines, const char* file, double filter_threshold,
                               unsigned long long seed, int metric, int device, int* loaded, bool points_only,
                               const MultiH::FundEstimator& estimator)
{
    std::ifstream infile(file);
    if (!infile.is_open()) return false;
    double x1, y1, x2, y2, a1, a2, a3, a4;
    if (points_only)                                                 // --points: x1 y1 x2 y2 per row, affines stays empty
        while (infile >> x1 >> y1 >> x2 >> y2) {
            srcPoints.push_back(cv::Point2d(x1, y1));
            dstPoints.push_back(cv::Point2d(x2, y2));
        }
    else while (infile >> x1 >> y1 >> x2 >> y2 >> a1 >> a2 >> a3 >> a4) {
        srcPoints.push_back(cv::Point2d(x1, y1));
        dstPoints.push_back(cv::Point2d(x2, y2));
        const double a[4] = { a1, a2, a3, a4 };
        cv::Mat A(2, 2, CV_64F);                                     // owns its storage (M/main.cpp:394 builds a Mat_<double>)
        for (int q = 0; q < 4; ++q) A.at<double>(q / 2, q % 2) = a[q];
        affines.push_back(A);
    }
    if (loaded) *loaded = (int)srcPoints.size();
    if (filter_threshold > 0.0 && srcPoints.size() >= 8 &&
        !multih::FilterCorrespondencesByEpipolarGeometry(srcPoints, dstPoints, affines, filter_threshold,
                                                         seed ^ 0x10adf117e4ull, 4000, metric, device, nullptr, estimator))
        return false;
    return true;
}

static bool SavePointsToFile(std::vector<cv::Point2d>& srcPoints, std::vector<cv::Point2d>& dstPoints,
                             std::vector<cv::Mat>& affines, std::vector<int>& labels, const char* file)
{
    std::ofstream outfile(file, std::ios::out);
    if (!outfile.is_open()) return false;
    if (affines.empty()) {                                           // the point-only route: x1 y1 x2 y2 label
        for (size_t i = 0; i < srcPoints.size(); ++i)
            outfile << srcPoints[i].x << " " << srcPoints[i].y << " " << dstPoints[i].x << " " << dstPoints[i].y << " " << labels[i]
                    << std::endl;
        return true;
    }
    for (size_t i = 0; i < srcPoints.size(); ++i)
        outfile << srcPoints[i].x << " " << srcPoints[i].y << " " << dstPoints[i].x << " " << dstPoints[i].y << " "
                << affines[i].at<double>(0, 0) << " " << affines[i].at<double>(0, 1) << " "
                << affines[i].at<double>(1, 0) << " " << affines[i].at<double>(1, 1) << " " << labels[i] << std::endl;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::cerr << "usage: multih_harness <in_corr.txt> <out_result.txt> [--epipolar file] [--thrF v] [--thrH v] "
                     "[--locality v] [--lambda v] [--min-inliers n] [--hypotheses n] [--max-models n] [--seed n] "
                     "[--iterations n] [--neighbourhood knn|radius|approx] [--load-filter px] [--f-metric opencv|sampson] [--f-estimator ls8|minimal] "
                     "[--stages file] [--points] [--estimator haf|3pt|dlt] [--no-epipolar] [--compat-fit dlt[:trials[:limit_scale]]] [--data-term reference|rising] [--smoothness uniform|cauchy:RHO[:QMAX]] [--merge meanshift|energy] [--label-cost P] [--residual forward|symmetric] [--tail-score count|msac] [--tail-refit N] [--tail-polish N] [--polish N] [--reweight n[:scale]] [--estimator-reweight n[:scale]] [--reweight-auto n[:kappa]] [--estimator-reweight-auto n[:kappa]] [--sampler uniform|local[:k[:u]]] [--proposals dlt|haf[:members[:stride]]|3pt] [--ranks n]\n";
        return 2;
    }
    double thrF = 2.6, thrH = 2.2, locality = 0.005, lambda = 0.5;     // M/main.cpp:55-59
    int min_inliers = 20, hypotheses = 10000, max_models = 32, iterations = 0;
    unsigned long long seed = 1234;
    int ranks = 0;
    double load_filter = 2.0;                                          // M/main.cpp:400
    int f_metric = MultiH::FUND_EPIPOLAR_MAX;
    MultiH::FundEstimator f_estimator;
    std::string epi, neighbourhood = "knn", stages_path;
    bool points_only = false, no_epipolar = false;
    int estimator = MultiH::ESTIMATOR_HAF;
    int data_term = MultiH::DATA_TERM_REFERENCE;
    int residual = MultiH::RESIDUAL_FORWARD;
    int smoothness_rule = MultiH::SMOOTHNESS_UNIFORM, smoothness_q_max = 16;
    double smoothness_rho = 0.0;
    int merge_mode = MultiH::MERGE_MEAN_SHIFT;
    double label_cost = 0.0;
    int tail_score = MultiH::TAIL_SCORE_COUNT;
    int tail_refit = 0, tail_polish = 0, model_polish = 0;
    int compat_fit = MultiH::COMPAT_FIT_3PT, compat_trials = 501;
    double compat_limit_scale = 0.0;
    int model_reweight = 0, estimator_reweight = 0;
    double model_reweight_scale = 0.0, estimator_reweight_scale = 0.0;
    int model_reweight_auto = 0, estimator_reweight_auto = 0;
    double model_reweight_kappa = 0.0, estimator_reweight_kappa = 0.0;
    int select_score = MultiH::SELECTION_SCORE_COUNT;
    int sampler = MultiH::PROPOSAL_UNIFORM, sampler_k = 32, sampler_u = 4;
    int proposals = MultiH::PROPOSAL_SOURCE_DLT, haf_members = 16, haf_stride = 1;
    for (int i = 3; i < argc; ++i) {
        const std::string k = argv[i];
        if (k == "--points") { points_only = true; continue; }      // the two options without a value
        if (k == "--no-epipolar") { no_epipolar = true; continue; }
        if (i + 1 >= argc) break;
        const char* v = argv[++i];
        if (k == "--epipolar") epi = v;
        else if (k == "--estimator") {
            if (std::string(v) == "haf") estimator = MultiH::ESTIMATOR_HAF;
            else if (std::string(v) == "3pt") estimator = MultiH::ESTIMATOR_3PT;
            else if (std::string(v) == "dlt") estimator = MultiH::ESTIMATOR_DLT;
            else { std::cerr << "--estimator: haf, 3pt or dlt\n"; return 2; }
        }
        else if (k == "--data-term") {
            if (std::string(v) == "reference") data_term = MultiH::DATA_TERM_REFERENCE;
            else if (std::string(v) == "rising") data_term = MultiH::DATA_TERM_RISING;
            else { std::cerr << "--data-term: reference or rising\n"; return 2; }
        }
        else if (k == "--smoothness") {
            const std::string sv(v);
            char tail = 0;
            if (sv == "uniform") smoothness_rule = MultiH::SMOOTHNESS_UNIFORM;
            else if (std::sscanf(v, "cauchy:%lf:%d%c", &smoothness_rho, &smoothness_q_max, &tail) == 2 ||
                     (smoothness_q_max = 16, std::sscanf(v, "cauchy:%lf%c", &smoothness_rho, &tail) == 1))
                smoothness_rule = MultiH::SMOOTHNESS_CAUCHY;
            else { std::cerr << "--smoothness: uniform or cauchy:RHO[:QMAX]\n"; return 2; }
        }
        else if (k == "--merge") {
            if (std::string(v) == "meanshift") merge_mode = MultiH::MERGE_MEAN_SHIFT;
            else if (std::string(v) == "energy") merge_mode = MultiH::MERGE_ENERGY;
            else { std::cerr << "--merge: meanshift or energy\n"; return 2; }
        }
        else if (k == "--label-cost") label_cost = std::atof(v);
        else if (k == "--residual") {
            if (std::string(v) == "forward") residual = MultiH::RESIDUAL_FORWARD;
            else if (std::string(v) == "symmetric") residual = MultiH::RESIDUAL_SYMMETRIC;
            else { std::cerr << "--residual: forward or symmetric\n"; return 2; }
        }
        else if (k == "--tail-score") {
            if (std::string(v) == "count") tail_score = MultiH::TAIL_SCORE_COUNT;
            else if (std::string(v) == "msac") tail_score = MultiH::TAIL_SCORE_MSAC;
            else { std::cerr << "--tail-score: count or msac\n"; return 2; }
        }
        else if (k == "--tail-refit") {
            const std::string tv = v;
            if (tv.empty() || tv.size() > 2 || tv.find_first_not_of("0123456789") != std::string::npos || atoi(v) > 16) {
                std::cerr << "--tail-refit: a whole number in [0, 16]\n";
                return 2;
            }
            tail_refit = atoi(v);
        }
        else if (k == "--tail-polish" || k == "--polish") {
            const std::string tv = v;
            if (tv.empty() || tv.size() > 2 || tv.find_first_not_of("0123456789") != std::string::npos || atoi(v) > 32) {
                std::cerr << k << ": a whole number in [0, 32]\n";
                return 2;
            }
            (k == "--polish" ? model_polish : tail_polish) = atoi(v);
        }
        else if (k == "--compat-fit") {
            // dlt | dlt:trials | dlt:trials:limit_scale — trials a whole number in [1, 4096], limit_scale a number > 0
            const std::string tv = v;
            const size_t c1 = tv.find(':'), c2 = c1 == std::string::npos ? c1 : tv.find(':', c1 + 1);
            bool ok = tv.substr(0, c1) == "dlt";
            if (ok && c1 != std::string::npos) {
                const std::string nv = tv.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
                ok = !nv.empty() && nv.size() <= 4 && nv.find_first_not_of("0123456789") == std::string::npos && atoi(nv.c_str()) >= 1 &&
                     atoi(nv.c_str()) <= 4096;
                if (ok) compat_trials = atoi(nv.c_str());
            }
            if (ok && c2 != std::string::npos) {
                char* end = nullptr;
                compat_limit_scale = strtod(tv.c_str() + c2 + 1, &end);
                ok = end != tv.c_str() + c2 + 1 && *end == '\0' && compat_limit_scale > 0.0 && compat_limit_scale <= 1e150;
            }
            if (!ok) {
                std::cerr << "--compat-fit: dlt[:trials[:limit_scale]], trials a whole number in [1, 4096], limit_scale a number > 0\n";
                return 2;
            }
            compat_fit = MultiH::COMPAT_FIT_DLT;
        }
        else if (k == "--reweight" || k == "--estimator-reweight") {
            // n | n:scale — a whole number of rounds in [0, 16], a scale in pixels > 0 (default: the homography threshold)
            const std::string tv = v;
            const size_t colon = tv.find(':');
            const std::string nv = tv.substr(0, colon);
            double scale = 0.0;
            bool ok = !nv.empty() && nv.size() <= 2 && nv.find_first_not_of("0123456789") == std::string::npos && atoi(nv.c_str()) <= 16;
            if (ok && colon != std::string::npos) {
                char* end = nullptr;
                scale = strtod(tv.c_str() + colon + 1, &end);
                ok = end != tv.c_str() + colon + 1 && *end == '\0' && scale > 0.0 && scale <= 1e150;
            }
            if (!ok) {
                std::cerr << k << ": n[:scale], n a whole number in [0, 16], scale a number of pixels > 0\n";
                return 2;
            }
            (k == "--reweight" ? model_reweight : estimator_reweight) = atoi(nv.c_str());
            (k == "--reweight" ? model_reweight_scale : estimator_reweight_scale) = scale;
        }
        else if (k == "--reweight-auto" || k == "--estimator-reweight-auto") {
            // n | n:kappa — a whole number of rounds in [0, 16], a factor kappa > 0 on the root of the label's median squared error
            // (default: kappa^2 = log2(100))
            const std::string tv = v;
            const size_t colon = tv.find(':');
            const std::string nv = tv.substr(0, colon);
            double kappa = 0.0;
            bool ok = !nv.empty() && nv.size() <= 2 && nv.find_first_not_of("0123456789") == std::string::npos && atoi(nv.c_str()) <= 16;
            if (ok && colon != std::string::npos) {
                char* end = nullptr;
                kappa = strtod(tv.c_str() + colon + 1, &end);
                ok = end != tv.c_str() + colon + 1 && *end == '\0' && kappa > 0.0 && kappa <= 1e150;
            }
            if (!ok) {
                std::cerr << k << ": n[:kappa], n a whole number in [0, 16], kappa a number > 0\n";
                return 2;
            }
            (k == "--reweight-auto" ? model_reweight_auto : estimator_reweight_auto) = atoi(nv.c_str());
            (k == "--reweight-auto" ? model_reweight_kappa : estimator_reweight_kappa) = kappa;
        }
        else if (k == "--select-score") {
            if (std::string(v) == "count") select_score = MultiH::SELECTION_SCORE_COUNT;
            else if (std::string(v) == "msac") select_score = MultiH::SELECTION_SCORE_MSAC;
            else { std::cerr << "--select-score: count or msac\n"; return 2; }
        }
        else if (k == "--sampler") {
            // uniform | local | local:k | local:k:u — whole numbers, nothing behind them
            const std::string sv = v;
            auto whole = [](const std::string& t, int lo, int hi, int& out) {
                if (t.empty() || t.size() > 3 || t.find_first_not_of("0123456789") != std::string::npos) return false;
                out = atoi(t.c_str());
                return out >= lo && out <= hi;
            };
            bool good = true;
            int kk = 32, uu = 4;
            if (sv == "uniform") sampler = MultiH::PROPOSAL_UNIFORM;
            else if (sv.compare(0, 5, "local") == 0 && (sv.size() == 5 || sv[5] == ':')) {
                if (sv.size() > 5) {
                    const std::string rest = sv.substr(6);
                    const size_t colon = rest.find(':');
                    good = whole(rest.substr(0, colon), 3, 32, kk) && (colon == std::string::npos || whole(rest.substr(colon + 1), 0, 16, uu));
                }
                if (good) { sampler = MultiH::PROPOSAL_LOCAL; sampler_k = kk; sampler_u = uu; }
            }
            else good = false;
            if (!good) { std::cerr << "--sampler " << sv << ": uniform, local, local:k or local:k:u with whole numbers 3 <= k <= 32, 0 <= u <= 16\n"; return 2; }
        }
        else if (k == "--proposals") {
            // dlt | haf | haf:members | haf:members:stride | 3pt — whole numbers, nothing behind them
            const std::string sv = v;
            auto whole = [](const std::string& t, int lo, int hi, int& out) {
                if (t.empty() || t.size() > 7 || t.find_first_not_of("0123456789") != std::string::npos) return false;
                out = atoi(t.c_str());
                return out >= lo && out <= hi;
            };
            bool good = true;
            int mm = 16, ss = 1;
            if (sv == "dlt") proposals = MultiH::PROPOSAL_SOURCE_DLT;
            else if (sv == "3pt") proposals = MultiH::PROPOSAL_SOURCE_3PT;
            else if (sv.compare(0, 3, "haf") == 0 && (sv.size() == 3 || sv[3] == ':')) {
                if (sv.size() > 3) {
                    const std::string rest = sv.substr(4);
                    const size_t colon = rest.find(':');
                    good = whole(rest.substr(0, colon), 0, 32, mm) && mm != 1 && mm != 2 &&
                           (colon == std::string::npos || whole(rest.substr(colon + 1), 1, 1000000, ss));
                }
                if (good) { proposals = MultiH::PROPOSAL_SOURCE_HAF; haf_members = mm; haf_stride = ss; }
            }
            else good = false;
            if (!good) {
                std::cerr << "--proposals " << sv << ": dlt, 3pt, haf, haf:members or haf:members:stride with whole numbers, members 0 or 3 .. 32, stride >= 1\n";
                return 2;
            }
        }
        else if (k == "--thrF") thrF = atof(v);
        else if (k == "--thrH") thrH = atof(v);
        else if (k == "--locality") locality = atof(v);
        else if (k == "--lambda") lambda = atof(v);
        else if (k == "--min-inliers") min_inliers = atoi(v);
        else if (k == "--hypotheses") hypotheses = atoi(v);
        else if (k == "--max-models") max_models = atoi(v);
        else if (k == "--seed") seed = strtoull(v, nullptr, 10);
        else if (k == "--iterations") iterations = atoi(v);
        else if (k == "--neighbourhood") neighbourhood = v;
        else if (k == "--ranks") ranks = atoi(v);
        else if (k == "--load-filter") load_filter = atof(v);
        else if (k == "--f-metric") {
            if (std::string(v) == "sampson") f_metric = MultiH::FUND_SAMPSON;
            else if (std::string(v) == "opencv") f_metric = MultiH::FUND_EPIPOLAR_MAX;
            else { std::cerr << "--f-metric: opencv or sampson\n"; return 2; }
        }
        else if (k == "--f-estimator") {
            if (std::string(v) == "ls8") f_estimator.mode = MultiH::FUND_ESTIMATOR_LS8;
            else if (std::string(v) == "minimal") f_estimator.mode = MultiH::FUND_ESTIMATOR_MINIMAL7;
            else { std::cerr << "--f-estimator: ls8 or minimal\n"; return 2; }
        }
        else if (k == "--stages") stages_path = v;
        else { std::cerr << "unknown option " << k << "\n"; return 2; }
    }
    if ((model_reweight > 0 && model_reweight_auto > 0) || (estimator_reweight > 0 && estimator_reweight_auto > 0)) {
        const char* base = model_reweight > 0 && model_reweight_auto > 0 ? "--reweight" : "--estimator-reweight";
        std::cerr << base << " and " << base << "-auto: one scale rule, not both\n";
        return 2;
    }

    // --ranks N: fork ranks 1..N-1 now — no HIP call has been made yet — then every rank joins the communicator.  RCCL's
    // 128-byte bootstrap id travels from rank 0 to each child through a pipe made before the fork: no file, so no
    // predictable path to plant a link at and no stale id of a crashed run to pick up (r03 advisor finding).
    int rank = 0;
    std::vector<pid_t> kids;
    std::vector<int> id_writers;                 // rank 0: write ends, one per child
    int id_reader = -1;                          // child: read end
    if (ranks > 1) {
        for (int r = 1; r < ranks; ++r) {
            int fds[2];
            if (pipe(fds) != 0) { perror("pipe"); return 1; }
            const pid_t pid = fork();
            if (pid < 0) { perror("fork"); return 1; }
            if (pid == 0) {
                rank = r;
                kids.clear();
                close(fds[1]);
                for (int w : id_writers) close(w);
                id_writers.clear();
                id_reader = fds[0];
                break;
            }
            close(fds[0]);
            id_writers.push_back(fds[1]);
            kids.push_back(pid);
        }
    }
    auto finish = [&](int rc) {
        for (int w : id_writers) close(w);       // (a child still waiting for the id sees end-of-file and gives up)
        id_writers.clear();
        for (pid_t pid : kids) {
            int st = 0;
            if (waitpid(pid, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) {
                std::cerr << "[Multi-H] a rank failed\n";
                if (rc == 0) rc = 1;
            }
        }
        return rc;
    };
    mhr_comm* comm = nullptr;
    int (*allgather)(void*, const void*, void*, unsigned long long, void*) = nullptr;
    void (*comm_destroy)(mhr_comm*) = nullptr;
    if (ranks >= 1) {
        void* lib = dlopen("libmultih_rccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) { std::cerr << "cannot load libmultih_rccl.so: " << dlerror() << "\n"; return finish(1); }
        auto init_id = (int (*)(mhr_comm**, int, int, const unsigned char*, int))dlsym(lib, "mhr_init");
        auto make_id = (int (*)(unsigned char*))dlsym(lib, "mhr_unique_id");
        auto last_error = (const char* (*)())dlsym(lib, "mhr_last_error");
        allgather = (int (*)(void*, const void*, void*, unsigned long long, void*))dlsym(lib, "mhr_allgather");
        comm_destroy = (void (*)(mhr_comm*))dlsym(lib, "mhr_destroy");
        if (!init_id || !make_id || !allgather || !comm_destroy || !last_error) { std::cerr << "libmultih_rccl.so lacks a symbol\n"; return finish(1); }
        unsigned char id[MHR_ID_BYTES];
        int rc = 0;
        if (rank == 0) {
            rc = make_id(id);
            for (int w : id_writers) {
                if (rc == 0 && write(w, id, MHR_ID_BYTES) != (ssize_t)MHR_ID_BYTES) { std::cerr << "[Multi-H] cannot hand the RCCL id to a rank\n"; rc = 1; }
                close(w);
            }
            id_writers.clear();
        } else {
            // the id arrives within two minutes or not at all (end-of-file: rank 0 gave up)
            size_t got = 0;
            struct pollfd pf = { id_reader, POLLIN, 0 };
            while (got < MHR_ID_BYTES) {
                if (poll(&pf, 1, 120000) <= 0) break;
                const ssize_t k = read(id_reader, id + got, MHR_ID_BYTES - got);
                if (k <= 0) break;
                got += (size_t)k;
            }
            close(id_reader);
            if (got != MHR_ID_BYTES) { std::cerr << "[Multi-H] rank " << rank << ": no RCCL id from rank 0\n"; return finish(1); }
        }
        if (rc == 0) {
            signal(SIGALRM, [](int) {
                static const char msg[] = "[Multi-H] the RCCL communicator was not complete after 300 s (a rank died?): giving up\n";
                (void)!write(2, msg, sizeof(msg) - 1);
                _exit(1);
            });
            alarm(300);                          // ncclCommInitRank waits for every rank: a peer that died must not hang the others
            rc = init_id(&comm, rank, std::max(ranks, 1), id, rank);
            alarm(0);
        }
        if (rc != 0) { std::cerr << "[Multi-H] rank " << rank << ": RCCL communicator: " << last_error() << "\n"; return finish(1); }
        printf("[Multi-H] rank %d of %d joined the RCCL communicator (device %d)\n", rank, ranks, rank);
    }

    std::vector<cv::Point2d> srcPointsOrig, dstPointsOrig;
    std::vector<cv::Mat> origAffines;
    int rows_loaded = 0;
    if (!LoadPointsFromFile(srcPointsOrig, dstPointsOrig, origAffines, argv[1], epi.empty() && !no_epipolar ? load_filter : 0.0, seed, f_metric,
                            comm ? rank : 0, &rows_loaded, points_only, f_estimator)) {
        std::cerr << "cannot read " << argv[1] << " (or the load filter failed)\n";
        return finish(1);
    }
    printf("Found %d matches.\n", (int)srcPointsOrig.size());
    const int rows_after_load_filter = (int)srcPointsOrig.size();

    MultiH* multiH = new MultiH(thrF, thrH, locality, lambda, min_inliers);
    if (!epi.empty()) {
        std::ifstream f(epi);
        double F[9], e2[2];
        bool ok = true;
        for (double& x : F) ok = ok && static_cast<bool>(f >> x);
        for (double& x : e2) ok = ok && static_cast<bool>(f >> x);
        if (!ok) { std::cerr << "cannot read epipolar geometry from " << epi << "\n"; return finish(1); }
        multiH->SetEpipolarGeometry(F, e2);
    }
    multiH->SetFundamentalMetric(f_metric);
    multiH->SetFundamentalEstimator(f_estimator.mode, f_estimator.max_samples, f_estimator.confidence);
    multiH->SetProposal(seed, hypotheses, max_models);
    multiH->SetFixedIterations(iterations);
    if (comm) {
        multiH->SetDevice(rank);
        multiH->SetShardingStream(rank, ranks, allgather, comm);
    }
    if (neighbourhood == "radius") multiH->SetNeighbourRadius(1.0 / locality);        // the complete list of M/MultiH.cpp:252-253 (see MultiH.h)
    else if (neighbourhood == "approx") multiH->SetNeighbourApprox(4, 32, 0x464c414e4eull + seed);   // ... as FLANN's default search answers it
    multiH->SetEstimator(estimator);
    multiH->SetEpipolarFree(no_epipolar);
    multiH->SetCompatibilityFit(compat_fit, compat_trials, compat_limit_scale);
    multiH->SetDataTerm(data_term);
    multiH->SetSmoothnessWeights(smoothness_rule, smoothness_rho, smoothness_q_max);
    multiH->SetMergeMode(merge_mode);
    multiH->SetLabelCost(label_cost);
    multiH->SetResidual(residual);
    multiH->SetTailScore(tail_score);
    multiH->SetTailRefit(tail_refit);
    multiH->SetTailPolish(tail_polish);
    multiH->SetModelPolish(model_polish);
    multiH->SetModelReweight(model_reweight, model_reweight_scale);
    multiH->SetEstimatorReweight(estimator_reweight, estimator_reweight_scale);
    multiH->SetModelReweightAuto(model_reweight_auto, model_reweight_kappa);
    multiH->SetEstimatorReweightAuto(estimator_reweight_auto, estimator_reweight_kappa);
    multiH->SetSelectionScore(select_score);
    multiH->SetProposalSampler(sampler, sampler_k, sampler_u);
    multiH->SetProposalSource(proposals, haf_members, haf_stride);
    const bool processed = points_only ? multiH->Process(srcPointsOrig, dstPointsOrig)
                                       : multiH->Process(srcPointsOrig, dstPointsOrig, origAffines);
    if (!processed) { delete multiH; return finish(1); }
    const std::string out_path = rank == 0 ? std::string(argv[2]) : std::string(argv[2]) + ".rank" + std::to_string(rank);
    {
        // the stage table: where the rows of the input file go before the loop sees them
        const MultiH::FrontStages st = multiH->GetFrontStages();
        printf("[Multi-H] stages: %d loaded, %d after the load filter (%.2f px), %d in Process()'s RANSAC mask (%.2f px), "
               "%d after OptimalTriangulation, %d after distanceError <= 1\n",
               rows_loaded, rows_after_load_filter, epi.empty() && !no_epipolar ? load_filter : 0.0, st.in_ransac_mask, thrF, st.triangulated,
               st.affine_consistent);
        if (!stages_path.empty() && rank == 0) {
            std::ofstream sf(stages_path);
            sf << "{\"loaded\": " << rows_loaded << ", \"after_load_filter\": " << rows_after_load_filter
               << ", \"load_filter_px\": " << (epi.empty() && !no_epipolar ? load_filter : 0.0) << ", \"in_ransac_mask\": " << st.in_ransac_mask
               << ", \"ransac_px\": " << thrF << ", \"after_optimal_triangulation\": " << st.triangulated
               << ", \"after_distance_error\": " << st.affine_consistent << ", \"f_metric\": \""
               << (f_metric == MultiH::FUND_SAMPSON ? "sampson" : "opencv") << "\", \"f_estimator\": \""
               << (f_estimator.mode == MultiH::FUND_ESTIMATOR_MINIMAL7 ? "minimal" : "ls8") << "\"}\n";
        }
    }

    std::vector<int> labeling;
    multiH->GetLabels(labeling);
    int iterationNum = multiH->GetIterationNumber();
    if (multiH->GetClusterNumber() < 1) {
        multiH->Release();
        std::cerr << "No homographies were found!\n";
        delete multiH;
        return finish(1);
    }
    printf("[Multi-H] %d clusters, %d iterations, energy %.0f\n", multiH->GetClusterNumber(), iterationNum,
           multiH->GetEnergy());
    if (merge_mode == MultiH::MERGE_ENERGY) {
        long long pairs = 0, accepted = 0, filtered = 0, sum_delta = 0;
        for (const MultiH::MergeLogRecord& r : multiH->GetMergeLog()) {
            pairs += r.pairs; accepted += r.merges_accepted; filtered += r.models_filtered; sum_delta += r.sum_delta;
        }
        printf("[Multi-H] Energy merges: %d steps, %lld pairs evaluated, %lld joined, %lld models filtered, sum of deltas %lld\n",
               (int)multiH->GetMergeLog().size(), pairs, accepted, filtered, sum_delta);
    }
    if (label_cost > 0.0) {
        long long candidates = 0, dropped = 0, members = 0, to_outlier = 0, beta = 0;
        for (const MultiH::DropLogRecord& r : multiH->GetDropLog()) {
            candidates += r.candidates; beta = r.beta;
            if (r.dropped >= 0) { ++dropped; members += r.members; to_outlier += r.to_outlier; }
        }
        printf("[Multi-H] Label cost: beta %lld, %d steps, %lld candidates evaluated, %lld labels dropped (%lld members, %lld to the outlier label)\n",
               beta, (int)multiH->GetDropLog().size(), candidates, dropped, members, to_outlier);
    }

    std::vector<cv::Point2d> src_points, dst_points;
    std::vector<cv::Mat> affinities;
    std::vector<int> labels;
    multiH->GetLabels(labels);
    bool saved;
    if (labels.size() == srcPointsOrig.size()) {                        // M/main.cpp:287-297
        saved = SavePointsToFile(srcPointsOrig, dstPointsOrig, origAffines, labels, out_path.c_str());
    } else {
        multiH->GetSourcePoints(src_points);
        multiH->GetDestinationPoints(dst_points);
        multiH->GetAffinities(affinities);
        saved = SavePointsToFile(src_points, dst_points, affinities, labels, out_path.c_str());
    }
    multiH->Release();
    delete multiH;
    if (comm) comm_destroy(comm);
    return finish(saved ? 0 : 1);
}
