// reweight_h.hip — mh_reweight_homographies: per label, iteratively reweighted normalised N-point DLT refits, gfx950.  Every
// other per-label estimate of the engine is a plain least-squares fit over whatever the labeling handed it; this one weighs
// each member by its MSAC gain 1 - d2 / c2 under the model that stands (mh_score_msac's expression in front of its 256.0 *),
// so that members the model explains badly pull less and members beyond c2 not at all.  The rule is stated operation by
// operation in include/multih_hip.h and restated in tests/reweight_h_numpy.py; the fit is wg_fit.hpp's fit(S) with every
// member's terms weighted (hartley_centroids_w, hartley_distances_w, hartley_scales_w, dlt_accumulate_w), dlt_solve as it stands.
//
// One 256-thread workgroup per label (blockIdx.x = k); all rounds of a call run inside ONE launch:
//     cur = H_in[k]
//     pass 1 (cur)   members counted; support c, W = sum of w, the four sums of w * coordinate     <- W and c of cur: the
//     pass 2 (cur)   the two sums of w * distance to the centroids -> scales                         outputs when the loop ends here
//     pass 3 (cur)   the 24 weighted sums
//     thread 0       dlt_solve -> the candidate; cur = candidate unless it is not finite or cur's bits
// so a call of r rounds is 3 r + 1 passes: the last pass 1 gives W and the support of the result.  The weight is recomputed from
// cur in each pass: no per-member storage.
// Members come from for_label_members, whose lane assignment is the engine's order of every FP64 sum.  Members with w == 0
// add no term.  The loop is bounded by `rounds` (at most REWEIGHT_H_MAX_ROUNDS), Jacobi by its 30 sweeps; nothing waits for
// anything but the workgroup's own barriers, and every exit is taken by the whole workgroup.
//
// The 9 x 9 Jacobi stands in the LDS reduction buffer, idle once a tree has run (as in k_dlt_reestimate): no private array with
// a run-time index, no scratch.

#include <cmath>
#include "mh_kernels.hpp"
#include "wg_fit.hpp"

namespace mh {

namespace {

constexpr int RW_HEAD = 7;                       // pass 1's columns: four weighted coordinate sums, W, members, support

} // namespace

// H_in, H_out: m x 9 (may be the same array: a workgroup reads its row before it writes it); gain: m x 2 (W of H_in, W of
// H_out), info: m x 4 (members, support of H_out, rounds done, status), counts: m (members) — the last three nullable.
__global__ void __launch_bounds__(256)
k_reweight_h(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
             const double* __restrict__ y2, int N, const int* __restrict__ labels, const double* H_in, double c2, int rounds,
             double* H_out, double* __restrict__ gain, int* __restrict__ info, int* __restrict__ counts)
{
    const int l = blockIdx.x, t = threadIdx.x;
    __shared__ double sv[256][DLT_SUMS];         // 48 KB: the partial sums; then dlt_solve's work space
    __shared__ double s_cur[9];                  // the model that stands
    __shared__ double s_par[6];                  // cx1 cy1 cx2 cy2 s1 s2
    __shared__ double s_G[DLT_SUMS];
    __shared__ int s_stop;
    auto members = [&](auto&& f) { for_label_members<16, long long>(labels, N, l, t, f); };

    if (t < 9) s_cur[t] = H_in[9 * (size_t)l + t];
    __syncthreads();
    bool finite_in = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) finite_in = finite_in && finite_dev(s_cur[j]);

    int n_members = 0, support = 0, done = 0, status = 0;
    double W_in = 0.0, W_cur = 0.0;
    for (int r = 0; ; ++r) {                     // at most rounds + 1 <= 17 trips
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = s_cur[i];
        auto weight = [&](double x, double y, double u, double v) {
            return reweight_w(fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x, y, u, v), c2);
        };

        // pass 1
        {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, aw = 0.0;
            int cnt = 0, in = 0;
            members([&](int n) {
                const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
                const double w = weight(x, y, u, v);
                ++cnt;
                if (w > 0.0) {
                    a0 = a0 + w * x; a1 = a1 + w * y; a2 = a2 + w * u; a3 = a3 + w * v;
                    aw = aw + w;
                    ++in;
                }
            });
            sv[t][0] = a0; sv[t][1] = a1; sv[t][2] = a2; sv[t][3] = a3; sv[t][4] = aw;
            sv[t][5] = (double)cnt; sv[t][6] = (double)in;                   // (a count is exact as a double)
            wg_tree<RW_HEAD>(sv, t);
        }
        const double W = sv[0][4];
        const int c = (int)sv[0][6];
        if (r == 0) {
            n_members = (int)sv[0][5];
            status = n_members < 4 ? 1 : (!finite_in ? 2 : 0);
            if (status != 0) break;              // (the same for every thread, like every break below)
            W_in = W;
        }
        W_cur = W; support = c;
        if (r == rounds) break;

        // wfit(cur)
        if (c < 4) break;
        Hartley hn;
        hartley_centroids_w(sv[0], W, s_par, t, hn);
        // pass 2
        {
            double d1 = 0.0, d2 = 0.0;
            members([&](int n) {
                const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
                const double w = weight(x, y, u, v);
                if (w > 0.0) hartley_distances_w(hn, w, x, y, u, v, d1, d2);
            });
            sv[t][0] = d1; sv[t][1] = d2;
            wg_tree<2>(sv, t);
        }
        hartley_scales_w(sv[0], W, s_par, t, hn);
        if (!finite_dev(hn.s1) || !finite_dev(hn.s2)) break;
        // pass 3
        {
            double acc[DLT_SUMS];
#pragma unroll
            for (int k = 0; k < DLT_SUMS; ++k) acc[k] = 0.0;
            members([&](int n) {
                const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
                const double w = weight(x, y, u, v);
                if (w > 0.0) dlt_accumulate_w(hn, w, x, y, u, v, acc);
            });
#pragma unroll
            for (int k = 0; k < DLT_SUMS; ++k) sv[t][k] = acc[k];
            wg_tree<DLT_SUMS>(sv, t);
        }
        if (t < DLT_SUMS) s_G[t] = sv[0][t];
        __syncthreads();                         // the reduction buffer is idle from here: the solve's work space
        if (t == 0) {
            double o[9];
            dlt_solve(s_G, hn, &sv[0][0], o);
            bool finite = true, same = true;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                finite = finite && finite_dev(o[j]);
                same = same && (__double_as_longlong(o[j]) == __double_as_longlong(s_cur[j]));
            }
            const bool stop = !finite || same;
            if (!stop) {
#pragma unroll
                for (int j = 0; j < 9; ++j) s_cur[j] = o[j];
            }
            s_stop = stop ? 1 : 0;
        }
        __syncthreads();
        if (s_stop) break;                       // (W_cur and support are those of the model that stands)
        ++done;
    }

    if (t < 9) H_out[9 * (size_t)l + t] = s_cur[t];                          // (H_in's bits when nothing was done)
    if (t == 0) {
        if (counts) counts[l] = n_members;
        if (gain) {
            gain[2 * (size_t)l] = status == 0 ? W_in : 0.0;
            gain[2 * (size_t)l + 1] = status == 0 ? W_cur : 0.0;
        }
        if (info) {
            int* o = info + 4 * (size_t)l;
            o[0] = n_members; o[1] = status == 0 ? support : 0; o[2] = done; o[3] = status;
        }
    }
}

hipError_t launch_reweight_h(const Points& p, const int* labels, const double* H_in, int m, double c2, int rounds, double* H_out,
                             double* gain, int* info, int* counts, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    if (p.n <= 0 || rounds < 0 || rounds > REWEIGHT_H_MAX_ROUNDS || !labels || !(c2 > 0.0) || !std::isfinite(c2))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_reweight_h, dim3(m), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, labels, H_in, c2, rounds, H_out, gain,
                       info, counts);
    return hipGetLastError();
}

} // namespace mh
