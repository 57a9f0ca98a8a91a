// reestimate_dlt.hip — per-label normalised N-point DLT re-estimation from points alone, gfx950 (mh_set_estimator(MH_ESTIMATOR_DLT)).
//
// H[k] = fit(S_k), S_k = { i : labels[i] == k }: wg_fit.hpp's fit(S), the one k_refit_h runs on a model's inliers, with no
// rounds and no acceptance test.  Neither F, the epipole nor the affinities are read: this is the re-estimator of the route
// without epipolar geometry, the counterpart of k_haf_reestimate and k_3pt_reestimate.
//
// One workgroup of 256 per label, three passes over its members (count and centroid sums; mean distances; the 24 sums), then
// thread 0 solves.  Members are found by for_label_members: that lane assignment IS the engine's order of every FP64 sum, so
// a compacted member list is not an option here.  A label whose fit fails (fewer than 4 members, a scale that is not finite,
// an entry of the result that is not finite) keeps its nine doubles.  counts[k] = |S_k|.
// Loops are bounded by N and by Jacobi's 30 sweeps; the workgroup waits for nothing but its own barriers, and every exit is
// uniform over the workgroup.

#include "mh_kernels.hpp"
#include "wg_fit.hpp"

namespace mh {

__global__ void __launch_bounds__(256)
k_dlt_reestimate(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                 const double* __restrict__ y2, const int* __restrict__ labels, int N, double* __restrict__ H,
                 int* __restrict__ counts)
{
    const int l = blockIdx.x, t = threadIdx.x;
    __shared__ double sv[256][DLT_SUMS];         // 48 KB: the partial sums; then dlt_solve's work space
    __shared__ int sc[256];
    __shared__ double s_par[6];                  // cx1 cy1 cx2 cy2 s1 s2
    __shared__ double s_G[DLT_SUMS];
    auto members = [&](auto&& f) { for_label_members<16, long long>(labels, N, l, t, f); };

    // pass 1
    {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int cnt = 0;
        members([&](int n) {
            a0 = a0 + x1[n]; a1 = a1 + y1[n]; a2 = a2 + x2[n]; a3 = a3 + y2[n];
            ++cnt;
        });
        sv[t][0] = a0; sv[t][1] = a1; sv[t][2] = a2; sv[t][3] = a3;
        sc[t] = cnt;
        // wg_tree's counted form, written out: as a call it moves a load of the label fetch above (the thread index is
        // widened once for the tree and the 64-bit match loop together), and the loops' instructions are to stay what they were
        __syncthreads();
        for (int s = 128; s >= 1; s >>= 1) {
            if (t < s) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sv[t][k] = sv[t][k] + sv[t + s][k];
                sc[t] += sc[t + s];
            }
            __syncthreads();
        }
    }
    const int c = sc[0];
    if (t == 0 && counts) counts[l] = c;
    if (c < 4) return;                           // keeps its H (c is the same in every thread)
    Hartley hn;
    hartley_centroids(sv[0], c, s_par, t, hn);
    // pass 2
    {
        double d1 = 0.0, d2 = 0.0;
        members([&](int n) { hartley_distances(hn, x1[n], y1[n], x2[n], y2[n], d1, d2); });
        sv[t][0] = d1; sv[t][1] = d2;
        wg_tree<2>(sv, t);
    }
    hartley_scales(sv[0], c, s_par, t, hn);
    if (!finite_dev(hn.s1) || !finite_dev(hn.s2)) return;                // keeps its H (the same for every thread)
    // pass 3
    {
        double acc[DLT_SUMS];
#pragma unroll
        for (int k = 0; k < DLT_SUMS; ++k) acc[k] = 0.0;
        members([&](int n) { dlt_accumulate(hn, x1[n], y1[n], x2[n], y2[n], acc); });
#pragma unroll
        for (int k = 0; k < DLT_SUMS; ++k) sv[t][k] = acc[k];
        wg_tree<DLT_SUMS>(sv, t);
    }
    if (t < DLT_SUMS) s_G[t] = sv[0][t];
    __syncthreads();                             // the reduction buffer is idle from here: the solve's work space
    if (t != 0) return;                          // (no barrier follows)

    double Hh[9];
    dlt_solve(s_G, hn, &sv[0][0], Hh);
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) finite = finite && finite_dev(Hh[j]);
    if (!finite) return;                         // keeps its H
    double* out = H + 9 * (size_t)l;
#pragma unroll
    for (int j = 0; j < 9; ++j) out[j] = Hh[j];
}

hipError_t launch_reestimate_dlt(const Points& p, const int* labels, int Nh, double* H, int* counts, hipStream_t s)
{
    if (Nh <= 0) return hipSuccess;
    if (p.n < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dlt_reestimate, dim3(Nh), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, labels, p.n, H, counts);
    return hipGetLastError();
}

} // namespace mh
