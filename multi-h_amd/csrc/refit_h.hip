// refit_h.hip — mh_refit_homography: one homography re-estimated from all its inliers, the step cv::findHomography(CV_RANSAC)
// runs behind its winning minimal sample (M/MultiH.cpp:719-741 calls it; OpenCV's own code is not in the reference tree, so the
// arithmetic is the engine's definition, stated operation by operation in include/multih_hip.h and restated in
// tests/refit_h_numpy.py).  The fit is wg_fit.hpp's fit(S) with a model's inliers as S; the order of the sums is stated there.
//
// All rounds of a call run inside ONE launch:
//     h = H_in
//     pass 1 (h)   inlier flags, count, centroid sums            <- for a candidate this IS its count: accept or reject here
//     pass 2       mean distances to the centroids -> scales
//     pass 3       the 24 sums
//     thread 0     dlt_solve -> the candidate; h = candidate
// so a call of r rounds is 3 r + 1 passes (+ 1 when the last candidate was rejected: the flags are written again for the model
// that stays).  The loop is bounded by `iterations` (at most REFIT_H_MAX_ITERATIONS), Jacobi by its 30 sweeps; nothing waits
// for anything but the workgroup's own barriers.

#include "mh_kernels.hpp"
#include "wg_fit.hpp"

namespace mh {

// out_i[0] = inliers of H_out, out_i[1] = fits accepted.  mask_out: n bytes.  iterations in [0, REFIT_H_MAX_ITERATIONS].
__global__ void __launch_bounds__(256)
k_refit_h(const double* __restrict__ x1, const double* __restrict__ y1,
          const double* __restrict__ x2, const double* __restrict__ y2, int N,
          const double* __restrict__ H_in, double thr2, int iterations, double* __restrict__ H_out,
          unsigned char* __restrict__ mask_out, int* __restrict__ out_i)
{
    const int t = threadIdx.x;
    __shared__ double sv[256][DLT_SUMS];         // 48 KB: the partial sums; then dlt_solve's work space
    __shared__ int sc[256];
    __shared__ double s_h[9];                    // the model the next pass 1 looks at: H_in, then each candidate
    __shared__ double s_cur[9];                  // the model that stands
    __shared__ double s_par[6];                  // cx1 cy1 cx2 cy2 s1 s2
    __shared__ double s_G[DLT_SUMS];
    __shared__ int s_stop;

    if (t < 9) { const double v = H_in[t]; s_h[t] = v; s_cur[t] = v; }
    if (t == 0) s_stop = 0;
    __syncthreads();

    int n_cur = 0, accepted = 0;
    bool flags_are_cur = true;                   // mask_out holds the flags of s_cur
    for (int r = 0; ; ++r) {                     // at most iterations + 1 <= 17 trips
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = s_h[i];

        // pass 1
        {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int cnt = 0;
            for (int n = t; n < N; n += 256) {
                const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
                const bool in = fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x, y, u, v) < thr2;
                mask_out[n] = in ? 1 : 0;
                if (in) { a0 = a0 + x; a1 = a1 + y; a2 = a2 + u; a3 = a3 + v; ++cnt; }
            }
            sv[t][0] = a0; sv[t][1] = a1; sv[t][2] = a2; sv[t][3] = a3;
            sc[t] = cnt;
            wg_tree<4>(sv, sc, t);
        }
        const int c = sc[0];
        if (r == 0) {
            n_cur = c;
        } else if (c < n_cur) {                  // the refit explains fewer points: it is dropped (key 30's rule)
            flags_are_cur = false;
            break;
        } else {
            n_cur = c; ++accepted;
            if (t < 9) s_cur[t] = h[t];          // (last read by thread 0 in the solve, barriers ago)
        }
        if (r == iterations) break;

        // fit(S(h)): h is the model that stands
        if (c < 4) break;
        Hartley hn;
        hartley_centroids(sv[0], c, s_par, t, hn);
        // pass 2
        {
            double d1 = 0.0, d2 = 0.0;
            for (int n = t; n < N; n += 256)
                if (mask_out[n]) hartley_distances(hn, x1[n], y1[n], x2[n], y2[n], d1, d2);      // (this thread's own flags of pass 1)
            sv[t][0] = d1; sv[t][1] = d2;
            wg_tree<2>(sv, t);
        }
        hartley_scales(sv[0], c, s_par, t, hn);
        if (!finite_dev(hn.s1) || !finite_dev(hn.s2)) break;            // (the same for every thread)
        // pass 3
        {
            double acc[DLT_SUMS];
#pragma unroll
            for (int k = 0; k < DLT_SUMS; ++k) acc[k] = 0.0;
            for (int n = t; n < N; n += 256)
                if (mask_out[n]) dlt_accumulate(hn, x1[n], y1[n], x2[n], y2[n], acc);
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
                s_h[j] = o[j];
            }
            s_stop = (!finite || same) ? 1 : 0;
        }
        __syncthreads();
        if (s_stop) break;                       // (pass 1 of h wrote the flags of the model that stands: they are current)
    }

    if (!flags_are_cur) {                        // the last pass 1 looked at a candidate that was dropped
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = s_cur[i];
        for (int n = t; n < N; n += 256)
            mask_out[n] = fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x1[n], y1[n], x2[n], y2[n]) < thr2 ? 1 : 0;
    }
    if (t < 9) H_out[t] = s_cur[t];
    if (t == 0) { out_i[0] = n_cur; out_i[1] = accepted; }
}

hipError_t launch_refit_h(const Points& p, const double* H_in, double thr2, int iterations, double* H_out,
                          unsigned char* mask_out, int* out_i, hipStream_t s)
{
    if (p.n <= 0 || iterations < 0 || iterations > REFIT_H_MAX_ITERATIONS || !mask_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refit_h, dim3(1), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H_in, thr2, iterations, H_out,
                       mask_out, out_i);
    return hipGetLastError();
}

} // namespace mh
