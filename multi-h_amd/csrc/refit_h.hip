// refit_h.hip — mh_refit_homography: one homography re-estimated from all its inliers, the step cv::findHomography(CV_RANSAC)
// runs behind its winning minimal sample (M/MultiH.cpp:719-741 calls it; OpenCV's own code is not in the reference tree, so the
// arithmetic is the engine's definition, stated operation by operation in include/multih_hip.h and restated in
// tests/refit_h_numpy.py).  Normalised N-point DLT through the 9 x 9 normal matrix of the two DLT rows per correspondence,
// k_fund_refit's scheme for a homography: one workgroup, strided passes over the points, every FP64 sum in the engine's order
// (thread t of 256 adds its members t, t + 256, ... from 0.0, then the binary tree 128 .. 1), -ffp-contract=off.
//
// All rounds of a call run inside ONE launch:
//     h = H_in
//     pass 1 (h)   inlier flags, count, centroid sums            <- for a candidate this IS its count: accept or reject here
//     pass 2       mean distances to the centroids -> scales
//     pass 3       the 24 sums G0..G3 over the six products p_a p_b
//     thread 0     9 x 9 cyclic Jacobi (jacobi_sym_dev), de-normalisation by k_dlt4's steps -> the candidate; h = candidate
// so a call of r rounds is 3 r + 1 passes (+ 1 when the last candidate was rejected: the flags are written again for the model
// that stays).  The loop is bounded by `iterations` (at most REFIT_H_MAX_ITERATIONS), Jacobi by its 30 sweeps; nothing waits
// for anything but the workgroup's own barriers.
//
// The 9 x 9 solve: jacobi_sym_dev indexes A and V by run-time p, q — as private arrays (k_fund_refit's form) they live in
// scratch memory.  Here A, V and D stand in the LDS reduction buffer, idle once the tree has run (the 24 sums are copied out
// first): no scratch, no private arrays with run-time indices.

#include "mh_kernels.hpp"
#include "mh_device.hpp"

namespace mh {

namespace {

constexpr int RH_SUMS = 24;

// v[t][0 .. K) += v[t + s][0 .. K), s = 128 .. 1; every thread of the workgroup calls it
template <int K>
__device__ __forceinline__ void refit_h_tree(double (*sv)[RH_SUMS], int t)
{
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sv[t][k] = sv[t][k] + sv[t + s][k];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool refit_h_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

} // namespace

// out_i[0] = inliers of H_out, out_i[1] = fits accepted.  mask_out: n bytes.  iterations in [0, REFIT_H_MAX_ITERATIONS].
__global__ void __launch_bounds__(256)
k_refit_h(const double* __restrict__ x1, const double* __restrict__ y1,
          const double* __restrict__ x2, const double* __restrict__ y2, int N,
          const double* __restrict__ H_in, double thr2, int iterations, double* __restrict__ H_out,
          unsigned char* __restrict__ mask_out, int* __restrict__ out_i)
{
    const int t = threadIdx.x;
    __shared__ double sv[256][RH_SUMS];          // 48 KB: the partial sums; then A (81), V (81), D (9) of the solve
    __shared__ int sc[256];
    __shared__ double s_h[9];                    // the model the next pass 1 looks at: H_in, then each candidate
    __shared__ double s_cur[9];                  // the model that stands
    __shared__ double s_par[6];                  // cx1 cy1 cx2 cy2 s1 s2
    __shared__ double s_G[RH_SUMS];
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
        if (t == 0) {
            const double inv = 1.0 / (double)c;
            s_par[0] = sv[0][0] * inv; s_par[1] = sv[0][1] * inv; s_par[2] = sv[0][2] * inv; s_par[3] = sv[0][3] * inv;
        }
        __syncthreads();
        const double cx1 = s_par[0], cy1 = s_par[1], cx2 = s_par[2], cy2 = s_par[3];
        // pass 2
        {
            double d1 = 0.0, d2 = 0.0;
            for (int n = t; n < N; n += 256) {
                if (mask_out[n]) {               // (this thread's own flags of pass 1)
                    const double ax = x1[n] - cx1, ay = y1[n] - cy1, bx = x2[n] - cx2, by = y2[n] - cy2;
                    d1 = d1 + sqrt(ax * ax + ay * ay);
                    d2 = d2 + sqrt(bx * bx + by * by);
                }
            }
            sv[t][0] = d1; sv[t][1] = d2;
            refit_h_tree<2>(sv, t);
            if (t == 0) {
                s_par[4] = sqrt(2.0) / (sv[0][0] / (double)c);
                s_par[5] = sqrt(2.0) / (sv[0][1] / (double)c);
            }
            __syncthreads();
        }
        const double s1 = s_par[4], s2 = s_par[5];
        if (!refit_h_finite(s1) || !refit_h_finite(s2)) break;          // (the same for every thread)
        // pass 3
        {
            double acc[RH_SUMS];
#pragma unroll
            for (int k = 0; k < RH_SUMS; ++k) acc[k] = 0.0;
            for (int n = t; n < N; n += 256) {
                if (mask_out[n]) {
                    const double x = (x1[n] - cx1) * s1, y = (y1[n] - cy1) * s1, u = (x2[n] - cx2) * s2, v = (y2[n] - cy2) * s2;
                    const double p[3] = { x, y, 1.0 };
                    const double w = u * u + v * v;
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int b = a; b < 3; ++b) {
                            const double tt = p[a] * p[b];
                            acc[k] = acc[k] + tt;
                            acc[6 + k] = acc[6 + k] + u * tt;
                            acc[12 + k] = acc[12 + k] + v * tt;
                            acc[18 + k] = acc[18 + k] + w * tt;
                            ++k;
                        }
                }
            }
#pragma unroll
            for (int k = 0; k < RH_SUMS; ++k) sv[t][k] = acc[k];
            refit_h_tree<RH_SUMS>(sv, t);
        }
        if (t < RH_SUMS) s_G[t] = sv[0][t];
        __syncthreads();                         // the reduction buffer is idle from here: A, V, D of the solve stand in it
        if (t == 0) {
            double* A = &sv[0][0];
            double* V = A + 81;
            double* D = V + 81;
            for (int i = 0; i < 81; ++i) A[i] = 0.0;
            {
                int k = 0;
                for (int a = 0; a < 3; ++a)
                    for (int b = a; b < 3; ++b) {
                        const double g0 = s_G[k], g1 = -s_G[6 + k], g2 = -s_G[12 + k], g3 = s_G[18 + k];
                        A[a * 9 + b] = g0; A[b * 9 + a] = g0;
                        A[(3 + a) * 9 + 3 + b] = g0; A[(3 + b) * 9 + 3 + a] = g0;
                        A[a * 9 + 6 + b] = g1; A[(6 + b) * 9 + a] = g1; A[b * 9 + 6 + a] = g1; A[(6 + a) * 9 + b] = g1;
                        A[(3 + a) * 9 + 6 + b] = g2; A[(6 + b) * 9 + 3 + a] = g2; A[(3 + b) * 9 + 6 + a] = g2; A[(6 + a) * 9 + 3 + b] = g2;
                        A[(6 + a) * 9 + 6 + b] = g3; A[(6 + b) * 9 + 6 + a] = g3;
                        ++k;
                    }
            }
            jacobi_sym_dev(9, A, V, D);
            int jm = 0;
            for (int j = 1; j < 9; ++j) if (D[j] < D[jm]) jm = j;
            double g[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) g[j] = V[j * 9 + jm];
            // de-normalise: k_dlt4's steps
            double A1[9];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double a = g[3 * q], b = g[3 * q + 1], cc = g[3 * q + 2];
                A1[3 * q] = a * s1;
                A1[3 * q + 1] = b * s1;
                A1[3 * q + 2] = (cc - (a * s1) * cx1) - (b * s1) * cy1;
            }
            const double is2 = 1.0 / s2;
            double Hh[9];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                Hh[j] = A1[j] * is2 + cx2 * A1[6 + j];
                Hh[3 + j] = A1[3 + j] * is2 + cy2 * A1[6 + j];
                Hh[6 + j] = A1[6 + j];
            }
            double fro = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) fro = fro + Hh[j] * Hh[j];
            double scl = 1.0 / sqrt(fro);
            if (Hh[8] < 0.0) scl = -scl;
            bool finite = true, same = true;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const double o = Hh[j] * scl;
                finite = finite && refit_h_finite(o);
                same = same && (__double_as_longlong(o) == __double_as_longlong(s_cur[j]));
                s_h[j] = o;
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
