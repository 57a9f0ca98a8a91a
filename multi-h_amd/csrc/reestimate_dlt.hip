// reestimate_dlt.hip — per-label normalised N-point DLT re-estimation from points alone, gfx950 (mh_set_estimator(MH_ESTIMATOR_DLT)).
//
// H[k] = fit(S_k), S_k = { i : labels[i] == k }, with fit(S) the rule stated operation by operation under mh_refit_homography in
// include/multih_hip.h (tests/refit_h_numpy.py::fit is its numpy twin): k_refit_h's arithmetic (refit_h.hip) with the label's
// members in the place of a model's inliers, and no rounds, no acceptance test.  Neither F, the epipole nor the affinities are
// read: this is the re-estimator of the route without epipolar geometry, the counterpart of k_haf_reestimate and k_3pt_reestimate.
//
// One workgroup of 256 per label.  Members are found by the match loop of k_haf_reestimate: thread t visits i = t, t + 256, ...
// in ascending order and compares labels[i] (the labels of DLT_BATCH of its points fetched per trip, the matching ones visited in
// order).  That lane assignment IS the engine's order of every FP64 sum (thread t adds the members with index = t mod 256 in
// ascending index from 0.0, then the binary tree 128 .. 1), so a compacted member list is not an option here.  Three passes:
//     1  member count and the four centroid sums
//     2  the two mean distances to the centroids -> the scales
//     3  the 24 sums G0..G3 over the six products p_a p_b
// then thread 0 runs the 9 x 9 cyclic Jacobi (jacobi_sym_dev) and k_dlt4's de-normalisation.  A, V and D of the solve stand in the
// LDS reduction buffer, idle once the tree has run (the 24 sums are copied out first), as in k_refit_h: no private array with a
// run-time index, no scratch memory.  A label whose fit fails (fewer than 4 members, a scale that is not finite, an entry of the
// result that is not finite) keeps its nine doubles.  counts[k] = |S_k|.
// Loops are bounded by N and by Jacobi's 30 sweeps; the workgroup waits for nothing but its own barriers, and every exit is
// uniform over the workgroup.  -ffp-contract=off.

#include "mh_kernels.hpp"
#include "mh_device.hpp"

namespace mh {

namespace {

constexpr int DLT_SUMS = 24;
constexpr int DLT_BATCH = 16;

// v[t][0 .. K) += v[t + s][0 .. K), s = 128 .. 1; every thread of the workgroup calls it
template <int K>
__device__ __forceinline__ void dlt_tree(double (*sv)[DLT_SUMS], int t)
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

__device__ __forceinline__ bool dlt_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

// the members of label l among the points t, t + 256, ... in ascending order
template <class Fn>
__device__ __forceinline__ void dlt_members(const int* __restrict__ labels, int N, int l, int t, Fn&& f)
{
    for (long long n0 = t; n0 < N; n0 += 256ll * DLT_BATCH) {
        int lb[DLT_BATCH];
#pragma unroll
        for (int j = 0; j < DLT_BATCH; ++j) {
            const long long i = n0 + 256ll * j;
            lb[j] = labels[i < N ? i : 0];
        }
        unsigned match = 0;
#pragma unroll
        for (int j = 0; j < DLT_BATCH; ++j) match |= (n0 + 256ll * j < N && lb[j] == l) ? 1u << j : 0u;
        while (match) {
            const int j = __builtin_ctz(match);
            match &= match - 1u;
            f((int)(n0 + 256ll * j));
        }
    }
}

} // namespace

__global__ void __launch_bounds__(256)
k_dlt_reestimate(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                 const double* __restrict__ y2, const int* __restrict__ labels, int N, double* __restrict__ H,
                 int* __restrict__ counts)
{
    const int l = blockIdx.x, t = threadIdx.x;
    __shared__ double sv[256][DLT_SUMS];         // 48 KB: the partial sums; then A (81), V (81), D (9) of the solve
    __shared__ int sc[256];
    __shared__ double s_par[6];                  // cx1 cy1 cx2 cy2 s1 s2
    __shared__ double s_G[DLT_SUMS];

    // pass 1
    {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int cnt = 0;
        dlt_members(labels, N, l, t, [&](int n) {
            a0 = a0 + x1[n]; a1 = a1 + y1[n]; a2 = a2 + x2[n]; a3 = a3 + y2[n];
            ++cnt;
        });
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
    if (t == 0 && counts) counts[l] = c;
    if (c < 4) return;                           // keeps its H (c is the same in every thread)
    if (t == 0) {
        const double inv = 1.0 / (double)c;
        s_par[0] = sv[0][0] * inv; s_par[1] = sv[0][1] * inv; s_par[2] = sv[0][2] * inv; s_par[3] = sv[0][3] * inv;
    }
    __syncthreads();
    const double cx1 = s_par[0], cy1 = s_par[1], cx2 = s_par[2], cy2 = s_par[3];
    // pass 2
    {
        double d1 = 0.0, d2 = 0.0;
        dlt_members(labels, N, l, t, [&](int n) {
            const double ax = x1[n] - cx1, ay = y1[n] - cy1, bx = x2[n] - cx2, by = y2[n] - cy2;
            d1 = d1 + sqrt(ax * ax + ay * ay);
            d2 = d2 + sqrt(bx * bx + by * by);
        });
        sv[t][0] = d1; sv[t][1] = d2;
        dlt_tree<2>(sv, t);
        if (t == 0) {
            s_par[4] = sqrt(2.0) / (sv[0][0] / (double)c);
            s_par[5] = sqrt(2.0) / (sv[0][1] / (double)c);
        }
        __syncthreads();
    }
    const double s1 = s_par[4], s2 = s_par[5];
    if (!dlt_finite(s1) || !dlt_finite(s2)) return;                      // keeps its H (the same for every thread)
    // pass 3
    {
        double acc[DLT_SUMS];
#pragma unroll
        for (int k = 0; k < DLT_SUMS; ++k) acc[k] = 0.0;
        dlt_members(labels, N, l, t, [&](int n) {
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
        });
#pragma unroll
        for (int k = 0; k < DLT_SUMS; ++k) sv[t][k] = acc[k];
        dlt_tree<DLT_SUMS>(sv, t);
    }
    if (t < DLT_SUMS) s_G[t] = sv[0][t];
    __syncthreads();                             // the reduction buffer is idle from here: A, V, D of the solve stand in it
    if (t != 0) return;                          // (no barrier follows)

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
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        Hh[j] = Hh[j] * scl;
        finite = finite && dlt_finite(Hh[j]);
    }
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
