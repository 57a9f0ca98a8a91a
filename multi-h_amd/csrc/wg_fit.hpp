// wg_fit.hpp — what the per-model fit kernels share: k_fund_refit, k_moments, k_haf_reestimate, k_3pt_reestimate, k_refit_h,
// k_polish_h, k_dlt_reestimate, k_reweight_h and k_autoscale_reweight_h (k_label_quantile: the member loop; k_merge_pair: a pair of labels per workgroup).  One 256-thread workgroup per model, strided passes over the points, thread 0 solves.
//
// The order of every FP64 sum, stated here once: thread t adds its members t, t + 256, ... in ascending index from 0.0, then
// the binary tree v[t] += v[t + s], s = 128 .. 1, over the workgroup's LDS buffer (wg_tree).  The twins (oracle/mh_oracle.cpp
// TreeAcc, tests/*_numpy.py) add in the same order, which is what makes the results comparable bit for bit.  Which points are
// a thread's members is the kernel's business: an inlier test, or a label match (for_label_members).  -ffp-contract=off.
//
// fit(S), the normalised N-point DLT of include/multih_hip.h (mh_refit_homography; tests/refit_h_numpy.py::fit), in four pieces:
//     Hartley                          the six numbers of the two similarity normalisations
//     hartley_centroids / _scales      the sums of pass 1 / pass 2 -> these numbers, in every thread (hartley_distances: pass 2's term)
//     dlt_accumulate                   pass 3: one correspondence into the 24 sums G0..G3 over the six products p_a p_b
//     dlt_solve                        thread 0: the 9 x 9 normal matrix, cyclic Jacobi, k_dlt4's de-normalisation, norm and sign
// k_refit_h and k_dlt_reestimate are these pieces around their own membership and exits; k_fund_refit shares the first two.
// wfit(H), the same fit with every member's terms weighted (mh_reweight_homographies; k_reweight_h): the weighted steps stand
// beside the unweighted ones (hartley_centroids_w, hartley_distances_w, hartley_scales_w, dlt_accumulate_w); Hartley and
// dlt_solve serve both.  With every weight 1.0 they give the unweighted steps' bits (w * t is exact, the sum of the weights is c).
// (k_dlt_reestimate writes pass 1's counted tree out: as a call it changes the instructions of its label fetch.)
#pragma once
#include "mh_device.hpp"

namespace mh {

__device__ __forceinline__ bool finite_dev(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

// sv[t][0 .. K) += sv[t + s][0 .. K), s = 128 .. 1: the sums end in sv[0].  Every thread of the workgroup calls it.
template <int K, int W>
__device__ __forceinline__ void wg_tree(double (*sv)[W], int t)
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

// ... with the member counts sc[256] reduced in the same trips: the count ends in sc[0]
template <int K, int W>
__device__ __forceinline__ void wg_tree(double (*sv)[W], int (&sc)[256], int t)
{
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sv[t][k] = sv[t][k] + sv[t + s][k];
            sc[t] += sc[t + s];
        }
        __syncthreads();
    }
}

// The members of label l among thread t's points t, t + 256, ... in ascending index: the labels of BATCH of them are fetched
// per trip (BATCH independent loads in flight; most points carry another label), the matching ones visited in order.  Index
// is the type the point index is computed in (long long where N + 256 BATCH may pass 2^31).
template <int BATCH, class Index, class Fn>
__device__ __forceinline__ void for_label_members(const int* __restrict__ labels, int N, int l, int t, Fn&& f)
{
    for (Index n0 = t; n0 < N; n0 += (Index)256 * BATCH) {
        int lb[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const Index i = n0 + (Index)256 * j;
            lb[j] = labels[i < N ? i : 0];
        }
        unsigned match = 0;                      // bit j: point n0 + 256 j carries label l
#pragma unroll
        for (int j = 0; j < BATCH; ++j) match |= (n0 + (Index)256 * j < N && lb[j] == l) ? 1u << j : 0u;
        while (match) {                          // ascending j = ascending point index
            const int j = __builtin_ctz(match);
            match &= match - 1u;
            f((int)(n0 + (Index)256 * j));
        }
    }
}

// The two-label form (k_merge_pair): the members of label a OR label b, the same trips and the same ascending order; f gets the
// point and whether it carries b.
template <int BATCH, class Index, class Fn>
__device__ __forceinline__ void for_pair_members(const int* __restrict__ labels, int N, int a, int b, int t, Fn&& f)
{
    for (Index n0 = t; n0 < N; n0 += (Index)256 * BATCH) {
        int lb[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const Index i = n0 + (Index)256 * j;
            lb[j] = labels[i < N ? i : 0];
        }
        unsigned match = 0, is_b = 0;            // bit j: point n0 + 256 j carries a or b / carries b
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const bool in = n0 + (Index)256 * j < N;
            match |= (in && (lb[j] == a || lb[j] == b)) ? 1u << j : 0u;
            is_b |= (in && lb[j] == b) ? 1u << j : 0u;
        }
        while (match) {                          // ascending j = ascending point index
            const int j = __builtin_ctz(match);
            match &= match - 1u;
            f((int)(n0 + (Index)256 * j), (is_b >> j & 1u) != 0u);
        }
    }
}

// Hartley's normalisation of both images: centroids, and the scales that bring the mean distance to them to sqrt(2).
struct Hartley { double cx1, cy1, cx2, cy2, s1, s2; };

// Pass 1's four coordinate sums over the c members -> the centroids, in two steps: thread 0 writes par[0 .. 3] (LDS); behind a
// barrier every thread reads them.  (k_fund_refit calls the steps itself: its early exit stands between them.)
__device__ __forceinline__ void hartley_put_centroids(const double* sums, int c, double* par)
{
    const double inv = 1.0 / (double)c;
    par[0] = sums[0] * inv; par[1] = sums[1] * inv; par[2] = sums[2] * inv; par[3] = sums[3] * inv;
}

__device__ __forceinline__ void hartley_get_centroids(const double* par, Hartley& hn)
{
    hn.cx1 = par[0]; hn.cy1 = par[1]; hn.cx2 = par[2]; hn.cy2 = par[3];
}

// Both steps and the barrier between them.  Every thread calls it, behind the tree's last barrier.
__device__ __forceinline__ void hartley_centroids(const double* sums, int c, double* par, int t, Hartley& hn)
{
    if (t == 0) hartley_put_centroids(sums, c, par);
    __syncthreads();
    hartley_get_centroids(par, hn);
}

// The weight of a member at squared transfer error d2 (k_reweight_h, k_autoscale_reweight_h): one IEEE division, one
// subtraction; 0 at and beyond c2 and for a NaN.
__device__ __forceinline__ double reweight_w(double d2, double c2) { return d2 < c2 ? 1.0 - (d2 / c2) : 0.0; }

// ... weighted: the four sums of w * coordinate and W, the sum of the weights
__device__ __forceinline__ void hartley_centroids_w(const double* sums, double W, double* par, int t, Hartley& hn)
{
    if (t == 0) {
        const double inv = 1.0 / W;
        par[0] = sums[0] * inv; par[1] = sums[1] * inv; par[2] = sums[2] * inv; par[3] = sums[3] * inv;
    }
    __syncthreads();
    hartley_get_centroids(par, hn);
}

// pass 2's term of one member: its distances to the two centroids
__device__ __forceinline__ void hartley_distances(const Hartley& hn, double x, double y, double u, double v, double& d1, double& d2)
{
    const double ax = x - hn.cx1, ay = y - hn.cy1, bx = u - hn.cx2, by = v - hn.cy2;
    d1 = d1 + sqrt(ax * ax + ay * ay);
    d2 = d2 + sqrt(bx * bx + by * by);
}

// ... weighted by w
__device__ __forceinline__ void hartley_distances_w(const Hartley& hn, double w, double x, double y, double u, double v, double& d1,
                                                    double& d2)
{
    const double ax = x - hn.cx1, ay = y - hn.cy1, bx = u - hn.cx2, by = v - hn.cy2;
    d1 = d1 + w * sqrt(ax * ax + ay * ay);
    d2 = d2 + w * sqrt(bx * bx + by * by);
}

// Pass 2's two distance sums -> the scales, in par[4], par[5] and hn; called like hartley_centroids.
__device__ __forceinline__ void hartley_scales(const double* sums, int c, double* par, int t, Hartley& hn)
{
    if (t == 0) {
        par[4] = sqrt(2.0) / (sums[0] / (double)c);
        par[5] = sqrt(2.0) / (sums[1] / (double)c);
    }
    __syncthreads();
    hn.s1 = par[4]; hn.s2 = par[5];
}

// ... from the weighted distance sums and W
__device__ __forceinline__ void hartley_scales_w(const double* sums, double W, double* par, int t, Hartley& hn)
{
    if (t == 0) {
        par[4] = sqrt(2.0) / (sums[0] / W);
        par[5] = sqrt(2.0) / (sums[1] / W);
    }
    __syncthreads();
    hn.s1 = par[4]; hn.s2 = par[5];
}

constexpr int DLT_SUMS = 24;                     // G0 | G1 | G2 | G3, six each: sums of p_a p_b times 1, u, v, u u + v v
constexpr int DLT_WORK = 171;                    // A (81), V (81), D (9) of the solve

// pass 3's term of one member (x, y) -> (u, v), normalised here
__device__ __forceinline__ void dlt_accumulate(const Hartley& hn, double x0, double y0, double u0, double v0, double (&acc)[DLT_SUMS])
{
    const double x = (x0 - hn.cx1) * hn.s1, y = (y0 - hn.cy1) * hn.s1, u = (u0 - hn.cx2) * hn.s2, v = (v0 - hn.cy2) * hn.s2;
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

// ... weighted: every term of the member carries wt = w * (p_a p_b)
__device__ __forceinline__ void dlt_accumulate_w(const Hartley& hn, double wgt, double x0, double y0, double u0, double v0,
                                                 double (&acc)[DLT_SUMS])
{
    const double x = (x0 - hn.cx1) * hn.s1, y = (y0 - hn.cy1) * hn.s1, u = (u0 - hn.cx2) * hn.s2, v = (v0 - hn.cy2) * hn.s2;
    const double p[3] = { x, y, 1.0 };
    const double w = u * u + v * v;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            const double tt = p[a] * p[b];
            const double wt = wgt * tt;
            acc[k] = acc[k] + wt;
            acc[6 + k] = acc[6 + k] + u * wt;
            acc[12 + k] = acc[12 + k] + v * wt;
            acc[18 + k] = acc[18 + k] + w * wt;
            ++k;
        }
}

// One thread: the 24 sums G -> the nine doubles h of the fit, unit Frobenius norm, h[8] >= 0 (finite or not: the caller's
// test).  jacobi_sym_dev indexes A and V by run-time p, q: as private arrays they would live in scratch memory, so they stand
// in `work` (DLT_WORK doubles), for which the callers hand in their LDS reduction buffer, idle once the tree has run and G has
// been copied out of it.
__device__ __forceinline__ void dlt_solve(const double* G, const Hartley& hn, double* work, double (&h)[9])
{
    double* A = work;
    double* V = A + 81;
    double* D = V + 81;
    for (int i = 0; i < 81; ++i) A[i] = 0.0;
    {
        int k = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                const double g0 = G[k], g1 = -G[6 + k], g2 = -G[12 + k], g3 = G[18 + k];
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
        A1[3 * q] = a * hn.s1;
        A1[3 * q + 1] = b * hn.s1;
        A1[3 * q + 2] = (cc - (a * hn.s1) * hn.cx1) - (b * hn.s1) * hn.cy1;
    }
    const double is2 = 1.0 / hn.s2;
    double Hh[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Hh[j] = A1[j] * is2 + hn.cx2 * A1[6 + j];
        Hh[3 + j] = A1[3 + j] * is2 + hn.cy2 * A1[6 + j];
        Hh[6 + j] = A1[6 + j];
    }
    double fro = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) fro = fro + Hh[j] * Hh[j];
    double scl = 1.0 / sqrt(fro);
    if (Hh[8] < 0.0) scl = -scl;
#pragma unroll
    for (int j = 0; j < 9; ++j) h[j] = Hh[j] * scl;
}

} // namespace mh
