// haf_propose.hip — one homography hypothesis per affine correspondence (mh_propose_haf), gfx950.
//
// Hypothesis s of a batch has counter c = first + s and anchor i = c * stride.  H0 is GetHomographyHAF of the anchor
// (M/MultiH.cpp:850-911), operation for operation what k_haf_point (reestimate.hip) writes for row i.  With members > 0 the
// first `members` entries of row i of the sampling table are tested against H0 (forward transfer error, strictly below thr2)
// and the consistent ones join the anchor in GetHomographyHAFNonminimal's least squares (:913-989): their ten A^T A terms are
// added to the anchor's one by one in table order, then the same eigen-solve and the same 1 / h33.  The definition is in
// include/multih_hip.h; tests/haf_propose_numpy.py re-enacts it.
//
// One lane per hypothesis, 64-lane workgroups: at 50 000 anchors that is 782 waves for 1 024 SIMDs, so nothing here is
// about occupancy and everything about the length of the dependent chain.  The row of the table is fetched whole (up to
// 32 independent loads), the neighbours' points for the test 16 at a time, and the eight doubles of a consistent
// neighbour eight neighbours at a time — a neighbour that failed the test re-reads the anchor's own row, which is in
// the cache.  Everything lives in registers under compile-time indices (the loops over j are unrolled to 32 and
// guarded by j < members); the second eigen-solve is skipped where no neighbour was consistent (the result is H0).

#include "mh_kernels.hpp"
#include "mh_device.hpp"

namespace mh {

namespace {

// the ten unique A^T A entries of ONE correspondence: s = r0a r0b, then s = s + rqa rqb for q = 1 .. 5
__device__ __forceinline__ void haf_terms(double a11, double a12, double a21, double a22, double px, double py, double qx,
                                          double qy, const double* F, double ex, double ey, double (&c)[10])
{
    double r[6][4];
    r[0][0] = a11 * px + qx - ex; r[0][1] = a11 * py;           r[0][2] = a11; r[0][3] = -F[3];
    r[1][0] = a12 * px;           r[1][1] = a12 * py + qx - ex; r[1][2] = a12; r[1][3] = -F[4];
    r[2][0] = a21 * px + qy - ey; r[2][1] = a21 * py;           r[2][2] = a21; r[2][3] = F[0];
    r[3][0] = a22 * px;           r[3][1] = a22 * py + qy - ey; r[3][2] = a22; r[3][3] = F[1];
    r[4][0] = ex * px - qx * px;  r[4][1] = ex * py - qx * py;  r[4][2] = ex - qx;
    r[4][3] = px * F[3] + py * F[4] + F[5];
    r[5][0] = ey * px - qy * px;  r[5][1] = ey * py - qy * py;  r[5][2] = ey - qy;
    r[5][3] = -(px * F[0] + py * F[1] + F[2]);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            double s = r[0][i] * r[0][j];
#pragma unroll
            for (int q = 1; q < 6; ++q) s = s + r[q][i] * r[q][j];
            c[k] = s;
            ++k;
        }
}

// ten sums -> H: the 4 x 4 eigen-solve, the column of the smallest eigenvalue (first index on ties), rows 1-2 from e2, F and
// lambda, times 1.0 / h33 (k_haf_point's tail)
__device__ __forceinline__ void haf_solve(const double (&u)[10], const double* F, double ex, double ey, double (&h)[9])
{
    double a[16], v[16], d[4];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) { a[i * 4 + j] = u[k]; a[j * 4 + i] = u[k]; ++k; }
    jacobi_sym_dev(4, a, v, d);
    double dm = d[0], h6 = v[0], h7 = v[4], h8 = v[8], lam = v[12];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const bool less = d[j] < dm;
        dm = less ? d[j] : dm;
        h6 = less ? v[0 * 4 + j] : h6;
        h7 = less ? v[1 * 4 + j] : h7;
        h8 = less ? v[2 * 4 + j] : h8;
        lam = less ? v[3 * 4 + j] : lam;
    }
    h[6] = h6; h[7] = h7; h[8] = h8;
    h[3] = ey * h6 - lam * F[0];
    h[4] = ey * h7 - lam * F[1];
    h[5] = ey * h8 - lam * F[2];
    h[0] = ex * h6 + lam * F[3];
    h[1] = ex * h7 + lam * F[4];
    h[2] = ex * h8 + lam * F[5];
    const double inv = 1.0 / h[8];                      // H = H / h33, cv::Mat / scalar scales by 1/s
#pragma unroll
    for (int q = 0; q < 9; ++q) h[q] = h[q] * inv;
}

constexpr int HAF_MAX_MEMBERS = 32, HAF_TEST_BATCH = 16, HAF_FIT_BATCH = 8;

} // namespace

__global__ void __launch_bounds__(64)
k_haf_propose(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
              const double* __restrict__ y2, const double* __restrict__ a11p, const double* __restrict__ a12p,
              const double* __restrict__ a21p, const double* __restrict__ a22p, int N, Epipolar ep,
              const int* __restrict__ nbr, int k, int members, double thr2, long long first, int m, int stride,
              double* __restrict__ H_out, unsigned* __restrict__ used_out)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= m) return;
    const long long anchor = (first + s) * (long long)stride;
    if (anchor < 0 || anchor >= N) return;                      // (the host has checked the whole range)
    const int i = (int)anchor;
    const double* F = ep.F;
    const double ex = ep.ex, ey = ep.ey;

    // the row of the table first: the anchor's own solve hides its latency
    int q[HAF_MAX_MEMBERS];
#pragma unroll
    for (int j = 0; j < HAF_MAX_MEMBERS; ++j) {
        int v = i;
        if (j < members) v = nbr[(size_t)i * k + j];
        q[j] = (unsigned)v < (unsigned)N ? v : i;                // a table entry is an index into the point set; never trust it blindly
    }

    double acc[10], h0[9];
    haf_terms(a11p[i], a12p[i], a21p[i], a22p[i], x1[i], y1[i], x2[i], y2[i], F, ex, ey, acc);
    haf_solve(acc, F, ex, ey, h0);

    unsigned used = 0;
#pragma unroll
    for (int b = 0; b < HAF_MAX_MEMBERS; b += HAF_TEST_BATCH) {
        if (b < members) {
            double px[HAF_TEST_BATCH], py[HAF_TEST_BATCH], qx[HAF_TEST_BATCH], qy[HAF_TEST_BATCH];
#pragma unroll
            for (int j = 0; j < HAF_TEST_BATCH; ++j) { px[j] = x1[q[b + j]]; py[j] = y1[q[b + j]]; qx[j] = x2[q[b + j]]; qy[j] = y2[q[b + j]]; }
#pragma unroll
            for (int j = 0; j < HAF_TEST_BATCH; ++j) {
                const double d2 = fwd_d2(h0[0], h0[1], h0[2], h0[3], h0[4], h0[5], h0[6], h0[7], h0[8], px[j], py[j], qx[j], qy[j]);
                used |= (b + j < members && d2 < thr2) ? 1u << (b + j) : 0u;      // strict; a NaN is not consistent
            }
        }
    }

    double h[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) h[t] = h0[t];
    if (used) {
#pragma unroll
        for (int b = 0; b < HAF_MAX_MEMBERS; b += HAF_FIT_BATCH) {
            if ((used >> b) & ((1u << HAF_FIT_BATCH) - 1u)) {
                double in[HAF_FIT_BATCH][8];
#pragma unroll
                for (int j = 0; j < HAF_FIT_BATCH; ++j) {
                    const int p = (used >> (b + j)) & 1u ? q[b + j] : i;
                    in[j][0] = a11p[p]; in[j][1] = a12p[p]; in[j][2] = a21p[p]; in[j][3] = a22p[p];
                    in[j][4] = x1[p]; in[j][5] = y1[p]; in[j][6] = x2[p]; in[j][7] = y2[p];
                }
#pragma unroll
                for (int j = 0; j < HAF_FIT_BATCH; ++j) {
                    if ((used >> (b + j)) & 1u) {                        // ascending j: the order of the definition
                        double c[10];
                        haf_terms(in[j][0], in[j][1], in[j][2], in[j][3], in[j][4], in[j][5], in[j][6], in[j][7], F, ex, ey, c);
#pragma unroll
                        for (int t = 0; t < 10; ++t) acc[t] = acc[t] + c[t];
                    }
                }
            }
        }
        haf_solve(acc, F, ex, ey, h);
    }
    double* out = H_out + 9 * (size_t)s;
#pragma unroll
    for (int t = 0; t < 9; ++t) out[t] = h[t];
    used_out[s] = used;
}

hipError_t launch_haf_propose(const Points& p, const Affines& a, const Epipolar& ep, const int* nbr, int k, int members,
                              double thr2, long long first, int m, int stride, double* H_out, unsigned* used_out, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_haf_propose, dim3((m + 63) / 64), dim3(64), 0, s, p.x1, p.y1, p.x2, p.y2, a.a11, a.a12, a.a21, a.a22,
                       p.n, ep, nbr, k, members, thr2, first, m, stride, H_out, used_out);
    return hipGetLastError();
}

} // namespace mh
