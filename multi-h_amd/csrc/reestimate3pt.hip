// reestimate3pt.hip — per-label 3-point least-squares homography re-estimation from points alone, gfx950.
//
// GetHomography3PT without its LM refinement (M/MultiH.cpp:995-1050; the host twin is multih::Homography3PTLinear,
// host/merge_step.cpp) for every label in one pass: H = [e']x F + e' v^T, so only the third row v of the normalised H is
// unknown, and it is the least-squares solution over ALL the label's members (n >= 3).  The affinities are not read: this is
// the re-estimator of the point-only route (mh_set_estimator(MH_ESTIMATOR_3PT)), the counterpart of k_haf_reestimate.
//
// Members first, in one of two forms chosen by size (launch_reestimate_3pt).  Few labels: a stable counting sort compacts the
// member indices of every label once, so a label's workgroup reads only its own points:
//   k_3pt_block_count  per block of 256 points: the rank of each point among the earlier points of its block with the same
//                      label, found by a broadcast scan of the block's labels in LDS; the last member of a label in the block
//                      writes the block's count into cnt[label * blocks + block] (label-major)
//   k_3pt_scan         one workgroup: exclusive prefix sum of cnt in place (label-major, blocks ascending), total behind it
//   k_3pt_scatter      members[cnt[label * blocks + block] + rank] = point
// so label l's members lie in members[cnt[l * blocks] .. cnt[(l + 1) * blocks]) in ascending point index.  Many labels: the
// single scan of labels x blocks counts costs more than it saves, and each workgroup finds its members by the match loop
// instead (wg_fit.hpp's for_label_members: 32 labels per trip, three passes).
//
// Then k_3pt_reestimate, one workgroup of 256 per label, three sums in the engine's deterministic FP64 order (wg_fit.hpp: thread t adds
// the label's members t, t + 256, ... in ascending order, then the LDS binary tree):
//   1. the centroids of both images (with the member count, for the match loop) (NormalizePoints, Homography_Refine3PTCallback.h:161-196),
//   2. the mean distances to them -> ratio = sqrt(2) / mean,
//   3. the normal equations of the 2n x 3 system (:1019-1037): A^T A (6 unique entries) and A^T b (3), two rows per point.
// Between the sums every thread derives the same scalars from the same LDS words (T1, T2, Fn = T2^-T F T1^-1 and the
// epipole of Fn, the eigenvector of Fn Fn^T with the smallest eigenvalue through jacobi_sym_dev).  Thread 0 solves the 3 x 3
// system by the pseudo-inverse through its eigen-decomposition (eigenvalues within 2 eps sum|w| of zero dropped, as
// sym_eig_solve3 does), builds Hn (:1040-1050) and H = T2^-1 Hn T1.  A label with fewer than 3 members keeps its H (the
// reference keeps an empty label's model, :592-593); so does a label whose fit is not finite.  counts[l] = member count.
// The host's sums run from 0.0 in index order, so the two agree to rounding, not bit for bit; so do the two forms.

#include "mh_kernels.hpp"
#include "wg_fit.hpp"

#include <algorithm>

namespace mh {

namespace {

constexpr int R3_BLOCK = 256;
constexpr size_t R3_COMPACT_MAX = 8192;      // block counts (labels x blocks of 256 points) up to which the lists are compacted

// rank of point i among the earlier points of its block with the same label, and whether it is the block's last such point
__device__ __forceinline__ void block_rank(const int* sl, int t, int l, int& rank, bool& last)
{
    int r = 0;
    bool lst = true;
    for (int j = 0; j < R3_BLOCK; ++j) {            // every lane reads the same word: an LDS broadcast
        const int lj = sl[j];
        r += (j < t && lj == l) ? 1 : 0;
        lst = lst && !(j > t && lj == l);
    }
    rank = r;
    last = lst;
}

// v[k][t] summed over t by the fixed binary tree; every thread returns with the sums in v[k][0].  The transposed twin of
// wg_fit.hpp's wg_tree: this kernel keeps its sums as [K][256].
template <int K>
__device__ __forceinline__ void tree_sum(double (*v)[R3_BLOCK], int t)
{
    __syncthreads();
    for (int s = R3_BLOCK / 2; s >= 1; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) v[k][t] = v[k][t] + v[k][t + s];
        }
        __syncthreads();
    }
}

} // namespace

__global__ void __launch_bounds__(R3_BLOCK)
k_3pt_block_count(const int* __restrict__ labels, int N, int Nh, int* __restrict__ cnt)
{
    __shared__ int sl[R3_BLOCK];
    const int t = threadIdx.x, b = blockIdx.x, blocks = gridDim.x;
    const int i = b * R3_BLOCK + t;
    for (int l = t; l < Nh; l += R3_BLOCK) cnt[(size_t)l * blocks + b] = 0;   // this block's column
    const int l = i < N ? labels[i] : -1;
    sl[t] = (l >= 0 && l < Nh) ? l : -1;
    __syncthreads();                                                        // (also orders the zeroing before the counts)
    if (sl[t] < 0) return;
    int rank;
    bool last;
    block_rank(sl, t, sl[t], rank, last);
    if (last) cnt[(size_t)sl[t] * blocks + b] = rank + 1;
}

// exclusive prefix sum of cnt[0 .. total) in place, cnt[total] = the sum; one workgroup of 1024
__global__ void __launch_bounds__(1024)
k_3pt_scan(int* __restrict__ cnt, int total)
{
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (total + 1023) / 1024;
    const int lo = min(t * per, total), hi = min(lo + per, total);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += cnt[k];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                                    // inclusive Hillis-Steele scan of the partials
        const int add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - s;                                                  // exclusive
    for (int k = lo; k < hi; ++k) { const int c = cnt[k]; cnt[k] = run; run += c; }
    if (t == 1023) cnt[total] = part[1023];
}

__global__ void __launch_bounds__(R3_BLOCK)
k_3pt_scatter(const int* __restrict__ labels, int N, int Nh, const int* __restrict__ start, int* __restrict__ members)
{
    __shared__ int sl[R3_BLOCK];
    const int t = threadIdx.x, b = blockIdx.x, blocks = gridDim.x;
    const int i = b * R3_BLOCK + t;
    const int l = i < N ? labels[i] : -1;
    sl[t] = (l >= 0 && l < Nh) ? l : -1;
    __syncthreads();
    if (sl[t] < 0) return;
    int rank;
    bool last;
    block_rank(sl, t, sl[t], rank, last);
    members[start[(size_t)sl[t] * blocks + b] + rank] = i;
}

// The members of label l in ascending point index, lane t taking every 256th: from the compacted list (COMPACT), or by
// the match loop (for_label_members: lane t then takes the members among the points t, t + 256, ...).  The two forms order
// the sums differently.
template <bool COMPACT, class Fn>
__device__ __forceinline__ void for_members(const int* mem, int n, const int* labels, int N, int l, int t, Fn&& f)
{
    if constexpr (COMPACT) {
        for (int k = t; k < n; k += R3_BLOCK) f(mem[k]);
    } else {
        for_label_members<32, int>(labels, N, l, t, f);
    }
}

template <bool COMPACT>
__global__ void __launch_bounds__(R3_BLOCK)
k_3pt_reestimate(const double* __restrict__ x1p, const double* __restrict__ y1p, const double* __restrict__ x2p,
                 const double* __restrict__ y2p, const int* __restrict__ labels, int N, const int* __restrict__ members,
                 const int* __restrict__ start, int blocks, Epipolar ep, double* __restrict__ H, int* __restrict__ counts)
{
    __shared__ double sv[9][R3_BLOCK];
    const int l = blockIdx.x, t = threadIdx.x;
    int beg = 0, n = 0;
    if (COMPACT) {
        beg = start[(size_t)l * blocks];
        n = start[(size_t)(l + 1) * blocks] - beg;
        if (n < 3) {                                         // keeps its H (uniform over the workgroup)
            if (t == 0 && counts) counts[l] = n;
            return;
        }
    }
    const int* mem = COMPACT ? members + beg : nullptr;

    // 1. centroids (and, for the match loop, the member count)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = 0;
    for_members<COMPACT>(mem, n, labels, N, l, t, [&](int i) {
        s0 = s0 + x1p[i]; s1 = s1 + y1p[i]; s2 = s2 + x2p[i]; s3 = s3 + y2p[i];
        ++c;
    });
    sv[0][t] = s0; sv[1][t] = s1; sv[2][t] = s2; sv[3][t] = s3; sv[4][t] = (double)c;
    tree_sum<5>(sv, t);
    if (!COMPACT) n = (int)sv[4][0];
    if (t == 0 && counts) counts[l] = n;
    if (n < 3) return;                                       // keeps its H (n is the same in every thread)
    const double invn = 1.0 / (double)n;
    const double c1x = invn * sv[0][0], c1y = invn * sv[1][0], c2x = invn * sv[2][0], c2y = invn * sv[3][0];
    __syncthreads();                                         // everyone has read the sums before sv is reused

    // 2. mean distances to the centroids
    double d1 = 0.0, d2 = 0.0;
    for_members<COMPACT>(mem, n, labels, N, l, t, [&](int i) {
        const double ax = x1p[i] - c1x, ay = y1p[i] - c1y, bx = x2p[i] - c2x, by = y2p[i] - c2y;
        d1 = d1 + sqrt(ax * ax + ay * ay);
        d2 = d2 + sqrt(bx * bx + by * by);
    });
    sv[0][t] = d1; sv[1][t] = d2;
    tree_sum<2>(sv, t);
    const double r1 = sqrt(2.0) / (sv[0][0] / n), r2 = sqrt(2.0) / (sv[1][0] / n);
    __syncthreads();

    // T = [r 0 -c r; 0 r -c r; 0 0 1]; Fn = T2^-T F T1^-1 and its epipole
    const double T1[9] = { r1, 0, -c1x * r1, 0, r1, -c1y * r1, 0, 0, 1 };
    const double T2[9] = { r2, 0, -c2x * r2, 0, r2, -c2y * r2, 0, 0, 1 };
    double T2i[9], Fn[9], e0, e1;
    normalised_epipolar_dev(ep.F, T1, T2, T2i, Fn, e0, e1);

    // 3. normal equations, rows 2k and 2k + 1 of point k in that order
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[q] = 0.0;
    for_members<COMPACT>(mem, n, labels, N, l, t, [&](int i) {
        const double x1 = (x1p[i] - c1x) * r1, y1 = (y1p[i] - c1y) * r1;
        const double x2 = (x2p[i] - c2x) * r2, y2 = (y2p[i] - c2y) * r2;
        const double ra[3] = { e0 * x1 - x2 * x1, e0 * y1 - x2 * y1, e0 - x2 };
        const double rb[3] = { e1 * x1 - y2 * x1, e1 * y1 - y2 * y1, e1 - y2 };
        const double ba = -(x1 * Fn[3] + y1 * Fn[4] + Fn[5]);
        const double bb = (x1 * Fn[0] + y1 * Fn[1] + Fn[2]);
        int q = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b) { acc[q] = acc[q] + ra[a] * ra[b]; acc[q] = acc[q] + rb[a] * rb[b]; ++q; }
#pragma unroll
        for (int a = 0; a < 3; ++a) { acc[6 + a] = acc[6 + a] + ra[a] * ba; acc[6 + a] = acc[6 + a] + rb[a] * bb; }
    });
#pragma unroll
    for (int q = 0; q < 9; ++q) sv[q][t] = acc[q];
    tree_sum<9>(sv, t);
    if (t != 0) return;

    double AtA[9], Atb[3], h3[3], Ho[9];
    AtA[0] = sv[0][0]; AtA[1] = sv[1][0]; AtA[2] = sv[2][0];
    AtA[3] = sv[1][0]; AtA[4] = sv[3][0]; AtA[5] = sv[4][0];
    AtA[6] = sv[2][0]; AtA[7] = sv[4][0]; AtA[8] = sv[5][0];
    Atb[0] = sv[6][0]; Atb[1] = sv[7][0]; Atb[2] = sv[8][0];
    sym_eig_solve3_dev(AtA, Atb, h3);
    if (!assemble_3pt_dev(h3, e0, e1, Fn, T1, T2i, Ho)) return;      // not finite: keeps its H
    double* out = H + 9 * (size_t)l;
    for (int q = 0; q < 9; ++q) out[q] = Ho[q];
}

size_t reestimate_3pt_scratch_ints(int n, int Nh)
{
    const size_t blocks = (size_t)std::max((n + R3_BLOCK - 1) / R3_BLOCK, 1);
    return (size_t)Nh * blocks + 1 + (size_t)std::max(n, 1);
}

hipError_t launch_reestimate_3pt(const Points& p, const int* labels, int Nh, const Epipolar& ep, double* H, int* counts,
                                 int* scratch, hipStream_t s, int form)
{
    if (Nh <= 0) return hipSuccess;
    const int blocks = std::max((p.n + R3_BLOCK - 1) / R3_BLOCK, 1);
    const size_t total = (size_t)Nh * blocks;
    // The faster form by the size of the compaction's one-workgroup scan (tools/points_only_bench.py, MI355X, medians of 21):
    // 50 000 points x 11 labels (2 156 block counts) 71.5 us compacted against 87.2 us by the match loop; 20 000 x 540
    // (42 660 block counts) 112 us against 48.6 us.
    if (form == 0) form = total <= R3_COMPACT_MAX ? 2 : 1;
    if (form == 1) {                             // the match loop over the whole label array
        hipLaunchKernelGGL(k_3pt_reestimate<false>, dim3(Nh), dim3(R3_BLOCK), 0, s, p.x1, p.y1, p.x2, p.y2, labels, p.n,
                           nullptr, nullptr, 0, ep, H, counts);
        return hipGetLastError();
    }
    if (total >= (size_t)0x7fffffff) return hipErrorInvalidValue;
    int* start = scratch;                        // Nh x blocks + 1
    int* members = scratch + total + 1;          // n
    hipLaunchKernelGGL(k_3pt_block_count, dim3(blocks), dim3(R3_BLOCK), 0, s, labels, p.n, Nh, start);
    hipLaunchKernelGGL(k_3pt_scan, dim3(1), dim3(1024), 0, s, start, (int)total);
    hipLaunchKernelGGL(k_3pt_scatter, dim3(blocks), dim3(R3_BLOCK), 0, s, labels, p.n, Nh, start, members);
    hipLaunchKernelGGL(k_3pt_reestimate<true>, dim3(Nh), dim3(R3_BLOCK), 0, s, p.x1, p.y1, p.x2, p.y2, labels, p.n, members, start,
                       blocks, ep, H, counts);
    return hipGetLastError();
}

} // namespace mh
