// pretest32.hpp — the FP32 pre-test of the score kernels, gfx950: the test, its bound and its launch rules, each stated once
// for its consumers (k_score32*, k_cost32* / k_rising32* of score32.hip, k_msac32 of msac32.hip).  Counts are the
// reference's, bit for bit.
//
// A score needs, per (point, model) pair, only the DECISION  d2 < thr^2  of the reference's FP64 formula
// (M/MultiH.cpp:434-443), never d2 itself.  This kernel evaluates the forward transfer error in FP32 (fused
// multiply-adds, hardware reciprocal: about a third of the FP64 sweep's issue cycles per pair) together with a RIGOROUS
// bound B on |d2_fp32 - d2_fp64|, decides the pairs for which the bound leaves no doubt
//         d2_fp32 + B <  thr^2   ->  inlier            d2_fp32 - B >= thr^2   ->  not an inlier
// (evaluated as |d2_fp32 - thr^2| > B with the sign of the difference telling which)
// and recomputes the others — pairs within B of the threshold, pairs near a model's horizon, anything that produced a
// NaN or an infinity on the way — with the FP64 formula in the reference's own operation order.  The result is the count
// the FP64 kernel (residual.hip) gives; the tests compare the two and put thresholds exactly ON residual values.
//
// The bound.  u = 2^-24.  Inputs are rounded to FP32 (relative error u each).  With X, Y = max |x|, |y| over all source
// points, per MODEL (k_model32, in FP64, rounded up):
//     E_s = 5u (|h6| X + |h7| Y + |h8|)          bounds |s_fp32 - s|   (two fmas on rounded inputs: (1+u)^4 - 1 < 5u)
//     E_n = 5u max(|h0| X + |h1| Y + |h2|, |h3| X + |h4| Y + |h5|)     the same for both numerators
// per PAIR, from the FP32 values (sigma = |s_fp32|, r = rcp(s_fp32) with |r sigma - 1| <= 3u, m = max(|u|, |v|)):
//     a pair is only decided in FP32 if sigma >= 64 E_s  (then the true |s| >= 63/64 sigma and the quotient's error is
//     first-order); the quotient n/s computed as n_fp32 * r then errs by at most
//         E_q = 1.1 (E_n + m E_s) |r| + 5u m                                     (1.1 covers 64/63, the reciprocal's
//                                                                                 3u and the second-order term)
//     dx = x2 - u errs by   E = E_q + u max(|x2|, |y2|) + 1.01u max(|dx|, |dy|)  (input rounding, the subtraction)
//     d2 = dx^2 + dy^2 errs by   B32 <= 2 E (2 max(|dx|, |dy|) + E) + 2.2u d2
// The FP64 value the reference computes differs from the exact one by the same expressions with 2^-53 for u (a few more
// roundings, no fma): less than 2^-27 B32.  B = 1.01 B32 covers that and the rounding of the bound's own evaluation (a
// dozen FP32 operations, every term non-negative).  Models or points outside the magnitudes for which "relative error
// u per operation" holds (overflow, underflow to subnormals) are not eligible: a model with a coefficient >= 2^100, not
// finite, or with E_s or E_n below 2^-80 gets tau = NaN (every comparison against it is false) and all its pairs go to FP64; the launcher uses this kernel
// only when every coordinate is finite and below 2^20 in magnitude.  A NaN anywhere makes both comparisons false, which
// also sends the pair to FP64.
//
// Most pairs are nowhere near the threshold — a random hypothesis maps a point hundreds of pixels from its match — and
// for them a much cheaper sufficient test decides "not an inlier" before d2, or even a quotient, is formed.  It works on
//         Wx = x2 s - nx = s dx,     Wy = y2 s - ny = s dy          (one fma each; no reciprocal)
// With Cmax = max |x2|, |y2| over all points, the computed Wx^ = fl(x2~ s~ - nx~) satisfies
//         |Wx^ - Wx| <= Cmax (1+u) E_s + E_n + u Cmax |s| + 1.01u |Wx^|         (s~, nx~ as above, x2~ = fl32(x2), the fma's rounding)
// so with the per-model constant A = 1.01 (Cmax E_s + E_n) and W^ = max(|Wx^|, |Wy^|), if
//         sigma >= 64 E_s,     W^ >= 1.12 thr sigma,     W^ >= 25 A,     W^ >= 25.4 u Cmax sigma
// then (|s| <= 65/64 sigma) the true max(|dx|, |dy|) = max(|Wx|, |Wy|) / |s| is at least
//         W^ (1 - 1.01u - 0.04 - 0.04) / (65/64 sigma) >= 0.9057 W^ / sigma >= 1.014 thr
// and the true d2 at least 1.028 thr^2 — a margin of 2.8 % against the 2^-50 by which the reference's own roundings can move
// d2.  (The factor was 2.5 at first; hypotheses fitted to four matches are often nearly right for a whole plane, 3 % of
// the pairs of a DLT batch lie within 5 pixels, and every pair that fails this test costs the full bound below.)  The second and fourth condition are one comparison against k1 sigma with the
// per-launch constant k1 = max(1.12 thr, 25.4 u Cmax) (rounded up); the third against the per-model constant 25.2 A.
// Products cannot overflow: eligible models have |h6| X + |h7| Y + |h8| and both numerators' sums below 2^100 and
// coordinates are below 2^20; they do not underflow into the subnormals either where it matters: W^ >= k1 sigma with
// sigma >= 2^-74 (E_s >= 2^-80) and thr^2 >= 2^-40 (the launcher's precondition) is a normal number.  When all 64 lanes
// of a wave pass this for a pair, the wave moves on (a wave-uniform branch); otherwise the pair takes the full bound.
// (Until late r03 this test was formed on the quotient, with a reciprocal and two multiplies more per pair.)
//
// An FP32 instruction with a scalar-register operand issues in 4 cycles, with vector operands only in 2
// (tools/ubench/valu_cost.hip), so the per-model constants are staged in LDS once per workgroup and broadcast into
// VGPRs per model (LDS instructions do not take VALU issue slots).
//
// Work split as k_residual: a 256-thread workgroup owns MC models (64 by default) and sweeps a slice of the points, a lane
// holds PPL = 4 points.
#pragma once
#include "mh_kernels.hpp"
#include "mh_device.hpp"

#include <cmath>

namespace mh {

constexpr float U32 = 5.9604644775390625e-08f;       // 2^-24

// ---- device side ---------------------------------------------------------------------------------------------------

// a kernel-argument constant that enters FP32 instructions: a VGPR copy, made once
__device__ __forceinline__ float vgpr_copy(float v)
{
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(v));
    return r;
}

// acc with add added to its lane mi (add and mi wave-uniform): lane mi of each wave accumulates model m0 + mi.  (Returned, not
// an int&: through a reference the model loop of the cost kernels came out with another latch — DESIGN 3.2.)
__device__ __forceinline__ int lane_acc_add(int acc, int mi, int add)
{
    const int v = __builtin_amdgcn_readlane(acc, mi) + add;
    asm("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %1, m0" : "+v"(acc) : "s"(v), "s"(mi) : "m0");
    return acc;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the pairs a wave's lanes sent through the FP64 formula, added to the device counter of mh_get_score_stats (nullable)
__device__ __forceinline__ void add_fp64_pairs(unsigned long long* __restrict__ counter, unsigned long long fb)
{
    if (counter) {
        fb = wave_sum(fb);
        if ((threadIdx.x & 63) == 0 && fb) atomicAdd(counter, fb);
    }
}

// A model's row of the k_model32 table: 9 coefficients in FP32, then 1.1 E_s, 1.1 E_n, tau = 64 E_s (or NaN: not eligible),
// 25.2 A (the cheap test), 3 pad.
struct Model32 {
    float h0, h1, h2, h3, h4, h5, h6, h7, h8, es, en, tau, a25;
};

// this workgroup's MC rows of the table into LDS (the caller's barrier follows); rows past M get tau = NaN
template <int MC, int THREADS>
__device__ __forceinline__ void stage_model32(float4* s_m, const float* __restrict__ H32, int m0, int M)
{
    for (int i = threadIdx.x; i < MC * 4; i += THREADS) {
        const size_t g = (size_t)m0 * 4 + i;
        s_m[i] = g < (size_t)M * 4 ? reinterpret_cast<const float4*>(H32)[g] : make_float4(0.f, 0.f, 0.f, NAN);
    }
}

// ... and their FP64 coefficients, for the lanes that need the reference's formula
template <int MC, int THREADS>
__device__ __forceinline__ void stage_model64(double* s_h, const double* __restrict__ H, int m0, int M)
{
    for (int i = threadIdx.x; i < MC * 9; i += THREADS) {
        const size_t g = (size_t)m0 * 9 + i;
        s_h[i] = g < (size_t)M * 9 ? H[g] : 0.0;
    }
}

// broadcast LDS reads: every lane gets the model's constants in VGPRs
__device__ __forceinline__ Model32 model32_from_lds(const float4* s_m, int mi)
{
    const float4 ma = s_m[4 * mi], mb = s_m[4 * mi + 1], mc = s_m[4 * mi + 2], md = s_m[4 * mi + 3];
    return { ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w, mc.x, mc.y, mc.z, mc.w, md.x };
}

// The FP32 copies of a lane's PPL points, padding lanes (n >= N) at 1.0; each(q, in_range, x1, y1, x2, y2) sees every
// point's FP64 values on the way.
template <int PPL, typename Each>
__device__ __forceinline__ void load_points32(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                                              const double* __restrict__ y2, int N, int n0, float (&fx)[PPL], float (&fy)[PPL],
                                              float (&gx)[PPL], float (&gy)[PPL], Each&& each)
{
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const int n = n0 + q;
        const bool ok = n < N;
        const double px = ok ? x1[n] : 1.0, py = ok ? y1[n] : 1.0, qx = ok ? x2[n] : 1.0, qy = ok ? y2[n] : 1.0;
        each(q, ok, px, py, qx, qy);
        fx[q] = (float)px; fy[q] = (float)py; gx[q] = (float)qx; gy[q] = (float)qy;
    }
}

// ... with what the full bound needs per point: cx = u max(|x2|, |y2|) (rounded up) and okm, the wave's mask of the lanes
// whose point q takes part (in range, and set in `mask` when MASK).  Only the FP32 copies stay in registers; the rare FP64
// decision reloads its point (L2-resident).
template <int PPL, bool MASK>
__device__ __forceinline__ void load_tile32(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                                            const double* __restrict__ y2, int N, int n0, const unsigned char* __restrict__ mask,
                                            float (&fx)[PPL], float (&fy)[PPL], float (&gx)[PPL], float (&gy)[PPL], float (&cx)[PPL],
                                            unsigned long long (&okm)[PPL])
{
    load_points32<PPL>(x1, y1, x2, y2, N, n0, fx, fy, gx, gy, [&](int q, bool ok, double, double, double, double) {
        if (MASK && ok) ok = mask[n0 + q] != 0;
        okm[q] = __builtin_amdgcn_ballot_w64(ok);
    });
#pragma unroll
    for (int q = 0; q < PPL; ++q) cx[q] = U32 * fmaxf(fabsf(gx[q]), fabsf(gy[q])) * 1.0000002f;
}

// Pass one, the cheap test: the wave's mask of the lanes whose pair is PROVABLY far (d2 >= 1.028 (vk1 / 1.12)^2; the cost
// kernels' near pairs are the complement).  Nothing but the mask survives it, so it needs few registers.
__device__ __forceinline__ unsigned long long cheap_far(const Model32& m, float fx, float fy, float gx, float gy, float vk1)
{
    const float s = __builtin_fmaf(m.h6, fx, __builtin_fmaf(m.h7, fy, m.h8));
    const float nx = __builtin_fmaf(m.h0, fx, __builtin_fmaf(m.h1, fy, m.h2));
    const float ny = __builtin_fmaf(m.h3, fx, __builtin_fmaf(m.h4, fy, m.h5));
    const float wx = __builtin_fmaf(gx, s, -nx), wy = __builtin_fmaf(gy, s, -ny);      // s dx, s dy
    const float W = fmaxf(fabsf(wx), fabsf(wy));
    return __builtin_amdgcn_ballot_w64(fabsf(s) >= m.tau) & __builtin_amdgcn_ballot_w64(W >= fmaxf(vk1 * fabsf(s), m.a25));
}

// Pass two, the full bound, for the pairs in which some lane is not provably far (the few FP32 operations of pass one are
// simply done again; this is the rare path): t = d2_fp32 - thr^2 and the lane masks straight from the compares — `trust`
// (sigma >= tau) and `clear` (|t| > B0; false for NaN).  A pair is decided in FP32 where both are set, by the sign of t.
struct Bound32 {
    unsigned long long trust, clear;
    float t;
};

__device__ __forceinline__ Bound32 full_bound(const Model32& m, float fx, float fy, float gx, float gy, float cx, float vthr2, float vc_thr)
{
    const float s = __builtin_fmaf(m.h6, fx, __builtin_fmaf(m.h7, fy, m.h8));
    const float nx = __builtin_fmaf(m.h0, fx, __builtin_fmaf(m.h1, fy, m.h2));
    const float ny = __builtin_fmaf(m.h3, fx, __builtin_fmaf(m.h4, fy, m.h5));
    const float r = __builtin_amdgcn_rcpf(s);
    const float uu = nx * r, vv = ny * r;
    const float dx = gx - uu, dy = gy - vv;
    const float w = fmaxf(fabsf(dx), fabsf(dy));
    const float d2 = __builtin_fmaf(dx, dx, dy * dy);
    // the bound (every term >= 0); B0 = everything but the 2.2u d2 term, which the constant c_thr absorbs: a pair
    // decided as inlier has d2 < thr^2, and "d2 - B0 >= thr^2 (1 + 3u)" implies "d2 (1 - 2.2u) - B0 >= thr^2"
    const float mm = fmaxf(fabsf(uu), fabsf(vv));
    const float eq = __builtin_fmaf(__builtin_fmaf(mm, m.es, m.en), fabsf(r), (5.0f * U32) * mm);
    const float E = __builtin_fmaf(1.01f * U32, w, eq + cx);
    const float B0 = __builtin_fmaf(2.02f * E, __builtin_fmaf(2.0f, w, E), vc_thr);
    const float t = d2 - vthr2;
    return { __builtin_amdgcn_ballot_w64(fabsf(s) >= m.tau), __builtin_amdgcn_ballot_w64(fabsf(t) > B0), t };
}

// The per-(model, slice) finish.  s_sum[k][wave][t]: wave's k-th sum for model m0 + t.  After a barrier, one plain store
// (a single slice) or one integer atomicAdd per model and sum into out[k].
template <int MC, int WAVES, int NS>
__device__ __forceinline__ void sums_to_global(int (&s_sum)[NS][WAVES][MC], int m0, int M, int psplit, int* const (&out)[NS])
{
    __syncthreads();
    if (threadIdx.x < MC && m0 + (int)threadIdx.x < M) {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) c += s_sum[k][w][t];
            if (psplit == 1) out[k][m0 + t] = c;
            else atomicAdd(&out[k][m0 + t], c);
        }
    }
}

// ... from the lane accumulators: lane t of each of the WAVES waves holds model m0 + t's NS sums (lane_acc_add)
template <int MC, int WAVES, int NS>
__device__ __forceinline__ void finish32(const int (&acc)[NS], int wave, int m0, int M, int psplit, int* const (&out)[NS])
{
    static_assert(MC <= 64, "lane mi of a wave accumulates model m0 + mi");
    const int lane = threadIdx.x & 63;
    __shared__ int s_sum[NS][WAVES][MC];
    if (lane < MC) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s_sum[k][wave][lane] = acc[k];
    }
    sums_to_global<MC, WAVES, NS>(s_sum, m0, M, psplit, out);
}

// A resident grid: as many workgroups as the chip holds hand themselves the gx x psplit work items (model block bx, point
// slice by) through the counter ctl[0] (as k_residual_resident, residual.hip); the last workgroup out (ctl[1]) leaves both
// words zero for the next launch.  slice_major: consecutive items are the point slices of one model block — the workgroups
// at work write a compact window of the output (tools/ubench/store_order.hip: a store stream alone gains 9 % from that order).
template <typename WG>
__device__ __forceinline__ void resident_items(int* __restrict__ ctl, int gx, int psplit, int nitems, int slice_major, WG&& wg)
{
    __shared__ int s_item;
#pragma unroll 1
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&ctl[0], 1);
        __syncthreads();
        const int item = s_item;
        if (item >= nitems) break;
        int bx, by;
        if (slice_major) { bx = item / psplit; by = item - bx * psplit; }
        else { by = item / gx; bx = item - by * gx; }
        wg(bx, by);
        __syncthreads();
    }
    if (threadIdx.x == 0 && atomicAdd(&ctl[1], 1) == (int)gridDim.x - 1) {
        ctl[1] = 0;
        __hip_atomic_store(&ctl[0], 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host side: the launch rules ------------------------------------------------------------------------------------

// The per-launch constants.  thr2_f: the threshold in FP32.  c_thr, the constant part of the bound: the rounding of the
// threshold itself (one ulp covers it either way) plus the 2.2u d2 term for d2 up to thr^2 (1 + 3u) (full_bound).  k1 of the
// cheap test = max(1.12 far_factor thr, 25.4 u Cmax), rounded up (the product k1 sigma is rounded once more in the kernel):
// far_factor 1 proves d2 >= 1.028 thr^2 (score, MSAC), 9/4 proves d2 >= 1.028 T beyond the cost matrix's truncation
// threshold T = (9/4 thr)^2.
struct Pretest32Launch {
    float thr2_f, c_thr, k1;
    Pretest32Launch(double thr2, double Cmax, double far_factor)
        : thr2_f((float)thr2),
          c_thr((float)(std::fabs((double)thr2_f - thr2) * 1.01 + 3.5 * (double)U32 * std::fabs(thr2) * 1.01) + 1e-45f),
          k1((float)(std::fmax(1.12 * far_factor * std::sqrt(std::fabs(thr2)), 25.4 * (double)U32 * Cmax) * (1.0 + 1e-6)) + 1e-30f)
    {
    }
};

inline int clamp_slices(int ps, int ntiles)
{
    if (ps > ntiles) ps = ntiles;
    return ps < 1 ? 1 : ps;
}

// Point slices of a launch over gx model blocks and ntiles point tiles: `chosen` (a resident grid's) if positive, else enough
// for ~2 048 workgroups, or `few` slices from `many_tiles` tiles on when the model blocks alone fill the chip; never more
// than tiles.  With more than one slice the kernels add into the sums (sums_to_global), which are cleared here.
inline hipError_t point_slices(int gx, int ntiles, int many_tiles, int few, int chosen, int M, int* sums, int* sums2, hipStream_t s, int* psplit)
{
    *psplit = clamp_slices(chosen > 0 ? chosen : gx < 1024 ? (2048 + gx - 1) / gx : (ntiles >= many_tiles ? few : 1), ntiles);
    for (int* a : { sums, sums2 })
        if (a && *psplit > 1) {
            hipError_t e = hipMemsetAsync(a, 0, sizeof(int) * (size_t)M, s);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// Should this launch run as a resident grid, and with how many point slices?  Returns the grid (workgroups; 0 = hardware
// dispatch) and sets *slices: `choice` if positive, else ~37 500 items.  Resident only when the items outnumber the
// workgroups the chip holds.  occ_cache: the kernel's workgroups per compute unit, asked once per ENGINE (the caller's cache,
// -1 = not asked yet; a function-local static would be shared by every engine, device and host thread — r04 advisor
// finding), and a failed query is not kept.
inline int resident_grid(const void* kernel, int threads, int* occ_cache, int cu_count, int choice, int gx, int ntiles, int* slices)
{
    int per_cu = occ_cache ? *occ_cache : -1;
    if (per_cu < 0) {
        int q = 0;
        per_cu = hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kernel, threads, 0) == hipSuccess ? q : 0;
        if (per_cu > 0 && occ_cache) *occ_cache = per_cu;
    }
    *slices = clamp_slices(choice > 0 ? choice : (37500 + gx - 1) / gx, ntiles);
    const int grid = per_cu * cu_count;
    return grid > 0 && gx * *slices > grid ? grid : 0;
}

} // namespace mh
