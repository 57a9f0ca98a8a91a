// msac32.hip — MSAC-weighted hypothesis scores, gfx950: per model the inlier count of score32.hip AND the sum of the
// inliers' integer gains (include/multih_hip.h, mh_score_msac):
//     d2 < thr2 (strictly)  ->  counts 1, weighs (int)round(256.0 * (1.0 - (d2 / thr2)))  = data_term<false>(d2, thr2, 256.0, 0)
//     otherwise (inf, NaN)  ->  counts 0, weighs 0
// Both sums are int32, so they are exact and do not depend on the order of summation.
//
// k_msac32 is score32_wg's work split (a 256-thread workgroup owns MC models and sweeps a slice of the points, a lane holds
// PPL points), its k_model32 table and its pass-one cheap test: a pair proven far has d2 >= 1.028 thr2 and is 0 / 0 without
// a quotient.  In pass two a pair that the full FP32 bound decides as "not an inlier" is 0 / 0 as well; every other pair —
// decided inlier, or too close to call — needs d2 itself and takes the FP64 formula in the reference's operation order
// (fwd_d2), then `d2 < thr2` and the gain.  So the FP64 share is the inlier share plus score32's undecided pairs.
// Counts go ballot -> popcount -> the lane-mi accumulator as in score32_wg; the gains of a (model, tile) are summed over the
// wave by six __shfl_xor steps, only under the wave-uniform branch "some lane had an inlier", into a second accumulator of
// the same kind.  One integer atomicAdd per (model, slice) ends it (a plain store with one slice).
//
// k_msac64 is the plain FP64 form for inputs the pre-test is not proved for (score_models' preconditions, capi_score.hip):
// every pair through fwd_d2, the same reductions.
#include "../../include/multih_hip.h"
#include "mh_kernels.hpp"
#include "mh_device.hpp"

#include <cmath>

namespace mh {

namespace {

constexpr float MSAC_U32 = 5.9604644775390625e-08f;       // 2^-24

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// acc's lane mi += add (add and mi wave-uniform)
__device__ __forceinline__ void lane_add(int& acc, int mi, int add)
{
    const int v = __builtin_amdgcn_readlane(acc, mi) + add;
    asm("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %1, m0" : "+v"(acc) : "s"(v), "s"(mi) : "m0");
}

// lane t of each of the four waves holds model m0 + t's sums: one store or atomicAdd per (model, slice)
template <int MC>
__device__ __forceinline__ void msac_finish(int cnt, int wgt, int m0, int M, int psplit, int* __restrict__ counts, int* __restrict__ weights)
{
    static_assert(MC <= 64, "lane mi of a wave accumulates model m0 + mi");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s_cnt[4][MC], s_wgt[4][MC];
    if (lane < MC) { s_cnt[wave][lane] = cnt; s_wgt[wave][lane] = wgt; }
    __syncthreads();
    if (threadIdx.x < MC && m0 + (int)threadIdx.x < M) {
        const int t = threadIdx.x;
        const int c = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
        const int w = s_wgt[0][t] + s_wgt[1][t] + s_wgt[2][t] + s_wgt[3][t];
        if (psplit == 1) { counts[m0 + t] = c; weights[m0 + t] = w; }
        else { atomicAdd(&counts[m0 + t], c); atomicAdd(&weights[m0 + t], w); }
    }
}

} // namespace

// (registers capped for six waves per SIMD, the cap k_score32<4, 64, *, 6> runs under: 78 VGPRs, no scratch; uncapped 84 and five waves)
template <int PPL, int MC, bool MASK>
__global__ void __launch_bounds__(256, 6)
k_msac32(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
         const double* __restrict__ y2, int N, const double* __restrict__ H, const float* __restrict__ H32, int M,
         double thr2, float thr2_f, float c_thr, float k1, int* __restrict__ counts, int* __restrict__ weights,
         const unsigned char* __restrict__ mask, int psplit, unsigned long long* __restrict__ fp64_pairs)
{
    constexpr int WAVE_PTS = 64 * PPL, TILE = 4 * WAVE_PTS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = blockIdx.x * MC;
    __shared__ float4 s_m[MC * 4];               // this workgroup's rows of the model table (k_model32)
    for (int i = threadIdx.x; i < MC * 4; i += 256) {
        const size_t g = (size_t)m0 * 4 + i;
        s_m[i] = g < (size_t)M * 4 ? reinterpret_cast<const float4*>(H32)[g] : make_float4(0.f, 0.f, 0.f, NAN);
    }
    __syncthreads();
    float vthr2, vc_thr, vk1;                    // kernel-argument constants that enter FP32 instructions: VGPR copies
    asm volatile("v_mov_b32 %0, %1" : "=v"(vthr2) : "s"(thr2_f));
    asm volatile("v_mov_b32 %0, %1" : "=v"(vc_thr) : "s"(c_thr));
    asm volatile("v_mov_b32 %0, %1" : "=v"(vk1) : "s"(k1));
    int cnt = 0, wgt = 0;                        // lane mi of each wave holds model m0 + mi's count and weight
    unsigned long long fb = 0;                   // pairs this lane sent through the FP64 formula
    for (int base = blockIdx.y * TILE; base < N; base += psplit * TILE) {
        const int n0 = base + wave * WAVE_PTS + lane * PPL;
        float fx[PPL], fy[PPL], gx[PPL], gy[PPL], cx[PPL];
        unsigned long long okm[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int n = n0 + q;
            bool ok = n < N;
            const double px = ok ? x1[n] : 1.0, py = ok ? y1[n] : 1.0, qx = ok ? x2[n] : 1.0, qy = ok ? y2[n] : 1.0;
            if (MASK && ok) ok = mask[n] != 0;
            okm[q] = __builtin_amdgcn_ballot_w64(ok);
            fx[q] = (float)px; fy[q] = (float)py; gx[q] = (float)qx; gy[q] = (float)qy;
            cx[q] = MSAC_U32 * fmaxf(fabsf(gx[q]), fabsf(gy[q])) * 1.0000002f;
        }
#pragma unroll 1
        for (int mi = 0; mi < MC; ++mi) {
            const int m = m0 + mi;
            if (m >= M) break;
            const float4 ma = s_m[4 * mi], mb = s_m[4 * mi + 1], mc = s_m[4 * mi + 2], md = s_m[4 * mi + 3];
            const float h0 = ma.x, h1 = ma.y, h2 = ma.z, h3 = ma.w, h4 = mb.x, h5 = mb.y, h6 = mb.z, h7 = mb.w, h8 = mc.x;
            const float es = mc.y, en = mc.z, tau = mc.w, a25 = md.x;
            // pass one: score32_wg's cheap test (the bound's derivation is at the head of score32.hip)
            unsigned long long farq[PPL], all_far = ~0ull;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const float s = __builtin_fmaf(h6, fx[q], __builtin_fmaf(h7, fy[q], h8));
                const float nx = __builtin_fmaf(h0, fx[q], __builtin_fmaf(h1, fy[q], h2));
                const float ny = __builtin_fmaf(h3, fx[q], __builtin_fmaf(h4, fy[q], h5));
                const float wx = __builtin_fmaf(gx[q], s, -nx), wy = __builtin_fmaf(gy[q], s, -ny);
                const float W = fmaxf(fabsf(wx), fabsf(wy));
                farq[q] = __builtin_amdgcn_ballot_w64(fabsf(s) >= tau) &
                          __builtin_amdgcn_ballot_w64(W >= fmaxf(vk1 * fabsf(s), a25));
                all_far &= farq[q];
            }
            if (all_far == ~0ull) continue;
            int c_m = 0, w_lane = 0;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                if (farq[q] == ~0ull) continue;
                asm volatile("; msac32: full bound");            // (keeps the two passes' arithmetic apart)
                const float s = __builtin_fmaf(h6, fx[q], __builtin_fmaf(h7, fy[q], h8));
                const float nx = __builtin_fmaf(h0, fx[q], __builtin_fmaf(h1, fy[q], h2));
                const float ny = __builtin_fmaf(h3, fx[q], __builtin_fmaf(h4, fy[q], h5));
                const float r = __builtin_amdgcn_rcpf(s);
                const float uu = nx * r, vv = ny * r;
                const float dx = gx[q] - uu, dy = gy[q] - vv;
                const float w = fmaxf(fabsf(dx), fabsf(dy));
                const float d2 = __builtin_fmaf(dx, dx, dy * dy);
                const float mm = fmaxf(fabsf(uu), fabsf(vv));
                const float eq = __builtin_fmaf(__builtin_fmaf(mm, es, en), fabsf(r), (5.0f * MSAC_U32) * mm);
                const float E = __builtin_fmaf(1.01f * MSAC_U32, w, eq + cx[q]);
                const float B0 = __builtin_fmaf(2.02f * E, __builtin_fmaf(2.0f, w, E), vc_thr);
                const float t = d2 - vthr2;
                const unsigned long long trust = __builtin_amdgcn_ballot_w64(fabsf(s) >= tau);
                const unsigned long long clear = __builtin_amdgcn_ballot_w64(fabsf(t) > B0);       // (false for NaN)
                const unsigned long long above = __builtin_amdgcn_ballot_w64(t >= 0.0f);
                // decided "not an inlier": 0 / 0.  Every other pair of a point that takes part needs d2 itself.
                const unsigned long long out = (trust & clear & above) | farq[q];
                const unsigned long long cand = ~out & okm[q];
                if (cand == 0ull) continue;
                bool in64 = false;
                if ((cand >> lane) & 1ull) {
                    const double* h = H + 9 * (size_t)m;
                    const int n = n0 + q;                            // (n < N: okm holds only real points)
                    const double e2 = fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x1[n], y1[n], x2[n], y2[n]);
                    in64 = e2 < thr2;
                    w_lane += data_term<false>(e2, thr2, (double)MH_MSAC_SCALE, 0);      // 0 unless e2 < thr2
                    ++fb;
                }
                c_m += __builtin_popcountll(__builtin_amdgcn_ballot_w64(in64));
            }
            if (c_m > 0) {                                           // wave-uniform: some lane had an inlier
                lane_add(cnt, mi, c_m);
                lane_add(wgt, mi, __builtin_amdgcn_readfirstlane(wave_sum(w_lane)));
            }
        }
    }
    msac_finish<MC>(cnt, wgt, m0, M, psplit, counts, weights);
    if (fp64_pairs) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) fb += __shfl_xor(fb, o, 64);
        if (lane == 0 && fb) atomicAdd(fp64_pairs, fb);
    }
}

// The plain form: a wave takes 64 points at a time, one per lane, against the workgroup's 64 models (FP64 coefficients in LDS).
template <bool MASK>
__global__ void __launch_bounds__(256)
k_msac64(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
         const double* __restrict__ y2, int N, const double* __restrict__ H, int M, double thr2, int* __restrict__ counts,
         int* __restrict__ weights, const unsigned char* __restrict__ mask, int psplit)
{
    constexpr int MC = 64, TILE = 256;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = blockIdx.x * MC;
    __shared__ double s_h[MC * 9];
    for (int i = threadIdx.x; i < MC * 9; i += 256) {
        const size_t g = (size_t)m0 * 9 + i;
        s_h[i] = g < (size_t)M * 9 ? H[g] : 0.0;
    }
    __syncthreads();
    int cnt = 0, wgt = 0;
    for (int base = blockIdx.y * TILE; base < N; base += psplit * TILE) {
        const int n = base + wave * 64 + lane;
        bool ok = n < N;
        const double px = ok ? x1[n] : 1.0, py = ok ? y1[n] : 1.0, qx = ok ? x2[n] : 1.0, qy = ok ? y2[n] : 1.0;
        if (MASK && ok) ok = mask[n] != 0;
        if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;
#pragma unroll 1
        for (int mi = 0; mi < MC; ++mi) {
            if (m0 + mi >= M) break;
            const double* h = s_h + 9 * mi;
            const double d2 = fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], px, py, qx, qy);
            const bool in = ok && d2 < thr2;
            const unsigned long long inl = __builtin_amdgcn_ballot_w64(in);
            if (inl == 0ull) continue;
            const int w = in ? data_term<false>(d2, thr2, (double)MH_MSAC_SCALE, 0) : 0;
            lane_add(cnt, mi, __builtin_popcountll(inl));
            lane_add(wgt, mi, __builtin_amdgcn_readfirstlane(wave_sum(w)));
        }
    }
    msac_finish<MC>(cnt, wgt, m0, M, psplit, counts, weights);
}

static hipError_t msac_clear(int* counts, int* weights, int M, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * (size_t)M, s);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(weights, 0, sizeof(int) * (size_t)M, s);
}

// H32: the table launch_model32 made for these M models with the same Cmax.  thr2 in [2^-40, 2^40], coordinates below 2^20.
// Hardware dispatch only (launch_score32_t's rule for the point slices).
hipError_t launch_msac32(const Points& p, const double* H, const float* H32, int M, double thr2, double Cmax, const unsigned char* mask,
                         int* counts, int* weights, unsigned long long* fp64_pairs, hipStream_t s)
{
    if (M <= 0 || p.n <= 0) return hipSuccess;
    constexpr int PPL = 4, MC = 64;
    const int gx = (M + MC - 1) / MC, ntiles = (p.n + 256 * PPL - 1) / (256 * PPL);
    int psplit = gx < 1024 ? (2048 + gx - 1) / gx : (ntiles >= 16 ? 4 : 1);
    if (psplit > ntiles) psplit = ntiles;
    if (psplit < 1) psplit = 1;
    if (psplit > 1) {
        hipError_t e = msac_clear(counts, weights, M, s);
        if (e != hipSuccess) return e;
    }
    // the threshold in FP32, the constant part of the bound and the cheap test's k1: launch_score32_t's, to the letter
    const float tf = (float)thr2;
    const float c_thr = (float)(std::fabs((double)tf - thr2) * 1.01 + 3.5 * 5.9604644775390625e-08 * std::fabs(thr2) * 1.01) + 1e-45f;
    const float k1 = (float)(std::fmax(1.12 * std::sqrt(std::fabs(thr2)), 25.4 * 5.9604644775390625e-08 * Cmax) * (1.0 + 1e-6)) + 1e-30f;
    if (mask) hipLaunchKernelGGL((k_msac32<PPL, MC, true>), dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, thr2, tf, c_thr, k1, counts, weights, mask, psplit, fp64_pairs);
    else hipLaunchKernelGGL((k_msac32<PPL, MC, false>), dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, thr2, tf, c_thr, k1, counts, weights, mask, psplit, fp64_pairs);
    return hipGetLastError();
}

hipError_t launch_msac64(const Points& p, const double* H, int M, double thr2, const unsigned char* mask, int* counts, int* weights,
                         hipStream_t s)
{
    if (M <= 0 || p.n <= 0) return hipSuccess;
    const int gx = (M + 63) / 64, ntiles = (p.n + 255) / 256;
    int psplit = gx < 1024 ? (2048 + gx - 1) / gx : (ntiles >= 64 ? 4 : 1);
    if (psplit > ntiles) psplit = ntiles;
    if (psplit < 1) psplit = 1;
    if (psplit > 1) {
        hipError_t e = msac_clear(counts, weights, M, s);
        if (e != hipSuccess) return e;
    }
    if (mask) hipLaunchKernelGGL(k_msac64<true>, dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, M, thr2, counts, weights, mask, psplit);
    else hipLaunchKernelGGL(k_msac64<false>, dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, M, thr2, counts, weights, mask, psplit);
    return hipGetLastError();
}

} // namespace mh
