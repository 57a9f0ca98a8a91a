// msac32.hip — MSAC-weighted hypothesis scores, gfx950: per model the inlier count of score32.hip AND the sum of the
// inliers' integer gains (include/multih_hip.h, mh_score_msac):
//     d2 < thr2 (strictly)  ->  counts 1, weighs (int)round(256.0 * (1.0 - (d2 / thr2)))  = data_term<false>(d2, thr2, 256.0, 0)
//     otherwise (inf, NaN)  ->  counts 0, weighs 0
// Both sums are int32, so they are exact and do not depend on the order of summation.
//
// k_msac32 runs behind the FP32 pre-test (pretest32.hpp) with score32_wg's work split: a pair proven far by pass one has
// d2 >= 1.028 thr2 and is 0 / 0 without a quotient.  In pass two a pair that the full FP32 bound decides as "not an inlier"
// is 0 / 0 as well; every other pair — decided inlier, or too close to call — needs d2 itself and takes the FP64 formula in
// the reference's operation order (fwd_d2), then `d2 < thr2` and the gain.  So the FP64 share is the inlier share plus
// score32's undecided pairs.  The gains of a (model, tile) are summed over the wave by six __shfl_xor steps, only under the
// wave-uniform branch "some lane had an inlier", into a second lane accumulator beside the count's.
//
// k_msac64 is the plain FP64 form for inputs the pre-test is not proved for (pretest_usable, capi_score.hip):
// every pair through fwd_d2, the same reductions.
#include "../../include/multih_hip.h"
#include "pretest32.hpp"

namespace mh {

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
    stage_model32<MC, 256>(s_m, H32, m0, M);
    __syncthreads();
    const float vthr2 = vgpr_copy(thr2_f), vc_thr = vgpr_copy(c_thr), vk1 = vgpr_copy(k1);
    int cnt = 0, wgt = 0;                        // lane mi of each wave holds model m0 + mi's count and weight
    unsigned long long fb = 0;                   // pairs this lane sent through the FP64 formula
    for (int base = blockIdx.y * TILE; base < N; base += psplit * TILE) {
        const int n0 = base + wave * WAVE_PTS + lane * PPL;
        float fx[PPL], fy[PPL], gx[PPL], gy[PPL], cx[PPL];
        unsigned long long okm[PPL];
        load_tile32<PPL, MASK>(x1, y1, x2, y2, N, n0, mask, fx, fy, gx, gy, cx, okm);
#pragma unroll 1
        for (int mi = 0; mi < MC; ++mi) {
            const int m = m0 + mi;
            if (m >= M) break;
            const Model32 mod = model32_from_lds(s_m, mi);
            unsigned long long farq[PPL], all_far = ~0ull;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                farq[q] = cheap_far(mod, fx[q], fy[q], gx[q], gy[q], vk1);
                all_far &= farq[q];
            }
            if (all_far == ~0ull) continue;
            int c_m = 0, w_lane = 0;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                if (farq[q] == ~0ull) continue;
                asm volatile("; msac32: full bound");            // (keeps the two passes' arithmetic apart)
                const Bound32 b = full_bound(mod, fx[q], fy[q], gx[q], gy[q], cx[q], vthr2, vc_thr);
                const unsigned long long above = __builtin_amdgcn_ballot_w64(b.t >= 0.0f);
                // decided "not an inlier": 0 / 0.  Every other pair of a point that takes part needs d2 itself.
                const unsigned long long out = (b.trust & b.clear & above) | farq[q];
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
                cnt = lane_acc_add(cnt, mi, c_m);
                wgt = lane_acc_add(wgt, mi, __builtin_amdgcn_readfirstlane(wave_sum(w_lane)));
            }
        }
    }
    finish32<MC, 4, 2>({ cnt, wgt }, threadIdx.x >> 6, m0, M, psplit, { counts, weights });
    add_fp64_pairs(fp64_pairs, fb);
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
    stage_model64<MC, 256>(s_h, H, m0, M);
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
            cnt = lane_acc_add(cnt, mi, __builtin_popcountll(inl));
            wgt = lane_acc_add(wgt, mi, __builtin_amdgcn_readfirstlane(wave_sum(w)));
        }
    }
    finish32<MC, 4, 2>({ cnt, wgt }, threadIdx.x >> 6, m0, M, psplit, { counts, weights });
}

// H32: the table launch_model32 made for these M models with the same Cmax.  thr2 in [2^-40, 2^40], coordinates below 2^20.
// Hardware dispatch only.
hipError_t launch_msac32(const Points& p, const double* H, const float* H32, int M, double thr2, double Cmax, const unsigned char* mask,
                         int* counts, int* weights, unsigned long long* fp64_pairs, hipStream_t s)
{
    if (M <= 0 || p.n <= 0) return hipSuccess;
    constexpr int PPL = 4, MC = 64;
    const int gx = (M + MC - 1) / MC, ntiles = (p.n + 256 * PPL - 1) / (256 * PPL);
    int psplit = 0;
    hipError_t e = point_slices(gx, ntiles, 16, 4, 0, M, counts, weights, s, &psplit);
    if (e != hipSuccess) return e;
    const Pretest32Launch c(thr2, Cmax, 1.0);
    if (mask) hipLaunchKernelGGL((k_msac32<PPL, MC, true>), dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, thr2, c.thr2_f, c.c_thr, c.k1, counts, weights, mask, psplit, fp64_pairs);
    else hipLaunchKernelGGL((k_msac32<PPL, MC, false>), dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, thr2, c.thr2_f, c.c_thr, c.k1, counts, weights, mask, psplit, fp64_pairs);
    return hipGetLastError();
}

hipError_t launch_msac64(const Points& p, const double* H, int M, double thr2, const unsigned char* mask, int* counts, int* weights,
                         hipStream_t s)
{
    if (M <= 0 || p.n <= 0) return hipSuccess;
    const int gx = (M + 63) / 64, ntiles = (p.n + 255) / 256;
    int psplit = 0;
    hipError_t e = point_slices(gx, ntiles, 64, 4, 0, M, counts, weights, s, &psplit);
    if (e != hipSuccess) return e;
    if (mask) hipLaunchKernelGGL(k_msac64<true>, dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, M, thr2, counts, weights, mask, psplit);
    else hipLaunchKernelGGL(k_msac64<false>, dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, M, thr2, counts, weights, mask, psplit);
    return hipGetLastError();
}

} // namespace mh
