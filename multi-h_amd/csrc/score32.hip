// score32.hip — inlier scoring and the int32 data-cost matrix behind the FP32 pre-test, gfx950 (the test, its bound and
// its derivation: pretest32.hpp).  Counts are the reference's, bit for bit.
#include "pretest32.hpp"

namespace mh {

// per model: 9 coefficients in FP32, then 1.1 E_s, 1.1 E_n, tau = 64 E_s (or NaN: not eligible), 25.2 A (the cheap test), 3 pad
__global__ void __launch_bounds__(256)
k_model32(const double* __restrict__ H, int M, double X, double Y, double Cmax, float* __restrict__ out)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const double* h = H + 9 * (size_t)m;
    float* o = out + 16 * (size_t)m;
    bool ok = true;
    for (int q = 0; q < 9; ++q) {
        ok = ok && fabs(h[q]) < 0x1p100;              // (false for NaN / inf)
        o[q] = (float)h[q];
    }
    const double u = 0x1p-24;
    const double as = fabs(h[6]) * X + fabs(h[7]) * Y + fabs(h[8]);
    const double an = fmax(fabs(h[0]) * X + fabs(h[1]) * Y + fabs(h[2]), fabs(h[3]) * X + fabs(h[4]) * Y + fabs(h[5]));
    const double es = 5.0 * u * as, en = 5.0 * u * an;
    ok = ok && es >= 0x1p-80 && en >= 0x1p-80 && as < 0x1p100 && an < 0x1p100;     // (as, an bound every product formed from this model)
    const double up = 1.0 + 0x1p-22;                  // round the bounds UP on their way to FP32
    o[9] = (float)(1.1 * es * up);
    o[10] = (float)(1.1 * en * up);
    o[11] = ok ? (float)(64.0 * es * up) : NAN;        // NaN, not +inf: an overflowed |s| = inf must not pass "|s| >= tau"
    o[12] = (float)(25.2 * 1.01 * (Cmax * es + en) * up);      // 25.2 A (25 = 1 / 0.04, the rest covers the test's own rounding)
    o[13] = o[14] = o[15] = 0.f;
}

// score32_wg: the work of ONE workgroup — model block bx (MC models), point slice by.
template <int PPL, int MC, bool MASK>
__device__ __forceinline__ void
score32_wg(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
           const double* __restrict__ y2, int N, const double* __restrict__ H, const float* __restrict__ H32, int M,
           double thr2, float thr2_f, float c_thr, float k1, int* __restrict__ counts, const unsigned char* __restrict__ mask,
           int psplit, unsigned long long* __restrict__ fallback_pairs, const int bx, const int by)
{
    constexpr int WAVE_PTS = 64 * PPL, TILE = 4 * WAVE_PTS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = bx * MC;
    __shared__ float4 s_m[MC * 4];               // this workgroup's rows of the model table
    stage_model32<MC, 256>(s_m, H32, m0, M);
    __syncthreads();
    const float vthr2 = vgpr_copy(thr2_f), vc_thr = vgpr_copy(c_thr), vk1 = vgpr_copy(k1);
    int cnt = 0;                                 // lane mi of each wave counts model m0 + mi
    unsigned long long fb = 0;                   // pairs this lane sent to FP64 (diagnostic)
    for (int base = by * TILE; base < N; base += psplit * TILE) {
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
            int c_m = 0;
            if (all_far != ~0ull) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    if (farq[q] == ~0ull) continue;
                    asm volatile("; score32: full bound");           // (keeps the two passes' arithmetic apart)
                    const Bound32 b = full_bound(mod, fx[q], fy[q], gx[q], gy[q], cx[q], vthr2, vc_thr);
                    const unsigned long long below = __builtin_amdgcn_ballot_w64(b.t < 0.0f);
                    const unsigned long long decided = (b.trust & b.clear) | farq[q];      // (the logic on the lane masks is scalar)
                    unsigned long long inl = b.trust & b.clear & below;
                    if (decided != ~0ull) {                               // rarer still: some lane's pair is too close to call
                        const bool need = ((decided >> lane) & 1ull) == 0ull;
                        bool in64 = false;
                        if (need) {
                            const double* h = H + 9 * (size_t)m;
                            const int n = n0 + q < N ? n0 + q : N - 1;      // (a padding lane: its result is masked out by okm)
                            const double e2 = fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x1[n], y1[n], x2[n], y2[n]);
                            in64 = e2 < thr2;
                            ++fb;
                        }
                        inl |= __builtin_amdgcn_ballot_w64(in64);
                    }
                    c_m += __builtin_popcountll(inl & okm[q]);
                }
            }
            cnt = lane_acc_add(cnt, mi, c_m);
        }
    }
    // (finish32 written out: through the shared helper the tile loop's latch of the 64-model kernels comes out with the other
    // branch polarity, and a row of the probe then left the parent's spread — DESIGN 3.2)
    __shared__ int s_cnt[4][MC];
    if (lane < MC) s_cnt[wave][lane] = cnt;
    __syncthreads();
    if (threadIdx.x < MC && m0 + (int)threadIdx.x < M) {
        const int t = threadIdx.x;
        const int c = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
        if (psplit == 1) counts[m0 + t] = c;
        else atomicAdd(&counts[m0 + t], c);
    }
    add_fp64_pairs(fallback_pairs, fb);
}

template <int PPL, int MC, bool MASK, int MINW = 1>
__global__ void __launch_bounds__(256, MINW)
k_score32(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
          const double* __restrict__ y2, int N, const double* __restrict__ H, const float* __restrict__ H32, int M,
          double thr2, float thr2_f, float c_thr, float k1, int* __restrict__ counts, const unsigned char* __restrict__ mask,
          int psplit, unsigned long long* __restrict__ fallback_pairs)
{
    score32_wg<PPL, MC, MASK>(x1, y1, x2, y2, N, H, H32, M, thr2, thr2_f, c_thr, k1, counts, mask, psplit, fallback_pairs, blockIdx.x, blockIdx.y);
}

// The same work items walked by a resident grid that hands them out through a counter (resident_items).
template <int PPL, int MC, bool MASK, int MINW = 1>
__global__ void __launch_bounds__(256, MINW)
k_score32_resident(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                   const double* __restrict__ y2, int N, const double* __restrict__ H, const float* __restrict__ H32, int M,
                   double thr2, float thr2_f, float c_thr, float k1, int* __restrict__ counts, const unsigned char* __restrict__ mask,
                   int psplit, unsigned long long* __restrict__ fallback_pairs, int gx, int nitems, int* __restrict__ ctl)
{
    resident_items(ctl, gx, psplit, nitems, 0, [&](int bx, int by) {
        score32_wg<PPL, MC, MASK>(x1, y1, x2, y2, N, H, H32, M, thr2, thr2_f, c_thr, k1, counts, mask, psplit, fallback_pairs, bx, by);
    });
}

// ---------------------------------------------------------------------------
// k_cost32 — the materialised int32 data-cost matrix (k_cost_matrix of datacost.hip: the s = 4 variant of SURVEY 8(d))
// behind the same pre-test.  dataEnergy (M/MultiH.cpp:473-504) of a pair whose d2 is at least T = thr^2 81/16 is the
// constant 2 round(lam T), and for a random hypothesis that is nearly every pair: the cheap test (cheap_far) with
// k1 = max(1.12 x 9/4 thr, 25.4 u Cmax) (Pretest32Launch with far_factor 9/4) proves max(|dx|, |dy|) >= 1.014 x 9/4 thr, i.e.
// d2 >= 1.028 T — a 2.8 % margin beyond the truncation threshold — per LANE; the other lanes (both |dx| and |dy| within
// 1.12 x 9/4 thr, models not eligible for FP32, NaN anywhere) evaluate the reference's
// FP64 formula — fwd_d2, the IEEE division d2 / T, C round() — exactly as k_cost_matrix does.  Same matrix, same fused
// inlier counts, bit for bit.  Measured at 50k x 100k DLT hypotheses: 7.7 -> 4.2 ms (the store stream alone would take 3.6 ms:
// 3.3 % of the pairs of such a batch are near — hypotheses fitted to four matches are often nearly right for a whole
// plane — and 42 % of the wave-model iterations contain one, each costing a pass through the IEEE formula).
// ---------------------------------------------------------------------------
// Lanes of ONE wave hand data to each other through LDS below (no workgroup barrier: the other waves are not involved).
// The LDS operations of a wave complete in program order, so all that is needed is that the COMPILER keeps the writes in
// front of the cross-lane reads: a compiler-level memory barrier and a wave barrier (a scheduling fence; no instruction).
// (r03 advisor finding.  A wave-scope release / acquire fence pair was tried first: the backend emits s_waitcnt for it and
// the kernel went from 4.3 to 4.9 ms.)
__device__ __forceinline__ void wave_lds_handover()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

#define MH_COST32_ARGS                                                                                                          \
    const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2, const double* __restrict__ y2, \
    int N, const double* __restrict__ H, const float* __restrict__ H32, int M, double lam, double T, double thr2, float k1,     \
    int* __restrict__ C, long long ldc, int* __restrict__ counts, int psplit
#define MH_COST32_PASS x1, y1, x2, y2, N, H, H32, M, lam, T, thr2, k1, C, ldc, counts, psplit

// cost32_wg: the work of ONE workgroup — model block bx (MC models), point slice by.
template <int MC, int WAVES, bool RISING>
__device__ __forceinline__ void
cost32_wg(MH_COST32_ARGS, const int bx, const int by)
{
    constexpr int PPL = 4, WAVE_PTS = 64 * PPL, TILE = WAVES * WAVE_PTS, THREADS = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = bx * MC;
    __shared__ float4 s_m[MC * 4];
    __shared__ double s_h[MC * 9];               // the FP64 coefficients, for the lanes that need the reference's formula
    __shared__ double s_p[WAVES * PPL * 4 * 64];     // [wave][point of the lane][x1 y1 x2 y2][lane]: every lane's own points in FP64
    stage_model32<MC, THREADS>(s_m, H32, m0, M);
    stage_model64<MC, THREADS>(s_h, H, m0, M);
    __syncthreads();
    double* wave_p = s_p + (size_t)wave * (PPL * 4 * 64);           // + (q * 4 + component) * 64 + lane
    double* my_p = wave_p + lane;
    __shared__ unsigned char s_list[WAVES * 64 * PPL];                 // per wave: the (point slot, lane) of the pairs that need FP64
    __shared__ int s_c[WAVES * 64 * PPL];                               // per wave: their costs, on the way back to the owning lane
    unsigned char* my_list = s_list + wave * (64 * PPL);
    int* my_c = s_c + wave * (64 * PPL);
    const float vk1 = vgpr_copy(k1);
    const int beyond = 2 * (int)round(lam * T);
    int cnt = 0;                                 // lane mi of each wave counts model m0 + mi
    for (int base = by * TILE; base < N; base += psplit * TILE) {
        const int base_n = base + wave * WAVE_PTS;
        const int n0 = base_n + lane * PPL;
        float fx[PPL], fy[PPL], gx[PPL], gy[PPL];
        load_points32<PPL>(x1, y1, x2, y2, N, n0, fx, fy, gx, gy, [&](int q, bool, double px, double py, double qx, double qy) {
            my_p[(q * 4 + 0) * 64] = px; my_p[(q * 4 + 1) * 64] = py; my_p[(q * 4 + 2) * 64] = qx; my_p[(q * 4 + 3) * 64] = qy;
        });
        wave_lds_handover();                     // the FP64 copies are read by OTHER lanes of this wave below
#pragma unroll 1
        for (int mi = 0; mi < MC; ++mi) {
            const int m = m0 + mi;
            if (m >= M) break;
            const Model32 mod = model32_from_lds(s_m, mi);
            int c[PPL];
            unsigned long long nearq[PPL], any_near = 0ull;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                nearq[q] = ~cheap_far(mod, fx[q], fy[q], gx[q], gy[q], vk1);
                any_near |= nearq[q];
                c[q] = beyond;
            }
            int c_m = 0;
            if (any_near) {
                // The near pairs of the wave's 256 (typically a few dozen, spread over all four point slots) are packed into
                // a list in LDS and evaluated 64 at a time by whichever lanes come first — a lane works on other lanes'
                // points, which is why every lane's FP64 copies live in LDS — instead of one masked pass per point slot.
                asm volatile("; cost32: FP64 pairs");
                int npairs = 0;
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    if ((nearq[q] >> lane) & 1ull) {
                        const int pos = npairs + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(nearq[q] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)nearq[q], 0u));
                        my_list[pos] = (unsigned char)(q * 64 + lane);
                    }
                    npairs += __builtin_popcountll(nearq[q]);
                }
                wave_lds_handover();             // the list is read across lanes
                const double* h = s_h + 9 * mi;
                const double h0d = h[0], h1d = h[1], h2d = h[2], h3d = h[3], h4d = h[4], h5d = h[5], h6d = h[6], h7d = h[7], h8d = h[8];
                for (int p0 = 0; p0 < npairs; p0 += 64) {
                    bool in64 = false;
                    if (p0 + lane < npairs) {
                        const int id = my_list[p0 + lane], q2 = id >> 6, l2 = id & 63;
                        const double* pp = wave_p + (q2 * 4) * 64 + l2;
                        const double d2 = fwd_d2(h0d, h1d, h2d, h3d, h4d, h5d, h6d, h7d, h8d, pp[0], pp[64], pp[128], pp[192]);
                        my_c[id] = data_term<RISING>(d2, T, lam, beyond);
                        in64 = (base_n + l2 * PPL + q2 < N) && d2 < thr2;
                    }
                    c_m += __builtin_popcountll(__builtin_amdgcn_ballot_w64(in64));
                }
                wave_lds_handover();             // the costs go back to the lanes that own the pairs
#pragma unroll
                for (int q = 0; q < PPL; ++q)
                    if ((nearq[q] >> lane) & 1ull) c[q] = my_c[q * 64 + lane];
                wave_lds_handover();             // (the next model's list and costs overwrite these)
            }
            int* dst = C + (size_t)m * ldc + n0;
            if (n0 + 3 < N) {
                typedef int i4v __attribute__((ext_vector_type(4)));
                const i4v v = { c[0], c[1], c[2], c[3] };
                __builtin_nontemporal_store(v, reinterpret_cast<i4v*>(dst));
            }
            else
                for (int q = 0; q < PPL; ++q) if (n0 + q < N) dst[q] = c[q];
            if (any_near) cnt = lane_acc_add(cnt, mi, c_m);
        }
    }
    finish32<MC, WAVES, 1>({ cnt }, wave, m0, M, psplit, { counts });
}

// cost32_wg_batched (r04 EXPERIMENT, mh_set_tuning key 28 = 1; not the default): the same matrix with the near pairs of
// SEVERAL models evaluated together.  Measured at 50k x 100k: the arithmetic side gains what was expected (4.13 -> 3.56 ms
// when the near pairs' costs are computed but not delivered), the delivery loses more: 4.45 ms with plain stores of the
// constant and 5.95 ms with non-temporal ones — a 4-byte store into a line that has already left L2 is a read-modify-write
// in memory, 150 million of them per launch.  Delivering through LDS to the owning lane before ITS store (the default
// form) needs the costs of all pending models in LDS, which the 64 KB of FP64 point copies leave hardly any room for: a
// second version (up to eight models pending, their lane masks and 272 list entries in the 1 376 bytes per wave that two
// workgroups per compute unit leave, rows written once with the costs fetched by rank in the mask) ran 4.36 ms — the
// bookkeeping of the pending rows costs what the fuller passes save.  In cost32_wg every
// wave x model iteration that contains a near pair (42 % of them on a DLT batch) pays a pass through the IEEE formula with,
// typically, a few dozen of its 64 lanes at work.  Here a wave writes the constant row segment at once, appends its near
// pairs — (model, point slot, lane) — to a list in LDS, and runs the formula only when 64 entries have gathered (and once at
// the end of a tile): full lanes, one eighth of the passes.  The cost of a near pair then goes straight to C[m][n], over
// the constant written before: the wave drains its stores (s_waitcnt vmcnt(0)) before the first such store of a batch, so
// the two writes of an address arrive in order.  Inlier counts go through an LDS counter per (wave, model).
template <int MC, int WAVES, bool RISING>
__device__ __forceinline__ void
cost32_wg_batched(MH_COST32_ARGS, const int bx, const int by)
{
    constexpr int PPL = 4, WAVE_PTS = 64 * PPL, TILE = WAVES * WAVE_PTS, THREADS = 64 * WAVES, LCAP = 64 + 64 * PPL;
    static_assert(MC <= 64, "a list entry carries the model in 6 bits");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = bx * MC;
    __shared__ float4 s_m[MC * 4];
    __shared__ double s_h[MC * 9];
    __shared__ double s_p[WAVES * PPL * 4 * 64];          // [wave][point of the lane][x1 y1 x2 y2][lane]
    __shared__ unsigned short s_list[WAVES * LCAP];       // per wave: (model << 8 | point slot << 6 | lane) of the pending near pairs
    __shared__ int s_cnt[1][WAVES][MC];
    stage_model32<MC, THREADS>(s_m, H32, m0, M);
    stage_model64<MC, THREADS>(s_h, H, m0, M);
    for (int i = threadIdx.x; i < WAVES * MC; i += THREADS) (&s_cnt[0][0][0])[i] = 0;
    __syncthreads();
    double* wave_p = s_p + (size_t)wave * (PPL * 4 * 64);
    double* my_p = wave_p + lane;
    unsigned short* my_list = s_list + wave * LCAP;
    const float vk1 = vgpr_copy(k1);
    const int beyond = 2 * (int)round(lam * T);
    typedef int i4v __attribute__((ext_vector_type(4)));
    const i4v vbeyond = { beyond, beyond, beyond, beyond };
    for (int base = by * TILE; base < N; base += psplit * TILE) {
        const int base_n = base + wave * WAVE_PTS;
        const int n0 = base_n + lane * PPL;
        float fx[PPL], fy[PPL], gx[PPL], gy[PPL];
        load_points32<PPL>(x1, y1, x2, y2, N, n0, fx, fy, gx, gy, [&](int q, bool, double px, double py, double qx, double qy) {
            my_p[(q * 4 + 0) * 64] = px; my_p[(q * 4 + 1) * 64] = py; my_p[(q * 4 + 2) * 64] = qx; my_p[(q * 4 + 3) * 64] = qy;
        });
        wave_lds_handover();                     // the FP64 copies are read by OTHER lanes of this wave below
        // One pass of the IEEE formula over the list entries [first, first + 64) (those below `count`).
        auto evaluate = [&](int first, int count) {
            if (first + lane < count) {
                const int id = my_list[first + lane], mi2 = id >> 8, q2 = (id >> 6) & 3, l2 = id & 63;
                const double* h = s_h + 9 * mi2;
                const double* pp = wave_p + (q2 * 4) * 64 + l2;
                const double d2 = fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], pp[0], pp[64], pp[128], pp[192]);
                const int cost = data_term<RISING>(d2, T, lam, beyond);
                const int n = base_n + l2 * PPL + q2;
                if (n < N) {
                    C[(size_t)(m0 + mi2) * ldc + n] = cost;
                    if (d2 < thr2) atomicAdd(&s_cnt[0][wave][mi2], 1);
                }
            }
        };
        int nlist = 0;                           // wave-uniform
#pragma unroll 1
        for (int mi = 0; mi < MC; ++mi) {
            const int m = m0 + mi;
            if (m >= M) break;
            const Model32 mod = model32_from_lds(s_m, mi);
            unsigned long long nearq[PPL], any_near = 0ull;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                nearq[q] = ~cheap_far(mod, fx[q], fy[q], gx[q], gy[q], vk1);
                any_near |= nearq[q];
            }
            int* dst = C + (size_t)m * ldc + n0;
            if (n0 + 3 < N) *reinterpret_cast<i4v*>(dst) = vbeyond;      // (a plain store: the line stays in L2 for the near pairs' costs)
            else
                for (int q = 0; q < PPL; ++q) if (n0 + q < N) dst[q] = beyond;
            if (any_near) {
                asm volatile("; cost32: near pairs to the list");
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    if ((nearq[q] >> lane) & 1ull) {
                        const int pos = nlist + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(nearq[q] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)nearq[q], 0u));
                        my_list[pos] = (unsigned short)((mi << 8) | (q << 6) | lane);
                    }
                    nlist += __builtin_popcountll(nearq[q]);
                }
                if (nlist >= 64) {
                    wave_lds_handover();         // the list is read across lanes
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the constants these pairs overwrite have landed
                    do {
                        nlist -= 64;
                        evaluate(nlist, nlist + 64);
                    } while (nlist >= 64);
                    wave_lds_handover();         // (the next entries overwrite what was just read)
                }
            }
        }
        if (nlist > 0) {
            wave_lds_handover();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (int p0 = 0; p0 < nlist; p0 += 64) evaluate(p0, nlist);
        }
        wave_lds_handover();                     // (the next tile's points and list overwrite these)
    }
    sums_to_global<MC, WAVES, 1>(s_cnt, m0, M, psplit, { counts });
}

// One work item in the default form or the key-28 experiment's.  The data term (mh_set_data_term) is a template argument of
// the workgroup functions, not of k_cost32 / k_cost32_resident: the product's two kernels keep their names and their code,
// and the rising term runs in kernels of its own name below.
template <int MC, int WAVES, bool BATCH, bool RISING>
__device__ __forceinline__ void
cost32_item(MH_COST32_ARGS, const int bx, const int by)
{
    if (BATCH) cost32_wg_batched<MC, WAVES, RISING>(MH_COST32_PASS, bx, by);
    else cost32_wg<MC, WAVES, RISING>(MH_COST32_PASS, bx, by);
}

template <int MC, int WAVES, bool BATCH>
__global__ void __launch_bounds__(64 * WAVES)
k_cost32(MH_COST32_ARGS)
{
    cost32_item<MC, WAVES, BATCH, false>(MH_COST32_PASS, blockIdx.x, blockIdx.y);
}

// The same work items walked by a resident grid that hands them out through a counter (resident_items).
template <int MC, int WAVES, bool BATCH>
__global__ void __launch_bounds__(64 * WAVES)
k_cost32_resident(MH_COST32_ARGS, int gx, int nitems, int* __restrict__ ctl, int slice_major)
{
    resident_items(ctl, gx, psplit, nitems, slice_major, [&](int bx, int by) { cost32_item<MC, WAVES, BATCH, false>(MH_COST32_PASS, bx, by); });
}

// MH_DATA_TERM_RISING: the same pre-test, lists and stores around round(lam * (d2 / T)) for the near pairs.
template <int MC, int WAVES, bool BATCH>
__global__ void __launch_bounds__(64 * WAVES)
k_rising32(MH_COST32_ARGS)
{
    cost32_item<MC, WAVES, BATCH, true>(MH_COST32_PASS, blockIdx.x, blockIdx.y);
}

template <int MC, int WAVES, bool BATCH>
__global__ void __launch_bounds__(64 * WAVES)
k_rising32_resident(MH_COST32_ARGS, int gx, int nitems, int* __restrict__ ctl, int slice_major)
{
    resident_items(ctl, gx, psplit, nitems, slice_major, [&](int bx, int by) { cost32_item<MC, WAVES, BATCH, true>(MH_COST32_PASS, bx, by); });
}
#undef MH_COST32_ARGS
#undef MH_COST32_PASS

// H32: the table launch_model32 made for these models with the same Cmax.  thr2 in [2^-40, 2^40], coordinates below 2^20.
template <bool BATCH, bool RISING>
static hipError_t launch_cost32_t(const Points& p, const double* H, const float* H32, int M, double lambda, double thr2, double Cmax,
                                  int* C, long long ldc, int* counts, hipStream_t s, int* resident_ctl, int cu_count, int psplit_override, int slice_major,
                                  int* occ_cache)
{
    if (M <= 0 || p.n <= 0) return hipSuccess;
    constexpr int MC = 32;
    // 512 threads: the FP64 copies of a wave's points take 8 KB of LDS, so two such workgroups (16 waves) fill a CU's 160 KB;
    // 256-thread workgroups got 12 waves onto a CU (4.7 ms), one 1 024-thread workgroup 16 again but 4.8 ms; this: 4.2 ms
    constexpr int WAVES = 8;
    const int gx = (M + MC - 1) / MC, ntiles = (p.n + 256 * WAVES - 1) / (256 * WAVES);
    const float k1 = Pretest32Launch(thr2, Cmax, 2.25).k1;
    const auto k_plain = RISING ? k_rising32<MC, WAVES, BATCH> : k_cost32<MC, WAVES, BATCH>;
    const auto k_resident = RISING ? k_rising32_resident<MC, WAVES, BATCH> : k_cost32_resident<MC, WAVES, BATCH>;
    // resident grid: as many workgroups as the chip holds, ~37 500 items (r04 experiment: mh_set_tuning key 23)
    int psplit = 0;
    const int grid = resident_ctl ? resident_grid((const void*)k_resident, 64 * WAVES, occ_cache, cu_count, psplit_override, gx, ntiles, &psplit) : 0;
    hipError_t e = point_slices(gx, ntiles, 8, 2, grid > 0 ? psplit : 0, M, counts, nullptr, s, &psplit);
    if (e != hipSuccess) return e;
    if (grid > 0)
        hipLaunchKernelGGL(k_resident, dim3(grid), dim3(64 * WAVES), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M,
                           100.0 / lambda, thr2 * 81.0 / 16.0, thr2, k1, C, ldc, counts, psplit, gx, gx * psplit, resident_ctl, slice_major);
    else
        hipLaunchKernelGGL(k_plain, dim3(gx, psplit), dim3(64 * WAVES), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, 100.0 / lambda,
                           thr2 * 81.0 / 16.0, thr2, k1, C, ldc, counts, psplit);
    return hipGetLastError();
}

hipError_t launch_cost32(const Points& p, const double* H, const float* H32, int M, double lambda, double thr2, double Cmax,
                         int* C, long long ldc, int* counts, hipStream_t s, int* resident_ctl, int cu_count, int psplit_override, int slice_major,
                         int batched, int* occ_cache, int rising)
{
    // batched: the experiment above (mh_set_tuning key 28) instead of the default form, in which every wave x model iteration
    // with a near pair runs the IEEE formula at once and hands the costs to the owning lanes through LDS
#ifdef MH_TUNING
    // (a measured-and-rejected variant: compiled into measurement libraries only, mh_set_tuning key 28; so are the
    // slice-major item order, key 27, and the other tilings of the score kernel below, key 16)
    if (batched && rising) return launch_cost32_t<true, true>(p, H, H32, M, lambda, thr2, Cmax, C, ldc, counts, s, resident_ctl, cu_count, psplit_override, slice_major, nullptr);
    if (batched) return launch_cost32_t<true, false>(p, H, H32, M, lambda, thr2, Cmax, C, ldc, counts, s, resident_ctl, cu_count, psplit_override, slice_major, nullptr);
#else
    (void)batched;
    slice_major = 0;
#endif
    // (the rising kernels differ from the default ones in a handful of FP64 instructions and hold the same registers and LDS —
    // DESIGN 3.7 — so the engine's cached occupancy answer serves both)
    if (rising) return launch_cost32_t<false, true>(p, H, H32, M, lambda, thr2, Cmax, C, ldc, counts, s, resident_ctl, cu_count, psplit_override, slice_major, occ_cache);
    return launch_cost32_t<false, false>(p, H, H32, M, lambda, thr2, Cmax, C, ldc, counts, s, resident_ctl, cu_count, psplit_override, slice_major, occ_cache);
}

hipError_t launch_model32(const double* H, int M, double X, double Y, double Cmax, float* H32, hipStream_t s)
{
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_model32, dim3((M + 255) / 256), dim3(256), 0, s, H, M, X, Y, Cmax, H32);
    return hipGetLastError();
}

template <int PPL, int MC, int MINW = 1>
static hipError_t launch_score32_t(const Points& p, const double* H, const float* H32, int M, double thr2, double Cmax, const unsigned char* mask,
                                   int* counts, unsigned long long* fallback_pairs, hipStream_t s, int* resident_ctl = nullptr,
                                   int cu_count = 256, int resident_slices = 0, int* occ_cache = nullptr)
{
    const int gx = (M + MC - 1) / MC, ntiles = (p.n + 256 * PPL - 1) / (256 * PPL);
    int psplit = 0, resident = 0;
    if (resident_ctl && resident_slices != 0 && !mask)
        resident = resident_grid((const void*)k_score32_resident<PPL, MC, false, MINW>, 256, occ_cache, cu_count, resident_slices, gx, ntiles, &psplit);
    hipError_t e = point_slices(gx, ntiles, 16, 4, resident > 0 ? psplit : 0, M, counts, nullptr, s, &psplit);
    if (e != hipSuccess) return e;
    const Pretest32Launch c(thr2, Cmax, 1.0);
    if (resident > 0) {
        hipLaunchKernelGGL((k_score32_resident<PPL, MC, false, MINW>), dim3(resident), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, thr2, c.thr2_f,
                           c.c_thr, c.k1, counts, mask, psplit, fallback_pairs, gx, gx * psplit, resident_ctl);
        return hipGetLastError();
    }
    if (mask) hipLaunchKernelGGL((k_score32<PPL, MC, true, MINW>), dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, thr2, c.thr2_f, c.c_thr, c.k1, counts, mask, psplit, fallback_pairs);
    else hipLaunchKernelGGL((k_score32<PPL, MC, false, MINW>), dim3(gx, psplit), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, H, H32, M, thr2, c.thr2_f, c.c_thr, c.k1, counts, mask, psplit, fallback_pairs);
    return hipGetLastError();
}

// H32: the table launch_model32 made for these M models.  fallback_pairs (nullable): device counter of the pairs decided in
// FP64.  tiling: points per lane / models per workgroup (a schedule choice; the counts do not depend on it).
hipError_t launch_score32(const Points& p, const double* H, const float* H32, int M, double thr2, double Cmax, const unsigned char* mask,
                          int* counts, unsigned long long* fallback_pairs, int tiling, hipStream_t s, int* resident_ctl, int cu_count,
                          int resident_slices, int* occ_cache)
{
    if (M <= 0 || p.n <= 0) return hipSuccess;
    if (tiling == 0 && resident_ctl && resident_slices != 0)
        return launch_score32_t<4, 64, 6>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s, resident_ctl, cu_count, resident_slices, occ_cache);
#ifdef MH_TUNING
    switch (tiling) {
    case 1: return launch_score32_t<4, 16>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 2: return launch_score32_t<8, 32>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 3: return launch_score32_t<4, 32>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 4: return launch_score32_t<8, 64>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 5: return launch_score32_t<6, 32>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 6: return launch_score32_t<8, 16>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 7: return launch_score32_t<4, 64>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 8: return launch_score32_t<4, 32, 5>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 9: return launch_score32_t<4, 32, 6>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 10: return launch_score32_t<4, 32, 8>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 11: return launch_score32_t<2, 32, 8>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 12: return launch_score32_t<4, 64, 6>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 13: return launch_score32_t<4, 32>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 14: return launch_score32_t<4, 64, 5>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 15: return launch_score32_t<4, 64, 8>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    case 16: return launch_score32_t<2, 64, 8>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
    default: break;
    }
#endif
    // 4 points per lane, 64 models per workgroup, registers capped at 80 for six waves per SIMD (2.20 ms; <4, 32, 5> 2.26, uncapped 2.51)
    return launch_score32_t<4, 64, 6>(p, H, H32, M, thr2, Cmax, mask, counts, fallback_pairs, s);
}

} // namespace mh
