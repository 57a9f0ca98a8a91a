// wg_select.hpp — one order statistic of a multiset of keys by a 256-thread workgroup: the radix select of label_scale.hip
// (k_label_quantile, k_autoscale_reweight_h) and of the 4-point compatibility trials (compat.hip: k_compat_median4,
// k_compat_cluster_median), stated once.
//
// A radix select on the 64-bit pattern of the key, most significant digit first — the pattern of k_compat_select: the key is a
// sum of two squares (never negative, never -0; a NaN is replaced by +inf), so its pattern orders like the number.
//     digit width     8 bits: at most eight passes, a 256-bin histogram (1 KB of LDS) whose prefix one wavefront finds with four bins
//                     per lane.  Wider digits save passes (11 bits: six) but need a scan over more bins than one wavefront
//                     holds in registers.
//     keys            recomputed by the caller's key_of in every pass: no per-member storage, so no bound on the members and no
//                     global scratch.
//     members, rank   the first pass matches every member, so its histogram's total is c = the number of members: the rank
//                     ((c - 1) * num) / den is formed there, no counting pass.  The sum over the passes of the matching keys in
//                     lower bins is the number of members strictly below the result.
// Every loop is bounded (eight digit passes), every exit is taken by the whole workgroup (the conditions are read from LDS behind
// a barrier), nothing waits on anything but the workgroup's own barriers.
#pragma once
#include <hip/hip_runtime.h>

namespace mh {

namespace {

typedef unsigned long long u64;

constexpr u64 KEY_INF = 0x7ff0000000000000ull;
constexpr u64 KEY_QNAN = 0x7ff8000000000000ull;

struct Quantile { u64 key; int members, rank, below; };     // members == 0: nothing else is set

// the key of a member: the pattern of its squared error, +inf for a NaN
__device__ __forceinline__ u64 quantile_key(double d2) { return d2 != d2 ? KEY_INF : (u64)__double_as_longlong(d2); }

// The element at 0-based rank ((c - 1) * num) / den of the ascending multiset { key_of(n) : n a member }.  Every thread of the
// workgroup calls it and gets the same result.  hist: 256 words of LDS, sel: 5 words of LDS (bin, rank inside the bin, keys in
// lower bins, members, keys in the bin); both free again on return.  Once the bin of the rank holds ONE key, that key is the
// result: one more pass fetches it instead of the remaining digit passes (continuous data: after three or four digits; ties
// run all eight).
template <class Members, class Key>
__device__ __forceinline__ Quantile label_quantile(Members&& members, Key&& key_of, int num, int den, unsigned* hist, int* sel, int t)
{
    Quantile q;
    q.key = 0; q.members = 0; q.rank = 0; q.below = 0;
    u64 prefix = 0, mask = 0;
    int want = 0;                                // rank still to be found among the keys that match the prefix
    bool lone = false;                           // exactly one key matches the prefix, and digits are left
#pragma unroll 1
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        members([&](int n) {
            const u64 k = key_of(n);
            if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
        });
        __syncthreads();
        if (t < 64) {                            // one wavefront: four bins per lane, prefix over the lanes
            const unsigned c0 = hist[4 * t], c1 = hist[4 * t + 1], c2 = hist[4 * t + 2], c3 = hist[4 * t + 3];
            const unsigned s = c0 + c1 + c2 + c3;
            unsigned incl = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const unsigned y = __shfl_up(incl, d, 64); if (t >= d) incl += y; }
            unsigned w = (unsigned)want;
            if (shift == 56) {                   // every member matched: the total is c, and the rank follows
                const unsigned c = __shfl(incl, 63, 64);
                w = c > 0 ? (unsigned)(((long long)(c - 1) * num) / den) : 0u;
                if (t == 0) sel[3] = (int)c;
            }
            const unsigned excl = incl - s;
            if (excl <= w && w < incl) {         // exactly one lane (none when there is no member)
                unsigned r = w - excl, lower = excl, eq = c0;
                int b = 4 * t;
                if (r >= c0) { r -= c0; lower += c0; ++b; eq = c1; if (r >= c1) { r -= c1; lower += c1; ++b; eq = c2; if (r >= c2) { r -= c2; lower += c2; ++b; eq = c3; } } }
                sel[0] = b; sel[1] = (int)r; sel[2] = (int)lower; sel[4] = (int)eq;
            }
        }
        __syncthreads();
        if (shift == 56) {
            q.members = sel[3];
            if (q.members == 0) break;           // (the same for every thread)
            q.rank = (int)(((long long)(q.members - 1) * num) / den);
        }
        want = sel[1];
        q.below += sel[2];
        prefix |= (u64)(unsigned)sel[0] << shift;
        mask |= 0xffull << shift;
        if (sel[4] == 1 && shift > 0) { lone = true; break; }
    }
    if (lone) {                                  // (the same for every thread) the one member that matches hands its key over
        members([&](int n) {
            const u64 k = key_of(n);
            if ((k & mask) == prefix) { hist[0] = (unsigned)k; hist[1] = (unsigned)(k >> 32); }
        });
        __syncthreads();
        prefix = (u64)hist[0] | ((u64)hist[1] << 32);
    }
    __syncthreads();                             // sel and hist are read no more: the caller may run the next selection
    q.key = prefix;
    return q;
}

} // namespace

} // namespace mh
