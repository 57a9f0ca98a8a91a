// mh_sampler.hpp — the counter RNG and the tuple samplers of the proposers: shared by dlt4.hip (k_dlt4,
// k_dlt4_lds, k_fund8, k_fund7) and propose3pt.hip (k_propose_3pt), so that a counter means the same tuple to all of them.
#pragma once
#include <hip/hip_runtime.h>

namespace mh {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// K distinct indices for hypothesis m: draw c gives r = splitmix64(seed + (m<<8) + c),
// idx = ((r>>32)*N)>>32; duplicates inside the tuple are rejected; at most MAXDRAW (<= 256) draws.
template <int K, int MAXDRAW>
__device__ __forceinline__ void sample_tuple(unsigned long long seed, unsigned long long m,
                                             unsigned int N, int* out)
{
    int got = 0;
    for (unsigned int c = 0; c < MAXDRAW && got < K; ++c) {
        const unsigned long long r = splitmix64(seed + (m << 8) + c);
        const int idx = (int)(((r >> 32) * (unsigned long long)N) >> 32);
        bool dup = false;
        for (int k = 0; k < got; ++k) dup = dup || (out[k] == idx);
        if (!dup) out[got++] = idx;
    }
    for (; got < K; ++got) out[got] = out[0];
}

__device__ __forceinline__ void sample4(unsigned long long seed, unsigned long long m,
                                        unsigned int N, int out[4])
{
    sample_tuple<4, 64>(seed, m, N, out);
}

// The tuple of hypothesis c under the sampler of k_dlt4 / k_dlt4_lds.  The kernels hand on their trailing
// arguments: none under DLT_SAMPLER_UNIFORM, which is sample4 and nothing else; the sampling table under DLT_SAMPLER_LOCAL.
// There the hypotheses with (c & 15) < uniform_per_16 keep the uniform tuple; the others take the uniform tuple's first index
// i0 and fill up from row i0 of the table (nbr: n x k, the k nearest neighbours of every point, all in [0, n)): draw
// j = 1 .. 63 proposes nbr[i0 k + (((r_j >> 32) k) >> 32)], taken unless it is already in the tuple; slots still empty after
// draw 63 take out[0] (sample_tuple's exhaustion rule).  One more dependent load per index than the uniform form; the indices
// live in named registers, not in an indexed array (no scratch).
// DLT_SAMPLER_SEGMENT (the trials of mh_compat_dlt_medians, register form only): the hypotheses of a launch are `trials` per
// segment of the point array; hypothesis c - first belongs to segment q = (c - first) / trials = [begin[q], begin[q + 1]), draws
// sample4's tuple for counter c over the segment's begin[q + 1] - begin[q] positions and adds begin[q].  The arguments are
// cluster_begin, trials, first.
constexpr int DLT_SAMPLER_UNIFORM = 0, DLT_SAMPLER_LOCAL = 1, DLT_SAMPLER_SEGMENT = 2;
// how many trailing arguments k_dlt4 / k_dlt4_lds hand on to sample4_by under a sampler
constexpr int dlt_sampler_args(int sampler) { return sampler == DLT_SAMPLER_UNIFORM ? 0 : 3; }

__device__ __forceinline__ void sample4_by(unsigned long long seed, unsigned long long c, unsigned int N, int out[4])
{
    sample4(seed, c, N, out);
}

__device__ __forceinline__ void sample4_by(unsigned long long seed, unsigned long long c, unsigned int N, int out[4],
                                           const int* __restrict__ nbr, int k, int uniform_per_16)
{
    if ((int)(c & 15ull) < uniform_per_16) { sample4(seed, c, N, out); return; }
    const unsigned long long base = seed + (c << 8);
    const int i0 = (int)(((splitmix64(base) >> 32) * (unsigned long long)N) >> 32);
    const int* __restrict__ row = nbr + (size_t)i0 * (size_t)k;
    int o1 = -1, o2 = -1, o3 = -1, got = 1;                       // (-1 equals no table entry)
    for (unsigned int j = 1; j < 64 && got < 4; ++j) {
        const unsigned long long r = splitmix64(base + j);
        const int cand = row[(int)(((r >> 32) * (unsigned long long)(unsigned int)k) >> 32)];
        if (cand != i0 && cand != o1 && cand != o2) {
            o1 = got == 1 ? cand : o1;
            o2 = got == 2 ? cand : o2;
            o3 = got == 3 ? cand : o3;
            ++got;
        }
    }
    out[0] = i0;
    out[1] = got > 1 ? o1 : i0;
    out[2] = got > 2 ? o2 : i0;
    out[3] = got > 3 ? o3 : i0;
}

// sample_tuple<4, 64> over the nc positions of the hypothesis' segment, shifted by the segment's start: the same draws, the same
// rejection and the same exhaustion rule, the tuple in named registers.  (The point count N of the launch is not read.)
__device__ __forceinline__ void sample4_by(unsigned long long seed, unsigned long long c, unsigned int, int out[4],
                                           const int* __restrict__ cluster_begin, int trials, long long first)
{
    const int q = (int)((long long)c - first) / trials;
    const int b0 = cluster_begin[q];
    const unsigned long long nc = (unsigned long long)(unsigned int)(cluster_begin[q + 1] - b0);
    const unsigned long long base = seed + (c << 8);
    int o0 = -1, o1 = -1, o2 = -1, o3 = -1, got = 0;                // (-1 equals no position)
    for (unsigned int j = 0; j < 64 && got < 4; ++j) {
        const int cand = (int)(((splitmix64(base + j) >> 32) * nc) >> 32);
        if (cand != o0 && cand != o1 && cand != o2) {
            o0 = got == 0 ? cand : o0;
            o1 = got == 1 ? cand : o1;
            o2 = got == 2 ? cand : o2;
            o3 = got == 3 ? cand : o3;
            ++got;
        }
    }
    out[0] = b0 + o0;
    out[1] = b0 + (got > 1 ? o1 : o0);
    out[2] = b0 + (got > 2 ? o2 : o0);
    out[3] = b0 + (got > 3 ? o3 : o0);
}

} // namespace mh
