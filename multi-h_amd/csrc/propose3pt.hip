// propose3pt.hip — F-constrained 3-point homography hypotheses as a proposal batch (mh_propose_3pt), gfx950.
//
// With F known a homography needs three point correspondences, H = [e']x F + e' v^T (GetHomography3PT, M/MultiH.cpp:995-1050).
// Hypothesis s of a batch has counter c = first + s; its tuple is the first three indices of the 4-tuple the proposer's sampler
// gives that counter (mh_sampler.hpp: sample_tuple<3, 64> draws what sample_tuple<4, 64> draws until its third index is found;
// sample4_by's i0, o1, o2 under the local sampler), its fit is homography_3pt_linear_dev (mh_device.hpp) — the post-filter's
// fit, operation for operation the host's Homography3PTLinear.  A fit that is not finite stores nine quiet NaNs: it scores 0.
// The definition is in include/multih_hip.h; tests/propose_3pt_numpy.py re-enacts it.
//
// One lane per hypothesis, 64-lane workgroups: at 100 000 hypotheses 1 563 waves for 1 024 SIMDs, each lane one dependent
// chain — the draws, twelve gathered doubles, two 3 x 3 Jacobi solves.  Nothing is shared between lanes; no LDS.  Out: 72 B of
// H and one 16-B store of the tuple (-1 in the fourth column, the width mh_get_samples has).  -ffp-contract=off.

#include "mh_kernels.hpp"
#include "mh_device.hpp"
#include "mh_sampler.hpp"

namespace mh {

namespace {

// the first three indices of sample4_by's tuple: the kernel hands on its trailing arguments as k_dlt4 does
__device__ __forceinline__ void sample3_by(unsigned long long seed, unsigned long long c, unsigned int N, int& i0, int& i1, int& i2)
{
    int t[3];
    sample_tuple<3, 64>(seed, c, N, t);
    i0 = t[0]; i1 = t[1]; i2 = t[2];
}

__device__ __forceinline__ void sample3_by(unsigned long long seed, unsigned long long c, unsigned int N, int& i0, int& i1, int& i2,
                                           const int* __restrict__ nbr, int k, int uniform_per_16)
{
    int t[4];
    sample4_by(seed, c, N, t, nbr, k, uniform_per_16);
    i0 = t[0]; i1 = t[1]; i2 = t[2];
}

} // namespace

template <int SAMPLER, class... TABLE>          // (as k_dlt4: no trailing argument, or nbr, k, uniform_per_16)
__global__ void __launch_bounds__(64)
k_propose_3pt(const double* __restrict__ x1, const double* __restrict__ y1,
              const double* __restrict__ x2, const double* __restrict__ y2, int N,
              unsigned long long seed, long long first, int M, Fund9 F, int* __restrict__ idx_out,
              double* __restrict__ H_out, TABLE... table)
{
    static_assert(sizeof...(TABLE) == (SAMPLER == DLT_SAMPLER_LOCAL ? 3 : 0), "the local sampler takes nbr, k, uniform_per_16");
    const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (s >= M) return;
    int i0, i1, i2;
    sample3_by(seed, (unsigned long long)(first + s), (unsigned int)N, i0, i1, i2, table...);
    double ms[6], md[6];
    ms[0] = x1[i0]; ms[1] = y1[i0]; md[0] = x2[i0]; md[1] = y2[i0];
    ms[2] = x1[i1]; ms[3] = y1[i1]; md[2] = x2[i1]; md[3] = y2[i1];
    ms[4] = x1[i2]; ms[5] = y1[i2]; md[4] = x2[i2]; md[5] = y2[i2];
    *reinterpret_cast<int4*>(idx_out + 4 * (size_t)s) = make_int4(i0, i1, i2, -1);
    double Hc[9];
    const bool good = homography_3pt_linear_dev(ms, md, F.f, Hc);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double* out = H_out + 9 * (size_t)s;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = good ? Hc[k] : qnan;
}

hipError_t launch_propose_3pt(const Points& p, const double F[9], unsigned long long seed, long long first, int M,
                              int* idx_out, double* H_out, hipStream_t s, Dlt4Local local)
{
    if (M <= 0) return hipSuccess;
    if (p.n < 3 || !idx_out || !H_out) return hipErrorInvalidValue;
    Fund9 f;
    for (int i = 0; i < 9; ++i) f.f[i] = F[i];
    const dim3 grid((unsigned)((M + 63) / 64));
    if (local.nbr) {
        if (local.k < 1 || local.k >= p.n || local.uniform_per_16 < 0 || local.uniform_per_16 > 16) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_propose_3pt<DLT_SAMPLER_LOCAL, const int*, int, int>), grid, dim3(64), 0, s, p.x1, p.y1, p.x2, p.y2,
                           p.n, seed, first, M, f, idx_out, H_out, local.nbr, local.k, local.uniform_per_16);
    } else
        hipLaunchKernelGGL(k_propose_3pt<DLT_SAMPLER_UNIFORM>, grid, dim3(64), 0, s, p.x1, p.y1, p.x2, p.y2,
                           p.n, seed, first, M, f, idx_out, H_out);
    return hipGetLastError();
}

} // namespace mh
