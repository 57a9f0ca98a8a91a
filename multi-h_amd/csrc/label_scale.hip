// label_scale.hip — mh_label_residual_quantile and mh_reweight_homographies_auto: per label, one order statistic of its
// members' forward transfer errors, and the reweighted rounds of reweight_h.hip with the scale c2 taken from that statistic in
// every round, gfx950.  The rules are stated in include/multih_hip.h and restated in tests/label_scale_numpy.py.
//
// One 256-thread workgroup per label (blockIdx.x = k).  Members come from for_label_members, so in the reweighting kernel the
// lane assignment stays the engine's order of every FP64 sum; the order statistic itself depends on no order at all.
//
// The selection (label_quantile, wg_select.hpp) is a radix select on the 64-bit pattern of the key, most significant digit
// first; its design notes stand there.  Here:
//     keys            recomputed from the model in every pass, as the weights of k_reweight_h are; the passes are label-fetch
//                     bound and small next to thread 0's serial Jacobi.
//     histogram       in LDS of its own, not in the idle reduction buffer: 1 KB beside the 48 KB, and the selection then
//                     never has to be ordered against the tree's or the solve's use of that buffer.
// Every loop is bounded (eight digit passes, rounds <= 16, Jacobi's 30 sweeps), every exit is taken by the whole workgroup
// (the conditions are read from LDS behind a barrier), nothing waits on anything but the workgroup's own barriers.
//
// k_autoscale_reweight_h is k_reweight_h with `c2 = scale(cur)` in front of each pass 1: a call of r rounds is r + 1
// selections and 3 r + 1 passes.  With c2_min == c2_max the clamp returns that value whatever the selection found, and every
// other operation is k_reweight_h's: the same bits.

#include <cmath>
#include "mh_kernels.hpp"
#include "wg_fit.hpp"
#include "wg_select.hpp"

namespace mh {

namespace {

// c2 from the order statistic q (never a NaN, never negative): one multiplication, clamped to [c2_min, c2_max]
__device__ __forceinline__ double autoscale_c2(double q, double kappa2, double c2_min, double c2_max)
{
    const double s = kappa2 * q;
    return s < c2_min ? c2_min : (s > c2_max ? c2_max : s);
}

constexpr int RW_HEAD = 6;                       // pass 1's columns: four weighted coordinate sums, W, support

} // namespace

// H: m x 9; d2_out: m doubles; info: m x 4 (members, rank, members strictly below the value, status), nullable.
__global__ void __launch_bounds__(256)
k_label_quantile(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                 const double* __restrict__ y2, int N, const int* __restrict__ labels, const double* __restrict__ H, int num, int den,
                 double* __restrict__ d2_out, int* __restrict__ info)
{
    const int l = blockIdx.x, t = threadIdx.x;
    __shared__ unsigned s_hist[256];
    __shared__ int s_sel[5];
    double h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = H[9 * (size_t)l + i];
    auto members = [&](auto&& f) { for_label_members<16, long long>(labels, N, l, t, f); };
    auto key_of = [&](int n) {
        return quantile_key(fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x1[n], y1[n], x2[n], y2[n]));
    };
    const Quantile q = label_quantile(members, key_of, num, den, s_hist, s_sel, t);
    if (t == 0) {
        const bool none = q.members == 0;
        d2_out[l] = __longlong_as_double((long long)(none ? KEY_QNAN : q.key));
        if (info) {
            int* o = info + 4 * (size_t)l;
            o[0] = q.members; o[1] = none ? 0 : q.rank; o[2] = none ? 0 : q.below; o[3] = none ? 1 : 0;
        }
    }
}

// H_in, H_out: m x 9 (may be the same array: a workgroup reads its row before it writes it); gain: m x 2 (W of H_in at its
// scale, W of H_out at its scale), scale: m x 2 (c2 under H_in, c2 under H_out), info: m x 4 (members, support of H_out at its
// scale, rounds done, status), counts: m (members) — the last four nullable.
__global__ void __launch_bounds__(256)
k_autoscale_reweight_h(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                       const double* __restrict__ y2, int N, const int* __restrict__ labels, const double* H_in, int num, int den,
                       double kappa2, double c2_min, double c2_max, int rounds, double* H_out, double* __restrict__ gain,
                       double* __restrict__ scale, int* __restrict__ info, int* __restrict__ counts)
{
    const int l = blockIdx.x, t = threadIdx.x;
    __shared__ double sv[256][DLT_SUMS];         // 48 KB: the partial sums; then dlt_solve's work space
    __shared__ double s_cur[9];                  // the model that stands
    __shared__ double s_par[6];                  // cx1 cy1 cx2 cy2 s1 s2
    __shared__ double s_G[DLT_SUMS];
    __shared__ unsigned s_hist[256];             // the selection's histogram
    __shared__ int s_sel[5];
    __shared__ int s_stop;
    auto members = [&](auto&& f) { for_label_members<16, long long>(labels, N, l, t, f); };

    if (t < 9) s_cur[t] = H_in[9 * (size_t)l + t];
    __syncthreads();
    bool finite_in = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) finite_in = finite_in && finite_dev(s_cur[j]);

    int n_members = 0, support = 0, done = 0, status = 0;
    double W_in = 0.0, W_cur = 0.0, c2_in = 0.0, c2_cur = 0.0;
    for (int r = 0; ; ++r) {                     // at most rounds + 1 <= 17 trips
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = s_cur[i];
        auto d2_of = [&](double x, double y, double u, double v) {
            return fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x, y, u, v);
        };

        // c2 = scale(cur)
        const Quantile q = label_quantile(members, [&](int n) { return quantile_key(d2_of(x1[n], y1[n], x2[n], y2[n])); }, num, den,
                                          s_hist, s_sel, t);
        if (r == 0) {
            n_members = q.members;
            status = n_members < 4 ? 1 : (!finite_in ? 2 : 0);
            if (status != 0) break;              // (the same for every thread, like every break below)
        }
        const double c2 = autoscale_c2(__longlong_as_double((long long)q.key), kappa2, c2_min, c2_max);
        auto weight = [&](double x, double y, double u, double v) { return reweight_w(d2_of(x, y, u, v), c2); };

        // pass 1
        {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, aw = 0.0;
            int in = 0;
            members([&](int n) {
                const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
                const double w = weight(x, y, u, v);
                if (w > 0.0) {
                    a0 = a0 + w * x; a1 = a1 + w * y; a2 = a2 + w * u; a3 = a3 + w * v;
                    aw = aw + w;
                    ++in;
                }
            });
            sv[t][0] = a0; sv[t][1] = a1; sv[t][2] = a2; sv[t][3] = a3; sv[t][4] = aw;
            sv[t][5] = (double)in;               // (a count is exact as a double)
            wg_tree<RW_HEAD>(sv, t);
        }
        const double W = sv[0][4];
        const int c = (int)sv[0][5];
        if (r == 0) { W_in = W; c2_in = c2; }
        W_cur = W; support = c; c2_cur = c2;
        if (r == rounds) break;

        // wfit(cur)
        if (c < 4) break;
        Hartley hn;
        hartley_centroids_w(sv[0], W, s_par, t, hn);
        // pass 2
        {
            double d1 = 0.0, d2 = 0.0;
            members([&](int n) {
                const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
                const double w = weight(x, y, u, v);
                if (w > 0.0) hartley_distances_w(hn, w, x, y, u, v, d1, d2);
            });
            sv[t][0] = d1; sv[t][1] = d2;
            wg_tree<2>(sv, t);
        }
        hartley_scales_w(sv[0], W, s_par, t, hn);
        if (!finite_dev(hn.s1) || !finite_dev(hn.s2)) break;
        // pass 3
        {
            double acc[DLT_SUMS];
#pragma unroll
            for (int k = 0; k < DLT_SUMS; ++k) acc[k] = 0.0;
            members([&](int n) {
                const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
                const double w = weight(x, y, u, v);
                if (w > 0.0) dlt_accumulate_w(hn, w, x, y, u, v, acc);
            });
#pragma unroll
            for (int k = 0; k < DLT_SUMS; ++k) sv[t][k] = acc[k];
            wg_tree<DLT_SUMS>(sv, t);
        }
        if (t < DLT_SUMS) s_G[t] = sv[0][t];
        __syncthreads();                         // the reduction buffer is idle from here: the solve's work space
        if (t == 0) {
            double o[9];
            dlt_solve(s_G, hn, &sv[0][0], o);
            bool finite = true, same = true;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                finite = finite && finite_dev(o[j]);
                same = same && (__double_as_longlong(o[j]) == __double_as_longlong(s_cur[j]));
            }
            const bool stop = !finite || same;
            if (!stop) {
#pragma unroll
                for (int j = 0; j < 9; ++j) s_cur[j] = o[j];
            }
            s_stop = stop ? 1 : 0;
        }
        __syncthreads();
        if (s_stop) break;                       // (W_cur, support and c2_cur are those of the model that stands)
        ++done;
    }

    if (t < 9) H_out[9 * (size_t)l + t] = s_cur[t];                          // (H_in's bits when nothing was done)
    if (t == 0) {
        if (counts) counts[l] = n_members;
        if (gain) {
            gain[2 * (size_t)l] = status == 0 ? W_in : 0.0;
            gain[2 * (size_t)l + 1] = status == 0 ? W_cur : 0.0;
        }
        if (scale) {
            scale[2 * (size_t)l] = status == 0 ? c2_in : 0.0;
            scale[2 * (size_t)l + 1] = status == 0 ? c2_cur : 0.0;
        }
        if (info) {
            int* o = info + 4 * (size_t)l;
            o[0] = n_members; o[1] = status == 0 ? support : 0; o[2] = done; o[3] = status;
        }
    }
}

static bool quantile_args_ok(int num, int den) { return den >= 1 && den <= LABEL_QUANTILE_MAX_DEN && num >= 0 && num <= den; }

hipError_t launch_label_quantile(const Points& p, const int* labels, const double* H, int m, int num, int den, double* d2_out,
                                 int* info, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    if (p.n <= 0 || !labels || !H || !d2_out || !quantile_args_ok(num, den)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_label_quantile, dim3(m), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, labels, H, num, den, d2_out, info);
    return hipGetLastError();
}

hipError_t launch_autoscale_reweight_h(const Points& p, const int* labels, const double* H_in, int m, const AutoScale& a, int rounds,
                                       double* H_out, double* gain, double* scale, int* info, int* counts, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    if (p.n <= 0 || rounds < 0 || rounds > REWEIGHT_H_MAX_ROUNDS || !labels || !autoscale_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_autoscale_reweight_h, dim3(m), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, labels, H_in, a.num, a.den,
                       a.kappa2, a.c2_min, a.c2_max, rounds, H_out, gain, scale, info, counts);
    return hipGetLastError();
}

bool autoscale_ok(const AutoScale& a)
{
    return quantile_args_ok(a.num, a.den) && std::isfinite(a.kappa2) && a.kappa2 > 0.0 && std::isfinite(a.c2_min) &&
           std::isfinite(a.c2_max) && a.c2_min > 0.0 && a.c2_min <= a.c2_max;
}

} // namespace mh
