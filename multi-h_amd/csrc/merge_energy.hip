// merge_energy.hip — the energy of a given labeling and the energy change of joining two labels, gfx950
// (mh_labeling_energy, mh_merge_deltas; the definitions: include/multih_hip.h).
//
// k_merge_pair: one workgroup of 256 per pair (a, b).  S = S_a u S_b is found by for_pair_members (wg_fit.hpp) — the lane
// assignment and the ascending order of for_label_members, so H_ab = fit(S) has the bits of k_dlt_reestimate on the relabelled
// points.  Passes 1-3 are that kernel's (count and centroid sums; mean distances; the 24 sums); thread 0 solves while the
// others wait at the next barrier, and H_ab reaches them through LDS.  Pass 4: every member's cost under its own resident
// model and under H_ab (fwd_d2 / sym_d2 and data_term, k_data_cost's arithmetic), and over its own CSR row the arcs to a lower
// index on the pair's other side (k_energy's `col[k] < p`: an undirected neighbour pair counts once).  The three integer
// partials are summed per wave by shuffles and per workgroup by one LDS atomic per wave: integer sums have no order.
// k_labeling_energy: one thread per site, the same two terms over the whole labeling, one int64 atomic per block and word.
//
// Loops are bounded by N, a row's length and Jacobi's 30 sweeps; a workgroup waits for nothing but its own barriers; every
// early exit is taken by all 256 threads on a value read from LDS behind a barrier, before any later barrier.  Every global
// index is bounded by its launch's sizes: points and labels by N, models by the host's check of the pairs and labels against
// Nh, arcs by rowptr (the engine's own symmetric graph), outputs by the pair / block index.

#include "mh_kernels.hpp"
#include "wg_fit.hpp"

namespace mh {

namespace {

template <bool RISING, bool SYM>
__device__ __forceinline__ int site_cost(const double* __restrict__ h, const double* __restrict__ adj, double x, double y, double u,
                                         double v, double T, double lam, int beyond)
{
    const double d2 = SYM ? sym_d2(h, adj, x, y, u, v) : fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x, y, u, v);
    return data_term<RISING>(d2, T, lam, beyond);
}

// the wave's sum in every lane
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

} // namespace

template <bool RISING, bool SYM>
__global__ void __launch_bounds__(256)
k_merge_pair(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
             const double* __restrict__ y2, const int* __restrict__ labels, int N, const double* __restrict__ H,
             const int* __restrict__ pairs, const int* __restrict__ rowptr, const int* __restrict__ col,
             const int* __restrict__ w, double lam, double T, int potts, double* __restrict__ H_out,
             long long* __restrict__ out /* npairs x 5: |S|, data_old, data_new, cut, delta */, int* __restrict__ status)
{
    const int pr = blockIdx.x, t = threadIdx.x;
    const int a = pairs[2 * pr], b = pairs[2 * pr + 1];
    __shared__ double sv[256][DLT_SUMS];         // 48 KB: the partial sums; then dlt_solve's work space
    __shared__ int sc[256];
    __shared__ double s_par[6];                  // cx1 cy1 cx2 cy2 s1 s2
    __shared__ double s_G[DLT_SUMS];
    __shared__ double s_M[3][9], s_A[SYM ? 3 : 1][9];      // H[a], H[b], H_ab and (SYM) their adjugates
    __shared__ unsigned long long s_sum[3];      // data_old, data_new, arcs across
    __shared__ int s_cb, s_ok;
    auto members = [&](auto&& f) { for_pair_members<16, long long>(labels, N, a, b, t, f); };

    if (t < 3) s_sum[t] = 0ull;
    if (t == 0) s_cb = 0;
    if (t < 18) s_M[t / 9][t % 9] = H[9 * (size_t)(t < 9 ? a : b) + t % 9];
    __syncthreads();
    // pass 1
    {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int cnt = 0, cnt_b = 0;
        members([&](int n, bool is_b) {
            a0 = a0 + x1[n]; a1 = a1 + y1[n]; a2 = a2 + x2[n]; a3 = a3 + y2[n];
            ++cnt;
            cnt_b += is_b ? 1 : 0;
        });
        sv[t][0] = a0; sv[t][1] = a1; sv[t][2] = a2; sv[t][3] = a3;
        sc[t] = cnt;
        if (cnt_b) atomicAdd(&s_cb, cnt_b);
        wg_tree<4>(sv, sc, t);
    }
    const int c = sc[0], cb = s_cb;              // (LDS, behind the tree's last barrier: the same in every thread)
    if (cb == 0 || cb == c) {
        if (t == 0) status[pr] = MERGE_EMPTY;
        return;
    }
    if (c < 4) {
        if (t == 0) status[pr] = MERGE_NO_FIT;
        return;
    }
    Hartley hn;
    hartley_centroids(sv[0], c, s_par, t, hn);
    // pass 2
    {
        double d1 = 0.0, d2 = 0.0;
        members([&](int n, bool) { hartley_distances(hn, x1[n], y1[n], x2[n], y2[n], d1, d2); });
        sv[t][0] = d1; sv[t][1] = d2;
        wg_tree<2>(sv, t);
    }
    hartley_scales(sv[0], c, s_par, t, hn);
    if (!finite_dev(hn.s1) || !finite_dev(hn.s2)) {                      // (s_par, behind hartley_scales' barrier)
        if (t == 0) status[pr] = MERGE_NO_FIT;
        return;
    }
    // pass 3
    {
        double acc[DLT_SUMS];
#pragma unroll
        for (int k = 0; k < DLT_SUMS; ++k) acc[k] = 0.0;
        members([&](int n, bool) { dlt_accumulate(hn, x1[n], y1[n], x2[n], y2[n], acc); });
#pragma unroll
        for (int k = 0; k < DLT_SUMS; ++k) sv[t][k] = acc[k];
        wg_tree<DLT_SUMS>(sv, t);
    }
    if (t < DLT_SUMS) s_G[t] = sv[0][t];
    __syncthreads();                             // the reduction buffer is idle from here: the solve's work space
    if (t == 0) {
        double Hh[9];
        dlt_solve(s_G, hn, &sv[0][0], Hh);
        bool finite = true;
#pragma unroll
        for (int j = 0; j < 9; ++j) finite = finite && finite_dev(Hh[j]);
#pragma unroll
        for (int j = 0; j < 9; ++j) s_M[2][j] = Hh[j];
        s_ok = finite ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) {
        if (t == 0) status[pr] = MERGE_NO_FIT;
        return;
    }
    if (SYM) {
        if (t < 3) adjugate(s_M[t], s_A[t]);
        __syncthreads();
    }
    // pass 4
    {
        const int beyond = 2 * (int)round(lam * T);
        long long d_old = 0, d_new = 0, across = 0;
        members([&](int n, bool is_b) {
            const double x = x1[n], y = y1[n], u = x2[n], v = y2[n];
            const int own = is_b ? 1 : 0;
            d_old += site_cost<RISING, SYM>(s_M[own], s_A[SYM ? own : 0], x, y, u, v, T, lam, beyond);
            d_new += site_cost<RISING, SYM>(s_M[2], s_A[SYM ? 2 : 0], x, y, u, v, T, lam, beyond);
            const int other = is_b ? a : b;
            for (int k = rowptr[n]; k < rowptr[n + 1]; ++k) {
                const int q = col[k];
                if (q < n && labels[q] == other) across += w[k];
            }
        });
        d_old = wave_sum(d_old); d_new = wave_sum(d_new); across = wave_sum(across);
        if ((t & 63) == 0) {
            atomicAdd(&s_sum[0], (unsigned long long)d_old);
            atomicAdd(&s_sum[1], (unsigned long long)d_new);
            atomicAdd(&s_sum[2], (unsigned long long)across);
        }
    }
    __syncthreads();
    if (t < 9) H_out[9 * (size_t)pr + t] = s_M[2][t];
    if (t != 0) return;
    const long long data_old = (long long)s_sum[0], data_new = (long long)s_sum[1], cut = (long long)potts * (long long)s_sum[2];
    long long* o = out + 5 * (size_t)pr;
    o[0] = c; o[1] = data_old; o[2] = data_new; o[3] = cut; o[4] = data_new - data_old - cut;
    status[pr] = MERGE_OK;
}

template <bool RISING, bool SYM>
__global__ void __launch_bounds__(256)
k_labeling_energy(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                  const double* __restrict__ y2, const int* __restrict__ labels, int N, const double* __restrict__ H,
                  const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ w, double lam, double T,
                  int potts, unsigned long long* __restrict__ out /* data, smooth */)
{
    const int t = threadIdx.x;
    const int p = blockIdx.x * 256 + t;
    __shared__ unsigned long long s_sum[2];
    if (t < 2) s_sum[t] = 0ull;
    __syncthreads();
    long long data = 0, arcs = 0;
    if (p < N) {
        const int lb = labels[p];
        if (lb < 0) {
            data = (int)round(lam * T);
        } else {
            const double* h = H + 9 * (size_t)lb;
            double adj[9];
            if (SYM) adjugate(h, adj);
            data = site_cost<RISING, SYM>(h, adj, x1[p], y1[p], x2[p], y2[p], T, lam, 2 * (int)round(lam * T));
        }
        for (int k = rowptr[p]; k < rowptr[p + 1]; ++k) {
            const int q = col[k];
            if (q < p && labels[q] != lb) arcs += w[k];
        }
    }
    data = wave_sum(data); arcs = wave_sum(arcs);
    if ((t & 63) == 0) {
        atomicAdd(&s_sum[0], (unsigned long long)data);
        atomicAdd(&s_sum[1], (unsigned long long)arcs);
    }
    __syncthreads();
    if (t == 0) {
        atomicAdd(&out[0], s_sum[0]);
        atomicAdd(&out[1], (unsigned long long)((long long)potts * (long long)s_sum[1]));
    }
}

hipError_t launch_merge_pairs(const Points& p, const int* labels, const double* H, const int* pairs, int npairs, const Graph& g,
                              double lambda, double thr2, double* H_out, long long* out, int* status, hipStream_t s, int rising,
                              int symmetric)
{
    if (npairs <= 0) return hipSuccess;
    if (p.n < 0) return hipErrorInvalidValue;
    const double lam = 100.0 / lambda, T = thr2 * 81.0 / 16.0;
    const int potts = (int)std::round(100.0 * lambda);
    auto run = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(npairs), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, labels, p.n, H, pairs, g.rowptr, g.col, g.w,
                           lam, T, potts, H_out, out, status);
    };
    if (symmetric) { if (rising) run(k_merge_pair<true, true>); else run(k_merge_pair<false, true>); }
    else if (rising) run(k_merge_pair<true, false>);
    else run(k_merge_pair<false, false>);
    return hipGetLastError();
}

hipError_t launch_labeling_energy(const Points& p, const int* labels, const double* H, const Graph& g, double lambda, double thr2,
                                  unsigned long long* out, hipStream_t s, int rising, int symmetric)
{
    if (p.n <= 0) return hipSuccess;
    const double lam = 100.0 / lambda, T = thr2 * 81.0 / 16.0;
    const int potts = (int)std::round(100.0 * lambda);
    auto run = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((p.n + 255) / 256), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, labels, p.n, H, g.rowptr, g.col,
                           g.w, lam, T, potts, out);
    };
    if (symmetric) { if (rising) run(k_labeling_energy<true, true>); else run(k_labeling_energy<false, true>); }
    else if (rising) run(k_labeling_energy<true, false>);
    else run(k_labeling_energy<false, false>);
    return hipGetLastError();
}

} // namespace mh
