// label_cost.hip — every site's best alternative label and the energy change of dropping a label, gfx950
// (mh_best_alternative, mh_drop_deltas; the definitions: include/multih_hip.h).
//
// k_best_alternative: the N x Nh arg-min, never written as a table.  One site per lane, 256 sites per workgroup; the models
// pass through LDS in tiles of BEST_ALT_TILE: a tile's nine coefficients, its used flag and (SYM) its adjugate, computed
// once per tile.  A lane walks the tile's used labels in ascending index and keeps a running (cost, label) that is replaced
// on a strictly smaller cost only: starting from the outlier's cost (where the site is not an outlier itself) that is the
// first minimum in the order -1, 0, 1, ...  The cost under the site's own label is kept aside (own_cost).  The arithmetic is
// k_data_cost's: fwd_d2 / sym_d2 with adj(H) by `adjugate`, data_term<RISING>.
// k_drop_label: one workgroup of 256 per candidate label k; its members by for_label_members (wg_fit.hpp).  Per member its
// cost under H[k], its alt_cost, and over its CSR row the arcs with an end in S_k: an arc to another member counts from the
// higher index alone, an arc to a site outside from the member's side alone, so every undirected pair counts once.  Four
// int64 partials per thread, summed per wave by shuffles and per workgroup by one LDS atomic per wave (k_merge_pair's way):
// integer sums have no order.
//
// Loops are bounded by N, Nh and a row's length; a workgroup waits for nothing but its own barriers, which every thread
// reaches (no thread leaves before the last one).  Every global index is bounded by its launch's sizes: points, labels, alt
// and alt_cost by N, models by Nh (the tile's guard; the host's check of labels and candidates), arcs by rowptr (the engine's
// own symmetric graph), outputs by the site / candidate index.

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

constexpr int NO_COST = 0x7fffffff;              // above every cost: a cost is at most 2 round(lam T), an int

} // namespace

template <bool RISING, bool SYM>
__global__ void __launch_bounds__(256)
k_best_alternative(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
                   const double* __restrict__ y2, const int* __restrict__ labels, int N, const double* __restrict__ H, int Nh,
                   const int* __restrict__ used, double lam, double T, int* __restrict__ alt, int* __restrict__ alt_cost,
                   int* __restrict__ own_cost)
{
    constexpr int TILE = BEST_ALT_TILE;
    const int t = threadIdx.x;
    const long long site = (long long)blockIdx.x * 256 + t;
    const bool in = site < N;
    const int i = in ? (int)site : 0;
    __shared__ double s_h[TILE][9];
    __shared__ double s_a[SYM ? TILE : 1][9];
    __shared__ int s_used[TILE];
    const int outlier = (int)round(lam * T), beyond = 2 * outlier;
    const int lb = in ? labels[i] : -1;
    const double x = in ? x1[i] : 0.0, y = in ? y1[i] : 0.0, u = in ? x2[i] : 0.0, v = in ? y2[i] : 0.0;
    int best = lb < 0 ? NO_COST : outlier, best_l = -1, own = outlier;
    for (int m0 = 0; m0 < Nh; m0 += TILE) {
        const int cnt = Nh - m0 < TILE ? Nh - m0 : TILE;
        __syncthreads();                         // the last tile's readers are done
        for (int k = t; k < 9 * cnt; k += 256) s_h[k / 9][k % 9] = H[9 * (size_t)m0 + k];
        if (t < cnt) s_used[t] = used[m0 + t];
        __syncthreads();
        if (SYM) {
            if (t < cnt && s_used[t]) adjugate(s_h[t], s_a[t]);
            __syncthreads();
        }
        if (!in) continue;                       // (the barriers above are reached in every trip: cnt and Nh are uniform)
        for (int mi = 0; mi < cnt; ++mi) {
            if (!s_used[mi]) continue;
            const int c = site_cost<RISING, SYM>(s_h[mi], s_a[SYM ? mi : 0], x, y, u, v, T, lam, beyond);
            const int l = m0 + mi;
            if (l == lb) own = c;
            else if (c < best) { best = c; best_l = l; }
        }
    }
    if (!in) return;
    alt[i] = best_l;
    if (alt_cost) alt_cost[i] = best == NO_COST ? outlier : best;
    if (own_cost) own_cost[i] = own;
}

template <bool RISING, bool SYM>
__global__ void __launch_bounds__(256)
k_drop_label(const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
             const double* __restrict__ y2, const int* __restrict__ labels, int N, const double* __restrict__ H,
             const int* __restrict__ cand, const int* __restrict__ alt, const int* __restrict__ alt_cost,
             const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ w, double lam, double T, int potts,
             long long* __restrict__ out /* ncand x 5: |S_k|, data_old, data_new, smooth_old, smooth_new */, int* __restrict__ status)
{
    const int c = blockIdx.x, t = threadIdx.x;
    const int k = cand[c];
    __shared__ double s_M[9], s_A[9];
    __shared__ unsigned long long s_sum[4];      // data_old, data_new, arcs cut before, arcs cut after
    __shared__ int s_cnt;
    if (t < 4) s_sum[t] = 0ull;
    if (t == 0) s_cnt = 0;
    if (t < 9) s_M[t] = H[9 * (size_t)k + t];
    __syncthreads();
    if (SYM) {
        if (t == 0) adjugate(s_M, s_A);
        __syncthreads();
    }
    const int beyond = 2 * (int)round(lam * T);
    long long d_old = 0, d_new = 0, a_old = 0, a_new = 0;
    int cnt = 0;
    for_label_members<16, long long>(labels, N, k, t, [&](int n) {
        ++cnt;
        d_old += site_cost<RISING, SYM>(s_M, s_A, x1[n], y1[n], x2[n], y2[n], T, lam, beyond);
        d_new += alt_cost[n];
        const int an = alt[n];
        for (int e = rowptr[n]; e < rowptr[n + 1]; ++e) {
            const int q = col[e];
            const int lq = labels[q];
            if (lq == k) {
                if (q < n && alt[q] != an) a_new += w[e];
            } else {
                a_old += w[e];
                if (lq != an) a_new += w[e];
            }
        }
    });
    d_old = wave_sum(d_old); d_new = wave_sum(d_new); a_old = wave_sum(a_old); a_new = wave_sum(a_new);
    if (cnt) atomicAdd(&s_cnt, cnt);
    if ((t & 63) == 0) {
        atomicAdd(&s_sum[0], (unsigned long long)d_old);
        atomicAdd(&s_sum[1], (unsigned long long)d_new);
        atomicAdd(&s_sum[2], (unsigned long long)a_old);
        atomicAdd(&s_sum[3], (unsigned long long)a_new);
    }
    __syncthreads();
    if (t != 0) return;                          // (behind the last barrier)
    if (s_cnt == 0) {
        status[c] = DROP_EMPTY;
        return;
    }
    long long* o = out + 5 * (size_t)c;
    o[0] = s_cnt;
    o[1] = (long long)s_sum[0];
    o[2] = (long long)s_sum[1];
    o[3] = (long long)potts * (long long)s_sum[2];
    o[4] = (long long)potts * (long long)s_sum[3];
    status[c] = DROP_OK;
}

hipError_t launch_best_alternative(const Points& p, const int* labels, const double* H, int Nh, const int* used, double lambda,
                                   double thr2, int* alt, int* alt_cost, int* own_cost, hipStream_t s, int rising, int symmetric)
{
    if (p.n <= 0) return hipSuccess;
    if (Nh < 0) return hipErrorInvalidValue;
    const double lam = 100.0 / lambda, T = thr2 * 81.0 / 16.0;
    auto run = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((p.n + 255) / 256), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, labels, p.n, H, Nh, used, lam, T,
                           alt, alt_cost, own_cost);
    };
    if (symmetric) { if (rising) run(k_best_alternative<true, true>); else run(k_best_alternative<false, true>); }
    else if (rising) run(k_best_alternative<true, false>);
    else run(k_best_alternative<false, false>);
    return hipGetLastError();
}

hipError_t launch_drop_labels(const Points& p, const int* labels, const double* H, const int* cand, int ncand, const int* alt,
                              const int* alt_cost, const Graph& g, double lambda, double thr2, long long* out, int* status,
                              hipStream_t s, int rising, int symmetric)
{
    if (ncand <= 0) return hipSuccess;
    if (p.n < 0) return hipErrorInvalidValue;
    const double lam = 100.0 / lambda, T = thr2 * 81.0 / 16.0;
    const int potts = (int)std::round(100.0 * lambda);
    auto run = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(ncand), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, labels, p.n, H, cand, alt, alt_cost, g.rowptr,
                           g.col, g.w, lam, T, potts, out, status);
    };
    if (symmetric) { if (rising) run(k_drop_label<true, true>); else run(k_drop_label<false, true>); }
    else if (rising) run(k_drop_label<true, false>);
    else run(k_drop_label<false, false>);
    return hipGetLastError();
}

} // namespace mh
