// graph.hip — the symmetric weighted neighbourhood graph, built on the device from a directed hit list.
//
// setNeighbors semantics (GCoptimization.cpp:1656-1681, M/MultiH.cpp:532-540): every directed hit i->j (j != i)
// appends j to i's list and i to j's list, so the weight of the pair is mult(i,j) = #[i->j] + #[j->i] (SURVEY A-2).
// Output: CSR with sorted rows, one entry per distinct neighbour, its multiplicity, and the index of the reverse
// arc — the persistent structure the alpha-expansion kernels run on (expand.hip).
//
//   k_hits_filter   (k-NN path) drops the hits beyond the reference's radius, in float32 like FLANN's L2
//   k_sym_count     degree of every site: own hits + hits received (atomics), index validation
//   k_scan          exclusive prefix sum (one workgroup; n is the number of sites)
//   k_sym_scatter   raw rows: every hit lands in the rows of both its ends
//   k_sym_fold      one wavefront per row: rank sort in LDS, duplicates folded into (column, multiplicity)
//   k_scan          final row pointers
//   k_sym_compact   rows to their final place
//   k_sym_rev       reverse-arc index by binary search in the neighbour's (sorted) row
//   k_row_wsum      per-site weight totals of the multiplicities (MH_SMOOTH_UNIFORM), or
//   k_arc_weights   multiplicity x distance weight per arc and the totals of those (MH_SMOOTH_CAUCHY)
//
// Entries land in a raw row in any order and are sorted there, so the result is deterministic.  The input is either
// a CSR (rowptr != null) or a dense n x stride table (k-NN output); a column of -1 is "no hit".
// 50k points / 0.8 M hits: the neighbourhood build fell from 50 ms to 9.8 ms (8.4 ms of it the k-NN kernel) when this replaced the host construction.

#include "mh_kernels.hpp"

namespace mh {

constexpr int GL = 16;                 // lanes per row in the hit-walking kernels

__device__ __forceinline__ void hit_range(const int* rowptr, int stride, int i, int& b, int& e)
{
    if (rowptr) { b = rowptr[i]; e = rowptr[i + 1]; }
    else { b = i * stride; e = b + stride; }
}

// the reference's radius (M/MultiH.cpp:252-253) in the k-NN kernel's float32 arithmetic: ((dx^2+dy^2)+dz^2)+dw^2 <= r^2
__global__ void __launch_bounds__(256)
k_hits_filter(Points p, int stride, float r2, int* __restrict__ col, int* __restrict__ err)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.n * stride) return;
    const int i = (int)(t / stride);
    const int c = col[t];
    if (c < 0 || c >= p.n) { atomicExch(err, 1); col[t] = -1; return; }
    const float dx = (float)p.x1[i] - (float)p.x1[c], dy = (float)p.y1[i] - (float)p.y1[c];
    const float dz = (float)p.x2[i] - (float)p.x2[c], dw = (float)p.y2[i] - (float)p.y2[c];
    const float d = ((dx * dx + dy * dy) + dz * dz) + dw * dw;
    if (!(d <= r2)) col[t] = -1;
}

__global__ void __launch_bounds__(256)
k_sym_count(int n, const int* __restrict__ rowptr, int stride, const int* __restrict__ col, int* __restrict__ deg,
            int* __restrict__ err)
{
    const int i = blockIdx.x * (256 / GL) + threadIdx.x / GL;
    const int sub = threadIdx.x % GL;
    if (i >= n) return;
    int b, e;
    hit_range(rowptr, stride, i, b, e);
    if (e < b) { if (sub == 0) atomicExch(err, 2); return; }
    int mine = 0;
    for (int k = b + sub; k < e; k += GL) {
        const int j = col[k];
        if (j == -1 || j == i) continue;
        if (j < 0 || j >= n) { atomicExch(err, 1); continue; }
        ++mine;
        atomicAdd(&deg[j], 1);
    }
#pragma unroll
    for (int m = GL / 2; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, GL);
    if (sub == 0 && mine) atomicAdd(&deg[i], mine);
}

// out[0..n] = exclusive prefix sums of in[0..n) (out[n] = total); info[0] = 1 if the total exceeds int32, info[1] = max in[]
__global__ void __launch_bounds__(1024)
k_scan(const int* __restrict__ in, int* __restrict__ out, int n, int* __restrict__ info)
{
    __shared__ long long s_part[16];
    __shared__ long long s_base;
    __shared__ int s_max[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_base = 0;
    int vmax = 0;
    __syncthreads();
    for (int b = 0; b < n; b += 1024) {
        const int i = b + threadIdx.x;
        const int v = i < n ? in[i] : 0;
        vmax = v > vmax ? v : vmax;
        long long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const long long y = __shfl_up(incl, o, 64); if (lane >= o) incl += y; }
        if (lane == 63) s_part[wave] = incl;
        __syncthreads();
        long long before = s_base;
        for (int w = 0; w < wave; ++w) before += s_part[w];
        if (i < n) {
            const long long ex = before + incl - v;
            out[i] = ex > 0x7fffffffll ? 0x7fffffff : (int)ex;
        }
        __syncthreads();
        if (threadIdx.x == 1023) s_base = before + incl;
        __syncthreads();
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(vmax, m, 64); vmax = o > vmax ? o : vmax; }
    if (lane == 0) s_max[wave] = vmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = 0;
        for (int w = 0; w < 16; ++w) m = s_max[w] > m ? s_max[w] : m;
        out[n] = s_base > 0x7fffffffll ? 0x7fffffff : (int)s_base;
        info[0] = s_base > 0x7fffffffll ? 1 : 0;
        info[1] = m;
    }
}

__global__ void __launch_bounds__(256)
k_sym_scatter(int n, const int* __restrict__ rowptr, int stride, const int* __restrict__ col,
              const int* __restrict__ start, int* __restrict__ cursor, int* __restrict__ raw)
{
    const int i = blockIdx.x * (256 / GL) + threadIdx.x / GL;
    const int sub = threadIdx.x % GL;
    if (i >= n) return;
    int b, e;
    hit_range(rowptr, stride, i, b, e);
    for (int k = b + sub; k < e; k += GL) {
        const int j = col[k];
        if (j < 0 || j >= n || j == i) continue;
        raw[start[i] + atomicAdd(&cursor[i], 1)] = j;
        raw[start[j] + atomicAdd(&cursor[j], 1)] = i;
    }
}

// One wavefront per row (rows of at most SYM_MAX_ROW entries): rank sort, then runs of equal columns become one entry.
// raw[start[i] ..] receives the distinct columns in ascending order, mult[..] their multiplicities, uniq[i] their number.
__global__ void __launch_bounds__(256)
k_sym_fold(int n, const int* __restrict__ start, int* __restrict__ raw, int* __restrict__ mult, int* __restrict__ uniq)
{
    __shared__ int s_in[4][SYM_MAX_ROW];
    __shared__ int s_out[4][SYM_MAX_ROW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (i >= n) return;
    const int b = start[i], d = start[i + 1] - b;
    int* in = s_in[wave];
    int* out = s_out[wave];
    for (int t = lane; t < d; t += 64) in[t] = raw[b + t];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int t = lane; t < d; t += 64) {
        const int v = in[t];
        int rank = 0;
        for (int x = 0; x < d; ++x) {
            const int y = in[x];
            rank += (y < v || (y == v && x < t)) ? 1 : 0;
        }
        out[rank] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int heads_before = 0;
    for (int c = 0; c < d; c += 64) {
        const int p = c + lane;
        const bool head = p < d && (p == 0 || out[p - 1] != out[p]);
        const unsigned long long m = __ballot(head);
        if (head) {
            int len = 1;
            while (p + len < d && out[p + len] == out[p]) ++len;
            const int pos = heads_before + __popcll(m & ((1ull << lane) - 1ull));
            raw[b + pos] = out[p];
            mult[b + pos] = len;
        }
        heads_before += __popcll(m);
    }
    if (lane == 0) uniq[i] = heads_before;
}

__global__ void __launch_bounds__(256)
k_sym_compact(int n, const int* __restrict__ start, const int* __restrict__ raw, const int* __restrict__ mult,
              const int* __restrict__ rowptr, int* __restrict__ col, int* __restrict__ w)
{
    const int i = blockIdx.x * (256 / GL) + threadIdx.x / GL;
    const int sub = threadIdx.x % GL;
    if (i >= n) return;
    const int src = start[i], dst = rowptr[i], len = rowptr[i + 1] - dst;
    for (int t = sub; t < len; t += GL) { col[dst + t] = raw[src + t]; w[dst + t] = mult[src + t]; }
}

__global__ void __launch_bounds__(256)
k_sym_rev(int n, const int* __restrict__ rowptr, const int* __restrict__ col, int* __restrict__ rev)
{
    const int i = blockIdx.x * (256 / GL) + threadIdx.x / GL;
    const int sub = threadIdx.x % GL;
    if (i >= n) return;
    for (int k = rowptr[i] + sub; k < rowptr[i + 1]; k += GL) {
        const int j = col[k];
        int lo = rowptr[j], hi = rowptr[j + 1];          // lower bound of i in row j (present by construction)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (col[mid] < i) lo = mid + 1; else hi = mid;
        }
        rev[k] = lo;
    }
}

__global__ void __launch_bounds__(256)
k_row_wsum(int n, const int* __restrict__ rowptr, const int* __restrict__ w, int* __restrict__ wsum)
{
    const int i = blockIdx.x * (256 / GL) + threadIdx.x / GL;
    const int sub = threadIdx.x % GL;
    if (i >= n) return;
    long long t = 0;
    for (int k = rowptr[i] + sub; k < rowptr[i + 1]; k += GL) t += w[k];
#pragma unroll
    for (int m = GL / 2; m >= 1; m >>= 1) t += __shfl_xor(t, m, GL);
    if (sub == 0) wsum[i] = t > 0x7fffffffll ? 0x7fffffff : (int)t;
}

// MH_SMOOTH_CAUCHY (include/multih_hip.h, mh_set_smoothness_weights): w[k] = mult[k] * q(d), d the float32 squared distance of
// the arc's two sites in k_hits_filter's arithmetic, q = max(1, round(q_max * r2 / (r2 + d))) in double.  Sixteen lanes walk a
// row as in the kernels above: the site's own coordinates are read once per lane, the partner's four are gathered (rows are
// sorted by column, and k-NN partners lie close in the arrays only by accident: these are the pass's scattered reads, 32 B an
// arc, nothing is staged in LDS).  The same pass folds the row's int64 sum into wsum, so it takes k_row_wsum's place under
// this rule.  *overflow is raised when a product or a row sum leaves int32 (the stored value is then clamped and the caller
// throws the buffers away).  d infinite gives t = 0, d NaN gives a NaN qf: both fail `qf >= 1.0` and take q = 1.
__global__ void __launch_bounds__(256)
k_arc_weights(Points p, const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ mult,
              double r2, int q_max, int* __restrict__ w, int* __restrict__ wsum, int* __restrict__ overflow)
{
    const int i = blockIdx.x * (256 / GL) + threadIdx.x / GL;
    const int sub = threadIdx.x % GL;
    if (i >= p.n) return;
    const float xi = (float)p.x1[i], yi = (float)p.y1[i], zi = (float)p.x2[i], wi = (float)p.y2[i];
    long long t = 0;
    bool over = false;
    for (int k = rowptr[i] + sub; k < rowptr[i + 1]; k += GL) {
        const int j = col[k];
        const float dx = xi - (float)p.x1[j], dy = yi - (float)p.y1[j];
        const float dz = zi - (float)p.x2[j], dw = wi - (float)p.y2[j];
        const float d = ((dx * dx + dy * dy) + dz * dz) + dw * dw;
        const double qf = (double)q_max * (r2 / (r2 + (double)d));
        const int q = qf >= 1.0 ? (int)round(qf) : 1;
        const long long prod = (long long)mult[k] * q;
        over = over || prod > 0x7fffffffll;
        w[k] = prod > 0x7fffffffll ? 0x7fffffff : (int)prod;
        t += prod;
    }
#pragma unroll
    for (int m = GL / 2; m >= 1; m >>= 1) t += __shfl_xor(t, m, GL);
    over = over || t > 0x7fffffffll;
    if (over) atomicExch(overflow, 1);
    if (sub == 0) wsum[i] = t > 0x7fffffffll ? 0x7fffffff : (int)t;
}

hipError_t launch_row_weight_sums(int n, const int* rowptr, const int* w, int* wsum, hipStream_t s)
{
    hipLaunchKernelGGL(k_row_wsum, dim3((n + 256 / GL - 1) / (256 / GL)), dim3(256), 0, s, n, rowptr, w, wsum);
    return hipGetLastError();
}

// *overflow must have been cleared on the stream
hipError_t launch_arc_weights(const Points& p, const int* rowptr, const int* col, const int* mult, double r2, int q_max, int* w,
                              int* wsum, int* overflow, hipStream_t s)
{
    hipLaunchKernelGGL(k_arc_weights, dim3((p.n + 256 / GL - 1) / (256 / GL)), dim3(256), 0, s, p, rowptr, col, mult, r2, q_max,
                       w, wsum, overflow);
    return hipGetLastError();
}

hipError_t launch_hits_filter(const Points& p, int stride, float r2, int* col, int* err, hipStream_t s)
{
    const long long total = (long long)p.n * stride;
    hipLaunchKernelGGL(k_hits_filter, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, stride, r2, col, err);
    return hipGetLastError();
}

hipError_t launch_sym_count(int n, const int* rowptr, int stride, const int* col, int* deg, int* start, int* info, hipStream_t s)
{
    const dim3 grid((n + 256 / GL - 1) / (256 / GL));
    hipError_t he = hipMemsetAsync(deg, 0, sizeof(int) * (size_t)n, s);
    if (he != hipSuccess) return he;
    hipLaunchKernelGGL(k_sym_count, grid, dim3(256), 0, s, n, rowptr, stride, col, deg, info + 2);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, deg, start, n, info);
    return hipGetLastError();
}

hipError_t launch_sym_build(int n, const int* rowptr, int stride, const int* col, const int* start, int* cursor, int* raw,
                            int* mult, int* uniq, int* out_rowptr, int* info, hipStream_t s)
{
    const dim3 grid((n + 256 / GL - 1) / (256 / GL));
    hipError_t he = hipMemsetAsync(cursor, 0, sizeof(int) * (size_t)n, s);
    if (he != hipSuccess) return he;
    hipLaunchKernelGGL(k_sym_scatter, grid, dim3(256), 0, s, n, rowptr, stride, col, start, cursor, raw);
    hipLaunchKernelGGL(k_sym_fold, dim3((n + 3) / 4), dim3(256), 0, s, n, start, raw, mult, uniq);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, uniq, out_rowptr, n, info + 4);
    return hipGetLastError();
}

hipError_t launch_sym_finish(int n, const int* start, const int* raw, const int* mult, const int* rowptr, int* col, int* w,
                             int* rev, hipStream_t s)
{
    const dim3 grid((n + 256 / GL - 1) / (256 / GL));
    hipLaunchKernelGGL(k_sym_compact, grid, dim3(256), 0, s, n, start, raw, mult, rowptr, col, w);
    hipLaunchKernelGGL(k_sym_rev, grid, dim3(256), 0, s, n, rowptr, col, rev);
    return hipGetLastError();
}

} // namespace mh
