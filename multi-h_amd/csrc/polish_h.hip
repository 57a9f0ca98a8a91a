// polish_h.hip — mh_polish_homographies: per label, the homography that stands is polished by Levenberg-Marquardt on the forward
// transfer error of its members, the step cv::findHomography runs behind its re-estimated winner (ten rounds there).  The
// callback (OpenCV's HomographyRefineCallback, 8 parameters, h33 = 1) is not in the reference tree; the loop is
// LMSolverImpl::run (M/Utilities.hpp:762-869), which host/merge_step.cpp restates for three parameters (lm_run3).  The
// arithmetic is the engine's definition, stated operation by operation in include/multih_hip.h and restated in
// tests/polish_h_numpy.py.
//
// One 256-thread workgroup per model (blockIdx.x = k); all iterations of a call run inside ONE launch:
//     Jacobian pass (x)    members counted; S, the 8 sums of J^T r, the 21 distinct sums of J^T J, max |r|
//     per iteration        thread 0: Ap = A + lambda D, d = pinv(Ap) v (8 x 8 cyclic Jacobi), xd = x - d
//                          candidate pass (xd): Sd alone
//                          thread 0: R, lambda (LMSolverImpl::run's two branches), accept iff Sd < S
//                          accepted: Jacobian pass (xd)
// so a call of r iterations is at most 2 r + 1 passes.  Every FP64 sum in the engine's order (wg_fit.hpp).  The loop is bounded by
// max_iterations (at most POLISH_H_MAX_ITERATIONS), Jacobi by its 30 sweeps; nothing waits for anything but the workgroup's own
// barriers, and every exit is taken by the whole workgroup.
//
// The 8 x 8 solve: jacobi_sym_dev indexes its matrices by run-time p, q.  Ap, V and W stand in the LDS reduction buffer, idle
// between two passes; A, v, D, x, xd and d are small LDS arrays: no private array with a run-time index, no scratch.

#include "mh_kernels.hpp"
#include "wg_fit.hpp"

namespace mh {

namespace {

constexpr int PH_SUMS = 30;                      // S | J^T r (8) | a a (6) | a bx (6) | a by (6) | the 2 x 2 block (3)
constexpr double PH_DEPS = 2.220446049250313e-16;
constexpr double PH_FEPS = 1.1920928955078125e-07;

// compute(x) of one member: the inverse denominator, the transferred point and the residual
struct PolishPoint { double ww, xi, yi, rx, ry; };
__device__ __forceinline__ PolishPoint polish_h_point(const double* x, double X, double Y, double u, double v)
{
    PolishPoint p;
    double ww = (x[6] * X + x[7] * Y) + 1.0;
    ww = fabs(ww) > PH_DEPS ? 1.0 / ww : 0.0;
    p.ww = ww;
    p.xi = ((x[0] * X + x[1] * Y) + x[2]) * ww;
    p.yi = ((x[3] * X + x[4] * Y) + x[5]) * ww;
    p.rx = p.xi - u;
    p.ry = p.yi - v;
    return p;
}

// out = pinv(M) b (b non-null) or the diagonal of pinv(M) (b null) for the symmetric 8 x 8 M through its eigen-decomposition,
// eigenvalues within 2 eps sum|w| of zero dropped (sym_eig_solve3's cut).  M is destroyed; V (64) and W (8) are work space.
__device__ inline void polish_h_pinv(double* M, double* V, double* W, const double* b, double* out)
{
    jacobi_sym_dev(8, M, V, W);
    double cut = 0.0;
    for (int k = 0; k < 8; ++k) cut = cut + fabs(W[k]);
    cut = cut * (2.0 * PH_DEPS);
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    for (int k = 0; k < 8; ++k) {
        const double w = W[k];
        if (fabs(w) <= cut) continue;
        if (b) {
            double proj = 0.0;
            for (int i = 0; i < 8; ++i) proj = proj + V[8 * i + k] * b[i];
            proj = proj / w;
            for (int i = 0; i < 8; ++i) out[i] = out[i] + proj * V[8 * i + k];
        } else {
            for (int i = 0; i < 8; ++i) out[i] = out[i] + V[8 * i + k] * V[8 * i + k] / w;
        }
    }
}

// The Jacobian pass at x (8 doubles in LDS): members counted, the 30 sums into G, max |r| into *maxr.  Every thread calls it;
// it ends on a barrier, after which the reduction buffer is idle.  Returns the member count.
__device__ __forceinline__ int polish_h_jacobian_pass(const double* __restrict__ x1, const double* __restrict__ y1,
                                                      const double* __restrict__ x2, const double* __restrict__ y2, int N,
                                                      const int* __restrict__ labels, int k, const double* xs,
                                                      double (*sv)[PH_SUMS], double* G, double* maxr, int t)
{
    double x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = xs[j];
    double acc[PH_SUMS];
#pragma unroll
    for (int q = 0; q < PH_SUMS; ++q) acc[q] = 0.0;
    double mr = 0.0;
    int cnt = 0;
    for (int n = t; n < N; n += 256) {
        if (labels[n] != k) continue;
        ++cnt;
        const double X = x1[n], Y = y1[n];
        const PolishPoint p = polish_h_point(x, X, Y, x2[n], y2[n]);
        const double a[3] = { X * p.ww, Y * p.ww, p.ww };
        const double bx[2] = { -(a[0] * p.xi), -(a[1] * p.xi) };
        const double by[2] = { -(a[0] * p.yi), -(a[1] * p.yi) };
        acc[0] = acc[0] + (p.rx * p.rx + p.ry * p.ry);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            acc[1 + i] = acc[1 + i] + a[i] * p.rx;
            acc[4 + i] = acc[4 + i] + a[i] * p.ry;
        }
        acc[7] = acc[7] + (bx[0] * p.rx + by[0] * p.ry);
        acc[8] = acc[8] + (bx[1] * p.rx + by[1] * p.ry);
        acc[9] = acc[9] + a[0] * a[0];   acc[10] = acc[10] + a[0] * a[1]; acc[11] = acc[11] + a[0] * a[2];
        acc[12] = acc[12] + a[1] * a[1]; acc[13] = acc[13] + a[1] * a[2]; acc[14] = acc[14] + a[2] * a[2];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[15 + 2 * i + j] = acc[15 + 2 * i + j] + a[i] * bx[j];
                acc[21 + 2 * i + j] = acc[21 + 2 * i + j] + a[i] * by[j];
            }
        acc[27] = acc[27] + (bx[0] * bx[0] + by[0] * by[0]);
        acc[28] = acc[28] + (bx[0] * bx[1] + by[0] * by[1]);
        acc[29] = acc[29] + (bx[1] * bx[1] + by[1] * by[1]);
        const double ax = fabs(p.rx), ay = fabs(p.ry);
        if (ax > mr) mr = ax;
        if (ay > mr) mr = ay;
    }
    // max |r| and the count first, in two columns of the buffer (a count is exact as a double; a max, so not wg_tree), then the 30 sums
    sv[t][0] = mr;
    sv[t][1] = (double)cnt;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) {
            if (sv[t + s][0] > sv[t][0]) sv[t][0] = sv[t + s][0];
            sv[t][1] = sv[t][1] + sv[t + s][1];
        }
        __syncthreads();
    }
    if (t == 0) *maxr = sv[0][0];
    const int members = (int)sv[0][1];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PH_SUMS; ++q) sv[t][q] = acc[q];
    wg_tree<PH_SUMS>(sv, t);
    if (t < PH_SUMS) G[t] = sv[0][t];
    __syncthreads();
    return members;
}

// A = J^T J (8 x 8, symmetric) and v = J^T r from the 30 sums; one thread
__device__ inline void polish_h_normal_equations(const double* G, double* A, double* v)
{
    for (int i = 0; i < 64; ++i) A[i] = 0.0;
    int q = 9;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double g = G[q++];
            A[8 * i + j] = g; A[8 * j + i] = g;
            A[8 * (3 + i) + 3 + j] = g; A[8 * (3 + j) + 3 + i] = g;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 2; ++j) {
            const double gx = G[15 + 2 * i + j], gy = G[21 + 2 * i + j];
            A[8 * i + 6 + j] = gx; A[8 * (6 + j) + i] = gx;
            A[8 * (3 + i) + 6 + j] = gy; A[8 * (6 + j) + 3 + i] = gy;
        }
    A[8 * 6 + 6] = G[27]; A[8 * 6 + 7] = G[28]; A[8 * 7 + 6] = G[28]; A[8 * 7 + 7] = G[29];
    for (int i = 0; i < 8; ++i) v[i] = G[1 + i];
}

} // namespace

// One workgroup per model k = blockIdx.x.  H_in, H_out: m x 9; cost: m x 2; info: m x 4 (members, iterations run, steps
// accepted, status).  max_iterations in [0, POLISH_H_MAX_ITERATIONS].
__global__ void __launch_bounds__(256)
k_polish_h(const double* __restrict__ x1, const double* __restrict__ y1,
           const double* __restrict__ x2, const double* __restrict__ y2, int N, const int* __restrict__ labels,
           const double* __restrict__ H_in, int max_iterations, double* __restrict__ H_out,
           double* __restrict__ cost, int* __restrict__ info)
{
    const int t = threadIdx.x;
    const int k = blockIdx.x;
    __shared__ double sv[256][PH_SUMS];          // 60 KB: the partial sums; between two passes Ap (64), V (64), W (8) of the solve
    __shared__ double s_G[PH_SUMS];
    __shared__ double s_A[64], s_v[8], s_D[8];
    __shared__ double s_x[8], s_xd[8], s_d[8], s_tmp[8];
    __shared__ double s_Sd, s_maxr;
    __shared__ int s_accept, s_stop;

    H_in += 9 * (size_t)k; H_out += 9 * (size_t)k; cost += 2 * (size_t)k; info += 4 * (size_t)k;
    if (t < 8) s_x[t] = H_in[t] / H_in[8];
    __syncthreads();
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) finite = finite && finite_dev(s_x[j]);

    const int members = polish_h_jacobian_pass(x1, y1, x2, y2, N, labels, k, s_x, sv, s_G, &s_maxr, t);
    const int status = members < 4 ? 1 : (!finite ? 2 : 0);

    // thread 0's loop state (the other threads follow s_accept and s_stop)
    double S = s_G[0], lambda = 1.0, lc = 0.75;
    const double S0 = S;
    int iter = 0, accepted = 0;

    if (status == 0 && max_iterations > 0) {     // (the same for every thread, like every break below)
        if (t == 0) {
            polish_h_normal_equations(s_G, s_A, s_v);
            for (int i = 0; i < 8; ++i) s_D[i] = s_A[9 * i];                 // D = diag(A), once
        }
        for (;;) {                               // LMSolverImpl::run's loop: at most max_iterations <= 32 trips
            if (t == 0) {
                double* Ap = &sv[0][0];
                double* V = Ap + 64;
                double* W = V + 64;
                for (int i = 0; i < 64; ++i) Ap[i] = s_A[i];
                for (int i = 0; i < 8; ++i) Ap[9 * i] = s_A[9 * i] + lambda * s_D[i];
                polish_h_pinv(Ap, V, W, s_v, s_d);
                for (int i = 0; i < 8; ++i) s_xd[i] = s_x[i] - s_d[i];
            }
            __syncthreads();
            // candidate pass: Sd
            {
                double x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = s_xd[j];
                double a0 = 0.0;
                for (int n = t; n < N; n += 256) {
                    if (labels[n] != k) continue;
                    const PolishPoint p = polish_h_point(x, x1[n], y1[n], x2[n], y2[n]);
                    a0 = a0 + (p.rx * p.rx + p.ry * p.ry);
                }
                sv[t][0] = a0;
                wg_tree<1>(sv, t);
                if (t == 0) s_Sd = sv[0][0];
                __syncthreads();                 // the reduction buffer is idle again
            }
            if (t == 0) {
                const double Sd = s_Sd;
                for (int i = 0; i < 8; ++i) {
                    double s = 0.0;
                    for (int j = 0; j < 8; ++j) s = s + s_A[8 * i + j] * s_d[j];
                    s_tmp[i] = -s + 2.0 * s_v[i];                            // gemm(A, d, -1, v, 2, temp_d), :809
                }
                double dS = 0.0;
                for (int i = 0; i < 8; ++i) dS = dS + s_d[i] * s_tmp[i];
                const double R = (S - Sd) / (fabs(dS) > PH_DEPS ? dS : 1.0);
                if (R > 0.75) {
                    lambda = lambda * 0.5;
                    if (lambda < lc) lambda = 0.0;
                } else if (R < 0.25) {
                    double tt = 0.0;
                    for (int i = 0; i < 8; ++i) tt = tt + s_d[i] * s_v[i];
                    double nu = (Sd - S) / (fabs(tt) > PH_DEPS ? tt : 1.0) + 2.0;
                    nu = nu < 2.0 ? 2.0 : nu;
                    nu = nu > 10.0 ? 10.0 : nu;
                    if (lambda == 0.0) {
                        double* Ap = &sv[0][0];
                        double* V = Ap + 64;
                        double* W = V + 64;
                        for (int i = 0; i < 64; ++i) Ap[i] = s_A[i];
                        polish_h_pinv(Ap, V, W, nullptr, s_tmp);             // invert(A, Ap, DECOMP_EIG), :827: its diagonal
                        double maxval = PH_DEPS;
                        for (int i = 0; i < 8; ++i) { const double a = fabs(s_tmp[i]); if (a > maxval) maxval = a; }
                        lambda = lc = 1.0 / maxval;
                        nu = nu * 0.5;
                    }
                    lambda = lambda * nu;
                }
                const bool accept = Sd < S;
                if (accept) {
                    S = Sd; ++accepted;
                    for (int i = 0; i < 8; ++i) s_x[i] = s_xd[i];
                }
                ++iter;
                double maxd = 0.0;
                bool dfin = true;
                for (int i = 0; i < 8; ++i) {
                    const double a = fabs(s_d[i]);
                    if (a > maxd) maxd = a;
                    dfin = dfin && finite_dev(s_d[i]);
                }
                s_accept = accept ? 1 : 0;
                s_stop = (iter >= max_iterations || maxd < PH_FEPS || !dfin) ? 1 : 0;
            }
            __syncthreads();
            if (s_stop) break;                   // (an accepted step's A, v and r are not needed any more)
            if (s_accept) {
                polish_h_jacobian_pass(x1, y1, x2, y2, N, labels, k, s_xd, sv, s_G, &s_maxr, t);
                if (t == 0) polish_h_normal_equations(s_G, s_A, s_v);
            }
            if (s_maxr < PH_FEPS) break;         // max |r| of the x that stands
        }
    }

    if (t == 0) {
        const bool moved = status == 0 && accepted > 0;
        for (int j = 0; j < 9; ++j) H_out[j] = moved ? (j < 8 ? s_x[j] : 1.0) : H_in[j];
        cost[0] = status == 0 ? S0 : 0.0;
        cost[1] = status == 0 ? S : 0.0;
        info[0] = members; info[1] = iter; info[2] = accepted; info[3] = status;
    }
}

hipError_t launch_polish_h(const Points& p, const int* labels, const double* H_in, int m, int max_iterations, double* H_out,
                           double* cost, int* info, hipStream_t s)
{
    if (p.n <= 0 || m < 1 || m > POLISH_H_MAX_MODELS || max_iterations < 0 || max_iterations > POLISH_H_MAX_ITERATIONS || !labels)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_polish_h, dim3(m), dim3(256), 0, s, p.x1, p.y1, p.x2, p.y2, p.n, labels, H_in, max_iterations, H_out,
                       cost, info);
    return hipGetLastError();
}

} // namespace mh
