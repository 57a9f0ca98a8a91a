// mh_device.hpp — small __device__ helpers shared by the kernels (header-only,
// no relocatable device code needed).
#pragma once
#include <hip/hip_runtime.h>

namespace mh {

// Forward transfer error of one (point, model) pair; association order of
// M/MultiH.cpp:434-441.  Compiled with -ffp-contract=off.
__device__ __forceinline__ double fwd_d2(double h0, double h1, double h2, double h3, double h4,
                                         double h5, double h6, double h7, double h8, double x,
                                         double y, double x2, double y2)
{
    const double s = h6 * x + h7 * y + h8;
    const double u = (h0 * x + h1 * y + h2) / s;
    const double v = (h3 * x + h4 * y + h5) / s;
    const double dx = x2 - u;
    const double dy = y2 - v;
    return dx * dx + dy * dy;
}

// adj(H), H^-1 up to scale: each entry is (mul, mul, sub), every operation rounded once.
__device__ __forceinline__ void adjugate(const double* __restrict__ h, double* __restrict__ a)
{
    a[0] = h[4] * h[8] - h[5] * h[7]; a[1] = h[2] * h[7] - h[1] * h[8]; a[2] = h[1] * h[5] - h[2] * h[4];
    a[3] = h[5] * h[6] - h[3] * h[8]; a[4] = h[0] * h[8] - h[2] * h[6]; a[5] = h[2] * h[3] - h[0] * h[5];
    a[6] = h[3] * h[7] - h[4] * h[6]; a[7] = h[1] * h[6] - h[0] * h[7]; a[8] = h[0] * h[4] - h[1] * h[3];
}

// Symmetric transfer error of one (point, model) pair (include/multih_hip.h, mh_set_residual_mode): the forward error plus
// the forward error of adj(H) on the swapped pair, one final rounded addition.  What select.hip's sel_d2 spells out and the
// symmetric sweep (residual.hip) computes with adj(H) staged per workgroup.
// a = adjugate(h), for a caller that meets one model with many points.
__device__ __forceinline__ double sym_d2(const double* __restrict__ h, const double* __restrict__ a, double x, double y,
                                         double x2, double y2)
{
    const double f = fwd_d2(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], x, y, x2, y2);
    return f + fwd_d2(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], x2, y2, x, y);
}

__device__ __forceinline__ double sym_d2(const double* __restrict__ h, double x, double y, double x2, double y2)
{
    double a[9];
    adjugate(h, a);
    return sym_d2(h, a, x, y, x2, y2);
}

// The data term of one (point, model) pair from its error d2 — forward, or sym_d2 under the symmetric route — (include/multih_hip.h, mh_set_data_term): one IEEE
// division, one rounded multiplication, C round(); a NaN d2 fails `d2 < T` and takes `beyond`.  RISING = false is
// dataEnergy (M/MultiH.cpp:496-503); RISING = true drops its `1.0 -` and nothing else.
template <bool RISING>
__device__ __forceinline__ int data_term(double d2, double T, double lam, int beyond)
{
    if (RISING) return d2 < T ? (int)round(lam * (d2 / T)) : beyond;
    return d2 < T ? (int)round(lam * (1.0 - (d2 / T))) : beyond;
}

// ---------------------------------------------------------------------------
// Shared-reciprocal division for the residual sweep.
//
// hipcc lowers an IEEE f64 division n/s to
//     v_div_scale(s), v_div_scale(n), v_rcp_f64, 4 fma (two Newton steps on the reciprocal),
//     v_mul, v_fma (remainder), v_div_fmas, v_div_fixup
// The sweep needs two quotients with the SAME denominator per (point, model) pair and is
// FP64-VALU bound, so the reciprocal refinement is done once and the v_div_* helpers are
// dropped where they are provably no-ops:
//   * If s is a normal number with unbiased exponent in [-255, 256] and the numerator n is a
//     normal number with exponent in [-766, 767], v_div_scale returns both operands unscaled
//     with VCC = 0 (none of its triggers fires: exponent difference < 768, no denormal operand,
//     1/s and n/s normal, exponent(n) > 53), v_div_fmas is then a plain fma and v_div_fixup
//     passes the quotient through.  The sequence below issues exactly the remaining rounded
//     operations, so its result is bit-identical to `n / s`.
//   * n == +-0 gives +-0 on both paths (the sign of a zero quotient cannot reach d2).
// The preconditions are split so that the per-pair cost is ONE compare on s:
//   * |s| < 2^257 and |n| < 2^768, both finite     -> guaranteed by |h_i| < 2^120 for the MODEL
//                                                     (`model_pre`, once per workgroup) and
//                                                     |x|,|y| < 2^120 for the POINT (`point_pre`,
//                                                     once per tile): |s|, |n| < 3 * 2^240;
//   * |s| >= 2^-255 (and s not NaN)                -> the per-pair v_cmp_f64 with the |.| modifier;
//   * 0 < |n| < 2^-766 (incl. denormals)           -> |u| < 2^-510 on BOTH paths; x2 - u rounds to
//                                                     x2 on both unless |x2| < 2^-450, a per-POINT
//                                                     property folded into `point_pre` (which also
//                                                     rejects inf/NaN targets).
// Any lane failing a check recomputes the pair with the compiler's full IEEE division.
// ---------------------------------------------------------------------------

__device__ __forceinline__ unsigned int abs_hi(double v) { return (unsigned int)__double2hiint(v) & 0x7fffffffu; }

// |v| < 2^120 and not NaN/inf
__device__ __forceinline__ bool mag_bounded(double v) { return abs_hi(v) < ((1023u + 120u) << 20); }

// 2^-450 <= |v| < 2^120
__device__ __forceinline__ bool mag_mid(double v) { return (abs_hi(v) - ((1023u - 450u) << 20)) < (570u << 20); }

// per-point precondition: source (x, y) bounded, target (x2, y2) neither tiny nor huge
__device__ __forceinline__ bool point_pre(double x, double y, double x2, double y2)
{
    return mag_bounded(x) && mag_bounded(y) && mag_mid(x2) && mag_mid(y2);
}

// per-model precondition: all nine coefficients bounded
__device__ __forceinline__ bool model_pre(const double* h)
{
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && mag_bounded(h[i]);
    return ok;
}

// Per-model bound on s over the bounding box of ALL source points: every operation of s = (h6*x + h7*y) + h8 is
// monotone in its operands and rounding is monotone, so the s the sweep computes for any point of the box lies in
// [lo, hi] as computed here with the same operations at the box's corners.  True when that interval keeps clear of
// (-2^-255, 2^-255): the model's horizon does not come near the data.  NaN / infinite bounds compare false.
__device__ __forceinline__ bool model_far(const double* h, double xmin, double xmax, double ymin, double ymax)
{
    const double a = h[6] * xmin, b = h[6] * xmax, c = h[7] * ymin, d = h[7] * ymax;
    const double lo = (fmin(a, b) + fmin(c, d)) + h[8];
    const double hi = (fmax(a, b) + fmax(c, d)) + h[8];
    const bool finite = (a == a) && (b == b) && (c == c) && (d == d);      // fmin/fmax would hide a NaN product
    return finite && (lo >= 0x1p-255 || hi <= -0x1p-255);
}

// SCHK = false: the caller has proved |s| >= 2^-255 for every point this model can meet (model_far below), so the
// per-pair compare disappears and the fallback is taken on the per-point / per-model precondition alone.
template <bool SCHK = true>
__device__ __forceinline__ double fwd_d2_fast(double h0, double h1, double h2, double h3,
                                              double h4, double h5, double h6, double h7,
                                              double h8, double x, double y, double x2, double y2,
                                              bool pre_ok)
{
    const double s = h6 * x + h7 * y + h8;
    const double nx = h0 * x + h1 * y + h2;
    const double ny = h3 * x + h4 * y + h5;
    double r = __builtin_amdgcn_rcp(s);
    double e = __builtin_fma(-s, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-s, r, 1.0);
    r = __builtin_fma(r, e, r);
    double q = nx * r;
    double d = __builtin_fma(-s, q, nx);
    const double u = __builtin_fma(d, r, q);
    q = ny * r;
    d = __builtin_fma(-s, q, ny);
    const double v = __builtin_fma(d, r, q);
    const double dx = x2 - u;
    const double dy = y2 - v;
    double d2 = dx * dx + dy * dy;
    // bitwise, not short-circuit: two lane masks and-ed on the scalar unit, one branch
    const int ok = SCHK ? ((int)pre_ok & (int)(__builtin_fabs(s) >= 0x1p-255)) : (int)pre_ok;
    if (__builtin_expect(!ok, 0)) {
        // The empty volatile asm keeps hipcc from if-converting this branch into
        // "compute both and select", which would put the IEEE sequence back on the hot path.
        asm volatile("; fwd_d2_fast: IEEE path");
        const double ui = nx / s;
        const double vi = ny / s;
        const double dxi = x2 - ui;
        const double dyi = y2 - vi;
        d2 = dxi * dxi + dyi * dyi;
    }
    return d2;
}

// The fast path of fwd_d2_fast alone, for callers that have proved ALL its preconditions beforehand for every lane
// (model_pre and model_far for the model, point_pre for every point of the wave's tile): the same rounded operations in
// the same order, so the same bits as `/`, and nothing else.
// s_out: the denominator, for the caller's |s| >= 2^-255 test where the model is not provably `far`.
__device__ __forceinline__ double fwd_d2_lean(double h0, double h1, double h2, double h3, double h4, double h5,
                                              double h6, double h7, double h8, double x, double y, double x2, double y2,
                                              double& s_out)
{
    const double s = h6 * x + h7 * y + h8;
    s_out = s;
    const double nx = h0 * x + h1 * y + h2;
    const double ny = h3 * x + h4 * y + h5;
    double r = __builtin_amdgcn_rcp(s);
    double e = __builtin_fma(-s, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-s, r, 1.0);
    r = __builtin_fma(r, e, r);
    double q = nx * r;
    double d = __builtin_fma(-s, q, nx);
    const double u = __builtin_fma(d, r, q);
    q = ny * r;
    d = __builtin_fma(-s, q, ny);
    const double v = __builtin_fma(d, r, q);
    const double dx = x2 - u;
    const double dy = y2 - v;
    return dx * dx + dy * dy;
}

// NOT the product arithmetic: the same residual with fused multiply-adds (20 FP64 operations per
// pair instead of 28).  It rounds differently from the reference (last-bit differences in d2, and
// therefore possibly different inlier decisions within an ulp of the threshold), so it exists only
// as tuning variant 10 of the residual kernel, to measure what the exact-rounding requirement costs
// (HISTORY.md section 7).
__device__ __forceinline__ double fwd_d2_contracted(double h0, double h1, double h2, double h3, double h4,
                                                    double h5, double h6, double h7, double h8, double x,
                                                    double y, double x2, double y2)
{
    const double s = __builtin_fma(h6, x, __builtin_fma(h7, y, h8));
    const double nx = __builtin_fma(h0, x, __builtin_fma(h1, y, h2));
    const double ny = __builtin_fma(h3, x, __builtin_fma(h4, y, h5));
    double r = __builtin_amdgcn_rcp(s);
    double e = __builtin_fma(-s, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-s, r, 1.0);
    r = __builtin_fma(r, e, r);
    double q = nx * r;
    double d = __builtin_fma(-s, q, nx);
    const double u = __builtin_fma(d, r, q);
    q = ny * r;
    d = __builtin_fma(-s, q, ny);
    const double v = __builtin_fma(d, r, q);
    const double dx = x2 - u;
    const double dy = y2 - v;
    return __builtin_fma(dx, dx, dy * dy);
}

// Cyclic Jacobi eigen-solver for a small symmetric matrix (n <= 4), run by a
// single thread.  Stands where the reference calls cv::eigen on 3x3 / 4x4
// matrices (M/MultiH.cpp:459, :973).  a: n*n row-major (destroyed);
// v: eigenvectors as columns; d: eigenvalues (unsorted).
// Sweep order (p<q lexicographic), the skip of exactly-zero off-diagonals and
// the stop test (off^2 <= 1e-30 * diag^2, <= 30 sweeps) define the result bits.
__device__ inline void jacobi_sym_dev(int n, double* a, double* v, double* d)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) v[i * n + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i) {
            diag = diag + a[i * n + i] * a[i * n + i];
            for (int j = i + 1; j < n; ++j) off = off + a[i * n + j] * a[i * n + j];
        }
        if (off <= 1e-30 * diag) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
                const double sg = (theta >= 0.0) ? 1.0 : -1.0;
                const double t = sg / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = a[k * n + p], akq = a[k * n + q];
                    a[k * n + p] = c * akp - s * akq;
                    a[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = a[p * n + k], aqk = a[q * n + k];
                    a[p * n + k] = c * apk - s * aqk;
                    a[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[k * n + p], vkq = v[k * n + q];
                    v[k * n + p] = c * vkp - s * vkq;
                    v[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < n; ++i) d[i] = a[i * n + i];
}

// ---------------------------------------------------------------------------
// Pieces of GetHomography3PT without refinement (M/MultiH.cpp:995-1050) shared by the device's 3-point fits — the
// post-filter's trials (compat.hip), the 3-point proposer (propose3pt.hip) and the per-label point-only re-estimator (reestimate3pt.hip) — operation for operation the
// host's Homography3PTLinear (host/merge_step.cpp: mat3_mul, similarity_inverse, jacobi3 = jacobi_sym_dev(3), sym_eig_solve3).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void mat3_mul_dev(const double* a, const double* b, double* c)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s = s + a[3 * i + k] * b[3 * k + j];
            c[3 * i + j] = s;
        }
}

// T.inv() of the similarity T = [r 0 tx; 0 r ty; 0 0 1], computed from T (:1009, :1054)
__device__ __forceinline__ void similarity_inverse_dev(const double* T, double* Ti)
{
    const double ir = 1.0 / T[0];
    Ti[0] = ir; Ti[1] = 0; Ti[2] = -T[2] * ir; Ti[3] = 0; Ti[4] = ir; Ti[5] = -T[5] * ir; Ti[6] = 0; Ti[7] = 0; Ti[8] = 1;
}

// Fn = T2^-T F T1^-1 (:1009) and the epipole (e0, e1, 1) of Fn: the eigenvector of Fn Fn^T with the smallest eigenvalue (:1013-1017);
// T2i receives T2^-1
__device__ inline void normalised_epipolar_dev(const double* F, const double* T1, const double* T2, double* T2i, double* Fn,
                                               double& e0, double& e1)
{
    double T1i[9], T2it[9], tmp[9];
    similarity_inverse_dev(T1, T1i);
    similarity_inverse_dev(T2, T2i);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T2it[3 * i + j] = T2i[3 * j + i];
    mat3_mul_dev(T2it, F, tmp);
    mat3_mul_dev(tmp, T1i, Fn);
    double FFt[9], Fnt[9], v[9], d[3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Fnt[3 * i + j] = Fn[3 * j + i];
    mat3_mul_dev(Fn, Fnt, FFt);
    jacobi_sym_dev(3, FFt, v, d);
    int jm = 0;
    for (int j = 1; j < 3; ++j) if (d[j] < d[jm]) jm = j;
    e0 = v[0 * 3 + jm] / v[2 * 3 + jm];
    e1 = v[1 * 3 + jm] / v[2 * 3 + jm];
}

// h3 = pinv(AtA) Atb through the eigen-decomposition, eigenvalues within 2 eps sum|w| of zero dropped (sym_eig_solve3);
// AtA (3 x 3, symmetric) is destroyed
__device__ inline void sym_eig_solve3_dev(double* AtA, const double* Atb, double* h3)
{
    double v[9], w[3];
    jacobi_sym_dev(3, AtA, v, w);
    double cut = 0.0;
    for (int k = 0; k < 3; ++k) cut = cut + fabs(w[k]);
    cut = cut * (2.0 * 2.220446049250313e-16);
    h3[0] = 0.0; h3[1] = 0.0; h3[2] = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (fabs(w[k]) <= cut) continue;
        double proj = 0.0;
        for (int i = 0; i < 3; ++i) proj = proj + v[3 * i + k] * Atb[i];
        proj = proj / w[k];
        for (int i = 0; i < 3; ++i) h3[i] = h3[i] + proj * v[3 * i + k];
    }
}

// the rows of the normalised H from its third row (:1040-1050), H = T2^-1 Hn T1 (:1054); true when every entry is finite
__device__ inline bool assemble_3pt_dev(const double* h3, double e0, double e1, const double* Fn, const double* T1,
                                        const double* T2i, double* H)
{
    double Hn[9], tmp[9];
    Hn[6] = h3[0]; Hn[7] = h3[1]; Hn[8] = h3[2];
    Hn[3] = e1 * h3[0] - Fn[0]; Hn[4] = e1 * h3[1] - Fn[1]; Hn[5] = e1 * h3[2] - Fn[2];
    Hn[0] = e0 * h3[0] + Fn[3]; Hn[1] = e0 * h3[1] + Fn[4]; Hn[2] = e0 * h3[2] + Fn[5];
    mat3_mul_dev(T2i, Hn, tmp);
    mat3_mul_dev(tmp, T1, H);
    bool ok = true;
    for (int i = 0; i < 9; ++i) if (!(fabs(H[i]) <= 1.7976931348623157e308)) ok = false;      // std::isfinite
    return ok;
}

// GetHomography3PT without refinement, whole: Hartley normalisation of the three source and the three destination points
// (Homography_Refine3PTCallback.h:161-196), then the pieces above.  The post-filter's trials (compat.hip, k_compat_fit) and the
// 3-point proposer (propose3pt.hip, k_propose_3pt) call it; false when the result is not finite.
__device__ __forceinline__ void normalize3_dev(const double* pts, double* out, double* T)
{
    double cx = 0.0, cy = 0.0;
    for (int i = 0; i < 3; ++i) { cx = cx + pts[2 * i]; cy = cy + pts[2 * i + 1]; }
    const double invn = 1.0 / 3.0;
    cx = invn * cx; cy = invn * cy;
    double avg = 0.0;
    for (int i = 0; i < 3; ++i) {
        out[2 * i] = pts[2 * i] - cx;
        out[2 * i + 1] = pts[2 * i + 1] - cy;
        avg = avg + sqrt(out[2 * i] * out[2 * i] + out[2 * i + 1] * out[2 * i + 1]);
    }
    avg = avg / 3.0;
    const double ratio = sqrt(2.0) / avg;
    for (int i = 0; i < 6; ++i) out[i] = out[i] * ratio;
    T[0] = ratio; T[1] = 0; T[2] = -cx * ratio; T[3] = 0; T[4] = ratio; T[5] = -cy * ratio; T[6] = 0; T[7] = 0; T[8] = 1;
}

__device__ inline bool homography_3pt_linear_dev(const double* pts1, const double* pts2, const double* F, double* H)
{
    double p1[6], p2[6], T1[9], T2[9], T2i[9], Fn[9], e0, e1;
    normalize3_dev(pts1, p1, T1);
    normalize3_dev(pts2, p2, T2);
    normalised_epipolar_dev(F, T1, T2, T2i, Fn, e0, e1);
    double A[18], rhs[6];
    for (int i = 0; i < 3; ++i) {
        const double x1 = p1[2 * i], y1 = p1[2 * i + 1], x2 = p2[2 * i], y2 = p2[2 * i + 1];
        double* r = &A[6 * i];
        r[0] = e0 * x1 - x2 * x1; r[1] = e0 * y1 - x2 * y1; r[2] = e0 - x2;
        r[3] = e1 * x1 - y2 * x1; r[4] = e1 * y1 - y2 * y1; r[5] = e1 - y2;
        rhs[2 * i] = -(x1 * Fn[3] + y1 * Fn[4] + Fn[5]);
        rhs[2 * i + 1] = (x1 * Fn[0] + y1 * Fn[1] + Fn[2]);
    }
    double AtA[9], Atb[3];
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int i = 0; i < 6; ++i) s = s + A[3 * i + a] * A[3 * i + c];
            AtA[3 * a + c] = s;
        }
        double s = 0.0;
        for (int i = 0; i < 6; ++i) s = s + A[3 * i + a] * rhs[i];
        Atb[a] = s;
    }
    double h3[3];
    sym_eig_solve3_dev(AtA, Atb, h3);                      // x = pinv(AtA) Atb
    return assemble_3pt_dev(h3, e0, e1, Fn, T1, T2i, H);
}

struct Fund9 { double f[9]; };          // F by value to a kernel

} // namespace mh
