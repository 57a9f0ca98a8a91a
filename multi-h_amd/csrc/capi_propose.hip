// capi_propose.hip: HAF proposals — a hypothesis per affine correspondence as the engine's model set (mh_propose_haf) and the
// neighbours each of them was refitted to (mh_get_haf_support) — and 3-point proposals — a hypothesis per sampled triple and F
// (mh_propose_3pt) — part of the C ABI of include/multih_hip.h (see capi_engine.hpp for the split).  The kernels are
// csrc/haf_propose.hip and csrc/propose3pt.hip.
#include "capi_engine.hpp"

extern "C" {

int mh_propose_haf(mh_engine* e, long long first, int m, int stride, int members, double thr2)
{
    return guarded([&]() -> int {
    int rc = require_points(e);
    if (rc) return rc;
    if (m < 0 || first < 0 || stride < 1) return fail(MH_ERR_INVALID, "mh_propose_haf: m >= 0, first >= 0 and stride >= 1");
    if (members < 0 || (members > 0 && members < 3) || members > 32) return fail(MH_ERR_INVALID, "mh_propose_haf: members must be 0 or in [3, k of the sampling table]");
    if (thr2 != thr2) return fail(MH_ERR_INVALID, "mh_propose_haf: thr2 is not a number");
    if (!e->have_aff) return fail(MH_ERR_NOT_SET, "affinities are not set");
    if (!e->have_epi) return fail(MH_ERR_NOT_SET, "fundamental matrix / epipole are not set");
    if (members > 0 && e->smp_k <= 0) return fail(MH_ERR_NOT_SET, "mh_propose_haf with members > 0 needs the sampling table; call mh_build_sample_neighbours");
    if (members > e->smp_k) return fail(MH_ERR_INVALID, "mh_propose_haf: members exceeds k of the sampling table");
    // the last anchor (first + m - 1) * stride must be a correspondence: compared by division, nothing can overflow
    if (m > 0 && first + (long long)m - 1 > (long long)(e->n - 1) / stride) return fail(MH_ERR_INVALID, "mh_propose_haf: (first + m - 1) * stride must be below n");
    drop_models(e);
    if (m == 0) {                                              // an empty model set, as mh_set_models(NULL, 0) leaves one — and a HAF batch
        install_models(e, 0, BatchOrigin::HAF, false, members);
        return MH_OK;
    }
    HIPCHK(e->H.reserve((size_t)m * 9));
    HIPCHK(e->haf_used.reserve((size_t)m));
    HIPCHK(reserve_counts(e, (size_t)m + 1));
    Affines a{ e->a11.p, e->a12.p, e->a21.p, e->a22.p };
    HIPCHK(launch_haf_propose(e->pts(), a, e->epi, members > 0 ? e->smp_nbr.p : nullptr, e->smp_k, members, thr2, first, m, stride,
                              e->H.p, e->haf_used.p, e->stream));
    install_models(e, m, BatchOrigin::HAF, false, members);
    return MH_OK;
    });
}

int mh_propose_3pt(mh_engine* e, unsigned long long seed, long long first, int m)
{
    return guarded([&]() -> int {
    int rc = require_points(e);
    if (rc) return rc;
    if (m < 0 || first < 0) return fail(MH_ERR_INVALID, "mh_propose_3pt: m >= 0 and first >= 0");
    if (e->n < 3) return fail(MH_ERR_INVALID, "mh_propose_3pt: need at least 3 correspondences");
    if (!e->have_epi) return fail(MH_ERR_NOT_SET, "fundamental matrix / epipole are not set");
    if (e->sampler == MH_SAMPLER_LOCAL && e->smp_k <= 0) return fail(MH_ERR_NOT_SET, "the local sampler has no table; call mh_build_sample_neighbours");
    drop_models(e);
    if (m == 0) {                                              // (as mh_propose_haf: an empty batch is one already)
        install_models(e, 0, BatchOrigin::P3, false);
        return MH_OK;
    }
    HIPCHK(e->H.reserve((size_t)m * 9));
    HIPCHK(e->samples.reserve((size_t)m * 4));
    HIPCHK(reserve_counts(e, (size_t)m + 1));
    HIPCHK(launch_propose_3pt(e->pts(), e->epi.F, seed, first, m, e->samples.p, e->H.p, e->stream, e->dlt_local()));
    install_models(e, m, BatchOrigin::P3, true);
    return MH_OK;
    });
}

int mh_get_haf_support(mh_engine* e, unsigned* used)
{
    return guarded([&]() -> int {
    int rc = enter(e);
    if (rc) return rc;
    if (e->origin != BatchOrigin::HAF) return fail(MH_ERR_NOT_SET, "the resident model set was not proposed by mh_propose_haf");
    if (e->m <= 0) return MH_OK;
    if (!used) return fail(MH_ERR_INVALID, "null argument");
    HIPCHK(hipMemcpyAsync(used, e->haf_used.p, sizeof(unsigned) * (size_t)e->m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MH_OK;
    });
}

} // extern "C"
