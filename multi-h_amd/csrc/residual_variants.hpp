// residual_variants.hpp — the measurement variants of the residual sweep (mh_set_tuning keys 0 and 1 beyond the product's
// values).  Compiled only with -DMH_TUNING (multi-h_amd/build.py --tuning) for tools/kernel_sweep.py and its kin; the
// product library carries none of this.  Included by residual.hip, inside namespace mh, behind everything of the product.
// Every variant is a named form with one member overridden per wrapper, so a row of the tables reads as what it measures.
// The numbers are referred to from DESIGN.md, HISTORY.md, profiles/ and tools/: they keep their meaning.
#pragma once

namespace tune {
template <class C, int V> struct AtPPL : C { static constexpr int PPL = V; };
template <class C, int V> struct AtMC : C { static constexpr int MC = V; };
template <class C, int V> struct Waves : C { static constexpr int MINW = V; };          // V waves per SIMD
template <class C, int V> struct StoreFlavour : C { static constexpr int SF = V; };
template <class C> struct Nt : C { static constexpr bool NT = true; };
template <class C> struct Hsgpr : C { static constexpr bool HSGPR = true; };
template <class C> struct Sym : C { static constexpr bool SYM = true; };
template <class C> struct Lean : C { static constexpr bool LEAN = true; };
template <class C> struct NoSemi : C { static constexpr bool SEMI = false; };
template <class C> struct CompilerDiv : C { static constexpr bool FAST = false; };
template <class C> struct Calib : C { static constexpr bool CALIB = true; };
template <class C> struct Contract : C { static constexpr bool CONTRACT = true; };
template <class C> struct Tiled : C { static constexpr bool TILED = true; };
struct R02Score : cfg::Base { static constexpr int PPL = 4, MC = 16; };    // the r02 kernels: the checked sweep everywhere,
struct R02 : R02Score { static constexpr bool WRITE_R = true; };           // plain stores, coefficients from LDS
using LeanR02 = Lean<R02>;
using Sweep16 = AtMC<ProductSweep, 16>;   // the product sweep at 16 (= the product of r03-r04) / 32 models per work item
using Sweep32 = AtMC<ProductSweep, 32>;
} // namespace tune
template <> constexpr bool on_resident_grid<tune::Sweep16> = true;
template <> constexpr bool on_resident_grid<tune::Sweep32> = true;

namespace tune {
static hipError_t launch_residual_variant(const Points& p, const double* H, int M, double thr2, double* R, long long ldr, int* counts,
                                          int variant, hipStream_t s, const SweepLaunch& how)
{
    auto run = [&](auto form, const SweepLaunch& o = {}) { return launch_rs<decltype(form)>(p, H, M, thr2, R, ldr, counts, nullptr, s, o); };
    auto split = [](int slices) { SweepLaunch o; o.slices = slices; return o; };     // the rows that force a point split
    if (variant == -2) return run(AtPPL<Sym<R02>, 2>{});    // symmetric mode at PPL 2 (PPL 4 measured 3 % faster)
    if (variant >= 700) return run(Calib<Nt<R02>>{}, split(variant - 700));    // 700 + psplit: store-only calibration with nt stores (the product's store instruction) and a forced point split
    if (variant >= 600) return run(Contract<R02>{}, split(variant - 600));     // 600 + psplit: fused multiply-adds (NOT bit-exact) with a forced point split
    if (variant >= 500) return run(Calib<R02>{}, split(variant - 500));        // 500 + psplit: store-only calibration (plain stores) with a forced point split
    if (variant >= 400) return run(Sweep16{}, split(variant - 400));           // 400 + psplit: the product kernel with a forced point split (tools/shard_proxy.py)
    if (variant >= 300) { SweepLaunch o = split(variant - 300); o.swapxy = 1; return run(R02{}, o); }        // 300 + s: s interleaved slices with the slice index as the fastest grid dimension
    if (variant >= 200) { SweepLaunch o = split(variant - 200); o.contiguous = true; return run(R02{}, o); } // 200 + s: s contiguous point slices instead of interleaved tiles
    if (variant >= 100) return run(R02{}, split(variant - 100));               // 100 + psplit: default kernel with a forced point split
    switch (variant) {
    // 50 / 51 / 52: the product sweep with 16 / 32 / 64 models per work item (the product: 64 since r05), resident grid and all
    case 50: return run(Sweep16{}, how);
    case 51: return run(Sweep32{}, how);
    case 52: return run(ProductSweep{}, how);
    case 1: return run(AtPPL<R02, 2>{});
    case 2: return run(Nt<R02>{});                      // nt stores
    case 3: return run(CompilerDiv<R02>{});             // compiler IEEE division
    case 4: return run(Hsgpr<R02>{});                   // coefficients in SGPRs
    case 5: return run(AtMC<R02, 8>{});
    case 6: return run(AtMC<R02, 32>{});
    case 7: return run(Calib<R02>{});                   // store-only calibration
    case 8: return run(AtPPL<R02, 8>{});
    case 9: return run(AtPPL<R02, 6>{});
    case 10: return run(Contract<R02>{});               // fused multiply-adds: NOT bit-exact
    case 20: return run(LeanR02{});                     // lean sweep on clean tiles, plain stores
    case 32: return run(R02{});                         // the r02 product kernel: checked sweep everywhere
    case 21: return run(Tiled<LeanR02>{});              // lean + tile-major R
    case 22: return run(Lean<Nt<R02>>{});               // lean + nt stores, coefficients from LDS
    case 23: return run(Tiled<R02>{});                  // tile-major R alone
    case 24: return run(Tiled<Calib<R02>>{});           // store-only calibration, tile-major R
    case 25: return run(AtPPL<LeanR02, 6>{});
    case 26: return run(AtPPL<LeanR02, 8>{});
    case 27: return run(AtPPL<LeanR02, 2>{});
    case 28: return run(StoreFlavour<LeanR02, 2>{});    // lean, sc1 stores
    case 29: return run(StoreFlavour<LeanR02, 3>{});    // lean, sc0 sc1 stores
    case 30: return run(StoreFlavour<LeanR02, 4>{});    // lean, sc1 nt stores
    case 31: return run(StoreFlavour<LeanR02, 5>{});    // lean, sc0 sc1 nt stores
    case 33: return run(Sweep16{});                     // lean + nt, coefficients through the scalar unit (= the product since r03)
    case 34: return run(NoSemi<Sweep16>{});             // as the product, but models that are not `far` take the checked sweep
    case 35: return run(Waves<Sweep16, 8>{});           // product, registers capped for 8 waves per SIMD
    case 36: return run(Waves<Sweep16, 7>{});
    case 37: return run(AtPPL<Sweep16, 6>{});
    case 38: return run(AtPPL<Sweep16, 2>{});
    case 39: return run(Sweep32{});
    case 40: return run(AtMC<ProductSweep, 8>{});
    case 41: return run(Waves<Sweep32, 7>{});
    case 42: return run(ProductSweep{});                // MC 64
    case 43: return run(AtPPL<Sweep32, 6>{});
    case 44: return run(Waves<ProductSweep, 7>{});
    case 45: return run(Sweep32{}, split(8));      // MC 32, 8 point slices
    case 46: return run(Sweep32{}, split(2));      // MC 32, 2 point slices
    case 47: return run(ProductSweep{}, split(8)); // MC 64, 8 point slices
    default: break;
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_score_variant(const Points& p, const double* H, int M, double thr2, int* counts, int variant, hipStream_t s)
{
    auto run = [&](auto form) { return launch_rs<decltype(form)>(p, H, M, thr2, nullptr, 0, counts, nullptr, s); };
    if (variant == 1) return run(AtPPL<R02Score, 2>{});
    if (variant == 32) return run(R02Score{});              // the r02 score kernel
    if (variant == 20) return run(Lean<R02Score>{});        // lean, coefficients from LDS
    if (variant == 3) return run(CompilerDiv<R02Score>{});  // compiler IEEE division
    return hipErrorInvalidValue;
}
} // namespace tune
