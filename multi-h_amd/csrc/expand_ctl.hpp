// expand_ctl.hpp — what the kernels of expand.hip (whole-graph and batch kernels, the host schedule) and of expand_solve.hip
// (the persistent solver) share: the layouts of the control words and accumulators, the kernel arguments that describe the
// moves in flight, the agent-scope accessors and the DPP row reductions.  MoveCtx, MoveBatch and SolveParams are kernel
// arguments: their byte layout is part of every kernel of the expansion.
#pragma once

#include "mh_kernels.hpp"

namespace mh {

// control words (int); the first EXPAND_HOST_WORDS are mirrored to the host
enum { C_TLAST = 0,        // index of the last accepted move, -1 before the first
       C_PEND = 1,         // alpha of an accepted move whose labels are not yet written, -1 none
       C_ERROR = 2,        // sticky: ERR_*
       C_ACCEPTED = 3,
       C_EXCESS_NODES = 4,
       C_ARRIVE = 5,       // arrivals at the first (flat) grid barrier of the running k_solve
       C_TICKET = 6,       // finished workgroups of the running k_delta
       C_FLOW_MOVES = 7,
       C_CORE = 8,         // 8 shard counters of the core list
       C_MOVES_SOLVED = 16, C_CORE_MAX = 17, C_MOVES_RUN = 18, C_XCD_USED = 19,
       C_TOOK_N = 20,      // sites in the context's took list (k_delta appends, k_commit walks; cleared by the move's first reduction launch)
       // grid barrier of k_solve, one 128-B line per XCD and one for the top level:
       //   line + 0 census (workgroups on this XCD), + 2 .. 9 four 64-bit {arrivals, changed, active} words, + 10 .. 13 four hmax words
       C_XCD = 64, C_LINE = 32, C_TOP = C_XCD + 8 * C_LINE,
       // k_delta's "last workgroup" ticket, two levels: 16 sub-tickets (one line each), then C_TICKET
       C_SUBTICKET = C_TOP + C_LINE, SUBTICKETS = 16,
       C_COUNT = EXPAND_FLAG_WORDS };
static_assert(C_SUBTICKET + SUBTICKETS * C_LINE <= C_COUNT, "control block too small");
// 64-bit accumulators
// (sums that every workgroup of a whole-graph launch contributes to are striped over STRIPES words, each on a
// 128-B line of its own, so that the adds of a launch do not queue behind ONE address: 3 000 adds to one word
// took 36 us; the reader adds the stripes up)
constexpr int STRIPES = 64, STRIPE_LL = 16;
enum { A_DELTA_S = 64, A_ENERGY_S = A_DELTA_S + STRIPES * STRIPE_LL, A_EXCESS_S = A_ENERGY_S + STRIPES * STRIPE_LL,
       A_TOTAL = A_EXCESS_S + STRIPES * STRIPE_LL };
static_assert(A_TOTAL <= EXPAND_ACC_WORDS, "accumulator block too small");
enum { A_DELTA = 0, A_ENERGY = 1, A_EXCESS_SUM = 2, A_CORE_SUM = 3, A_OUTER = 4, A_RELAX = 5, A_PUSH = 6,
       A_BARRIERS = 7, A_TICKS = 8, A_T_BAR = 9, A_T_RELAX = 10, A_T_PUSH = 11, A_T_TAIL = 12, A_TAIL_ROUNDS = 13, A_MAX_WAIT = 14, A_COUNT = 16 /* mirrored to the host */ };
enum { ERR_OVERFLOW = 1, ERR_BARRIER_TIMEOUT = 2, ERR_NO_CONVERGENCE = 3 };

// r06: the per-move state of ONE move in flight (a "context"), and a batch of them: every kernel of a move takes a MoveBatch
// and serves the context blockIdx.y selects, so K consecutive moves that are solved on the same labeling (see k_commit) cost
// the launches of one.  A move alone is a batch of one on context 0.
// The sixteen contexts are alike (ExpandWork::ctx).  Context 0 differs in meaning only: its control words are the GLOBAL ones
// (C_TLAST, C_ERROR, C_ACCEPTED and the statistics: k_batch_prep / k_batch_commit copy them to the others, k_stats_merge
// gathers the others' into them), and its words and accumulators are the ones k_publish mirrors to the host.
struct MoveCtx {
    int* cap; int* sent; int* excess; int* sink_cap; int* height; int* decided; unsigned char* took; int* core;
    int* took_list;        // the sites with took[] set, in any order (null: not kept — a move alone applies its labels lazily from took[])
    int* flags; long long* acc;
    int* saved_flow; int* saved_sink; int* trace; int* detail;
    int alpha, t, warm;
};
struct MoveBatch { MoveCtx c[EXPAND_MAX_CTX]; int count; };
// batch control words (device) and what k_commit publishes to the host
enum { B_TLAST0 = 0,       // index of the last accepted move when the batch began (what its moves' skip tests saw)
       B_SEQ = 1,
       B_TICKET = 2,       // workgroups of the running k_batch_commit that have finished
       B_BAD = 8,          // EXPAND_MAX_CTX words: bit k of word j = move k of the batch fails its test against what move j changes
       B_WORDS = 8 + EXPAND_MAX_CTX };
static_assert(EXPAND_MAX_CTX <= 32, "one bit per move of a batch");
enum { HB_FIRST_INVALID = 0, HB_TLAST = 1, HB_ERROR = 2, HB_ACCEPTED_HERE = 3, HB_DIRTY = 4, HB_SEQ = 5, HB_WORDS = 8 };

#define LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// Every launch of a move evaluates this on words that only EARLIER launches wrote.
__device__ __forceinline__ bool move_is_skipped(const int* flags, int t, int L)
{
    return flags[C_ERROR] != 0 || (t >= L && flags[C_TLAST] <= t - L);
}

// Reductions over the W = 8 or 16 consecutive lanes of a site, as DPP moves inside the VALU (quad_perm xor 1, xor 2,
// row_half_mirror, row_mirror): a butterfly through ds_bpermute costs an LDS round trip per step, and the solver's push
// cycle has four of them on its critical path.
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ long long dpp_mov64(long long v)
{
    const int lo = dpp_mov<CTRL>((int)(unsigned)((unsigned long long)v & 0xffffffffull)), hi = dpp_mov<CTRL>((int)(v >> 32));
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
template <int W>
__device__ __forceinline__ int row_min(int v)
{
    static_assert(W == 8 || W == 16, "a DPP row");
    int o = dpp_mov<DPP_XOR1>(v); v = o < v ? o : v;
    o = dpp_mov<DPP_XOR2>(v); v = o < v ? o : v;
    o = dpp_mov<DPP_HALF_MIRROR>(v); v = o < v ? o : v;
    if (W == 16) { o = dpp_mov<DPP_MIRROR>(v); v = o < v ? o : v; }
    return v;
}
template <int W>
__device__ __forceinline__ long long row_min64(long long v)
{
    static_assert(W == 8 || W == 16, "a DPP row");
    long long o = dpp_mov64<DPP_XOR1>(v); v = o < v ? o : v;
    o = dpp_mov64<DPP_XOR2>(v); v = o < v ? o : v;
    o = dpp_mov64<DPP_HALF_MIRROR>(v); v = o < v ? o : v;
    if (W == 16) { o = dpp_mov64<DPP_MIRROR>(v); v = o < v ? o : v; }
    return v;
}
template <int W>
__device__ __forceinline__ long long row_sum64(long long v)
{
    static_assert(W == 8 || W == 16, "a DPP row");
    v += dpp_mov64<DPP_XOR1>(v);
    v += dpp_mov64<DPP_XOR2>(v);
    v += dpp_mov64<DPP_HALF_MIRROR>(v);
    if (W == 16) v += dpp_mov64<DPP_MIRROR>(v);
    return v;
}
template <int W>
__device__ __forceinline__ int row_sum(int v)
{
    static_assert(W == 8 || W == 16, "a DPP row");
    v += dpp_mov<DPP_XOR1>(v);
    v += dpp_mov<DPP_XOR2>(v);
    v += dpp_mov<DPP_HALF_MIRROR>(v);
    if (W == 16) v += dpp_mov<DPP_MIRROR>(v);
    return v;
}

struct SolveParams { int reduce_rounds, relax_rounds, push_cycles, push_phases, push_mult, max_outer, cascade_iters; unsigned long long barrier_timeout, barrier_first_timeout; };

// The solver launch of an expansion (expand_solve.hip): prepare_solve sizes it once — slots per solver row for a core of all n
// sites and the dynamic LDS that holds their scalars — and launch_solve enqueues k_solve for the moves of b.
struct SolveLaunch {
    int grid = 0, mslots = 0;
    size_t lds = 0;
    bool fits = false;         // false: more sites than the per-row state in LDS holds (nothing may be launched)
};
hipError_t prepare_solve(int n, int solve_grid, SolveLaunch* sl);
void launch_solve(const SolveLaunch& sl, const Graph& g, int L, const MoveBatch& b, const SolveParams& sp, hipStream_t s);

} // namespace mh
