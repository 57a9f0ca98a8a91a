// expand.hip — alpha-expansion relabel sweep on gfx950.
//
// Replaces GCoptimization::expansion's standard-cycle branch
// (GCoptimization.cpp:1032-1049), oneExpansionIteration (:1278-1289) and
// alpha_expansion (:1212-1274) together with the Energy/Graph/BK max-flow
// stack underneath (energy.h:204-253,324-328; maxflow.cpp:472-604;
// graph.h:478-488).  Energies are int32 like the reference's
// (GCoptimization.h:166-170); totals are accumulated in int64 and checked.
//
// The whole sweep is driven from the device: the host enqueues the launches of a move, or of a batch of
// moves solved together (see CONCURRENT ALPHA-MOVES below), and looks at the control words once per batch
// and once per cycle (the energy test of :1045).  How many launches that is: see Launcher below.
//
// Three files: this one holds the whole-graph and batch kernels and the host schedule (run_expansion);
// expand_solve.hip the persistent solver k_solve with its grid barrier; expand_ctl.hpp what both sides
// share.  Which moves run together is decided by expand_plan.hpp, host arithmetic alone.
//
// Per move (label alpha, fixed order 0..L-1, :1285-1286; t = running move index):
//   k_move_setup   applies the previous accepted move (labels are updated lazily, see below), then
//                  builds the binary energy's s-t graph on the PERSISTENT symmetric CSR (only
//                  capacities change per move):
//                    t-links  : add_term1(i, E0=cost(i,alpha), E1=cost(i,cur))   (:336-342)
//                               + Potts terms against neighbours already at alpha (:360-362)
//                               + the D part of add_term2 for j<i with different labels (energy.h:220)
//                    n-links  : for active pair i>j: cap(i->j)=w*potts,
//                               cap(j->i)= (l_i==l_j) ? w*potts : 0              (energy.h:221-252)
//                  turns t-links into excess / sink capacity (Graph::add_tweights keeps only the
//                  difference) and takes the first dominance verdict from the site's own numbers.
//   k_reduce       dominance reduction (exact; a second launch in front of it is a schedule option): a site whose net source surplus exceeds the total
//                  capacity of its outgoing n-links is on the source side of EVERY minimum cut; one
//                  whose net sink surplus exceeds its incoming capacity can always reach the sink.
//                  Such sites are decided, their n-links are folded into the neighbours' t-links,
//                  and the test cascades.  At 50k sites / 11 labels it settles 70-95 % of the sites
//                  of a move before any flow is pushed.  The second launch appends the sites that
//                  are still undecided to a compact list (the "core": points that are inliers of
//                  both the current and the candidate plane, a few thousand sites).
//   k_solve        (expand_solve.hip) ONE persistent launch over the core only (8 lanes per site, arcs in registers,
//                  phases separated by a grid barrier): finishes the reduction cascade, then
//                  alternates exact global relabelling (chaotic min-relaxation from the sink to a
//                  fixed point) with lock-free preflow pushes (agent-scope atomics on excess and
//                  residual capacities, heights written only by their owner) until, right after a
//                  global relabel, no site with positive excess can still reach the sink.
//                  Cut read-out: the sites that cannot reach the sink in the residual graph are the
//                  SOURCE side and take alpha (var 0, :429-433).  This is BK's what_segment rule
//                  (free nodes default to SOURCE, graph.h:478-488) = the unique minimal sink side of
//                  any maximum (pre)flow, so labels are solver-independent (SURVEY A-1).
//   k_delta        int64 energy difference of the candidate labeling; the last workgroup to finish
//                  accepts the move iff the energy strictly decreases (:1259,1273) and records it in
//                  the control words.  The labels themselves are rewritten by the NEXT launch that
//                  walks the sites (the next k_move_setup, or k_apply_pending at the end of a cycle).
//
// Idempotent moves are skipped on the device: the expansion on alpha of a labeling that has not
// changed since the previous expansion on alpha completed cannot lower the energy (every expansion
// of f' = move_alpha(f) is an expansion of f, and f' was the minimum over those), so the reference
// rejects it (:1259) and leaves the labels untouched.  Every launch of such a move returns at once.
// The last cycle of every expansion (the one that confirms convergence) consists of such moves.
//
// A cycle ends with k_energy; the loop stops when the energy is unchanged (:1045).
//
// Roofline: irregular, latency/atomic bound (no dense tile anywhere); reported as time per
// LabelingStep, launches and grid barriers, not as a bandwidth fraction.

#include "expand_ctl.hpp"
#include "expand_plan.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>

namespace mh {

__global__ void k_ctl_init(MoveBatch b)                 // one workgroup per context
{
    int* flags = b.c[blockIdx.x].flags;
    long long* acc = b.c[blockIdx.x].acc;
    for (int t = threadIdx.x; t < C_COUNT; t += blockDim.x) flags[t] = (t == C_TLAST || t == C_PEND) ? -1 : 0;
    for (int t = threadIdx.x; t < A_TOTAL; t += blockDim.x) acc[t] = 0;
}

__global__ void __launch_bounds__(256)
k_init_labeling(const int* __restrict__ cost, int L, int n, const int* __restrict__ init,
                int* __restrict__ label, int* __restrict__ cur_cost)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = init ? init[i] : 0;
    label[i] = l;
    cur_cost[i] = cost[(size_t)i * L + l];        // updateLabelingDataCosts, :445-451
}

// solveSpecialCases (:470-491): no neighbours at all -> per-site argmin, first minimum wins.
__global__ void __launch_bounds__(256)
k_argmin_labels(const int* __restrict__ cost, int L, int n, int* __restrict__ label,
                long long* __restrict__ acc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    long long mine = 0;
    if (i < n) {
        int best = 0, bc = cost[(size_t)i * L];
        for (int l = 1; l < L; ++l) {
            const int c = cost[(size_t)i * L + l];
            if (c < bc) { bc = c; best = l; }
        }
        label[i] = best;
        mine = bc;
    }
    __shared__ long long s[256];
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        atomicAdd((unsigned long long*)&acc[A_ENERGY_S + (blockIdx.x % STRIPES) * STRIPE_LL], (unsigned long long)s[0]);
}

// ---------------------------------------------------------------------------
// Whole-graph kernels.  A site's arcs are contiguous in the CSR, so LPN = 16 consecutive lanes
// (one DPP row; four sites per wavefront) scan them together: coalesced 64-B reads of col/cap and
// width-16 shuffles for the reductions.  All lanes of a site keep identical copies of the site's
// scalars; lane 0 alone writes.
// ---------------------------------------------------------------------------
constexpr int LPN = 16;
constexpr int SITES_PER_BLOCK = 256 / LPN;


// Most sites of a move need no arc work at all — they are decided by their own numbers, or already carry alpha —
// so the whole-graph kernels of a move run in two steps per wavefront: one LANE per site looks at the site's scalars
// (64 sites per wave), then the sites that do need their arcs walked get LPN lanes each, four sites at a time.
// for_flagged calls body(m) on the 16 lanes of a group with m = the wave lane whose site the group serves; `mask`
// (the ballot of the lanes that asked for it) is wave-uniform, so every lane runs the loop and cross-lane reads of
// per-site scalars (__shfl(value, m)) may precede the call.
template <typename F>
__device__ __forceinline__ void for_flagged(unsigned long long mask, F body)
{
    const int grp = (int)(threadIdx.x & 63) / LPN;
    while (mask) {
        int b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            b[q] = mask ? (int)__builtin_ctzll(mask) : -1;
            if (mask) mask &= mask - 1;
        }
        const int m = grp == 0 ? b[0] : grp == 1 ? b[1] : grp == 2 ? b[2] : b[3];
        body(m);
    }
}
// Sites per wavefront in step one.  64 would use every lane, but then a 50k-site graph is 782 waves — less than one
// per SIMD — and a wave with many flagged sites serves them one group of four after the other (k_reduce at 11 labels:
// 27 us against 16 us for the plain LPN-lanes-per-site mapping).  16 keeps 3 125 waves and at most four rounds.
// r06: with several moves per launch (context = blockIdx.y) the launch has that many times the waves, and 16 sites per wave
// leave it with several rounds of residency, each paying the kernel's chain of dependent loads: `spw` is a launch argument,
// 64 for a batch's k_delta (few sites move), 16 / 32 / 64 by the size of the launch for its setup and reduction (run_expansion).
constexpr int SPW = 16;                         // a move alone
constexpr int SPW_MAX = 64;
constexpr int SITES_PER_WBLOCK_MAX = 4 * SPW_MAX;      // per 256-thread workgroup

// `label` is read (neighbours) and written (own site, pending move) in the same launch: a neighbour
// j with took[j] reads as `pa` whether or not its row has already stored the new label.
__global__ void __launch_bounds__(256)
k_move_setup(Graph g, const int* __restrict__ cost, int L, int potts, int reduce_on,
             int* label, int* __restrict__ cur_cost, MoveBatch b, int spw)
{
    const MoveCtx& c = b.c[blockIdx.y];
    const int alpha = c.alpha, t = c.t;
    const unsigned char* __restrict__ took = c.took;
    int* __restrict__ cap = c.cap;
    int* __restrict__ excess = c.excess;
    int* __restrict__ sink_cap = c.sink_cap;
    int* __restrict__ decided = c.decided;
    int* __restrict__ flags = c.flags;
    long long* __restrict__ acc = c.acc;
    const int lane = threadIdx.x & 63;
    const int sub = threadIdx.x % LPN;
    const int s0 = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * spw;
    const int i = s0 + lane;
    const bool in = lane < spw && i < g.n;
    const int pa = flags[C_PEND];
    int li = 0, cc = 0;
    if (in) {
        li = label[i];
        cc = cur_cost[i];
        if (pa >= 0 && took[i]) {                    // applyNewLabeling of the previous move, :423-441
            li = pa;
            cc = cost[(size_t)i * L + pa];
            label[i] = pa; cur_cost[i] = cc;
        }
    }
    if (__shfl(move_is_skipped(flags, t, L) ? 1 : 0, 0)) return;      // one evaluation per wave: C_ERROR may be raised meanwhile
    // step one.  A site that carries alpha is not in the graph (its neighbours clear the arcs towards it, both
    // directions).  A site whose own costs already outweigh every n-link it has is on the sink side whatever its
    // neighbours are: S <= cc + potts * wsum and in <= potts * wsum, so K - cc > 2 * potts * wsum implies -tr > in below.
    long long K = 0;
    bool walk = false;
    if (in) {
        if (li == alpha) decided[i] = 3;
        else {
            K = cost[(size_t)i * L + alpha];
            if (reduce_on && K - cc > 2ll * potts * g.wsum[i]) decided[i] = 2;
            else walk = true;
        }
    }
    for_flagged(__ballot(walk), [&](int m) {
        const int mm = m < 0 ? 0 : m;
        const int li_m = __shfl(li, mm), cc_m = __shfl(cc, mm);
        const long long K_m = __shfl(K, mm);
        if (m < 0) return;
        const int im = s0 + m;
        const int k0 = g.rowptr[im], k1 = g.rowptr[im + 1];
        long long S = 0, out = 0, inn = 0;
        for (int k = k0 + sub; k < k1; k += LPN) {
            const int j = g.col[k];
            const long long wk64 = (long long)g.w[k] * potts;
            if (wk64 > 0x7fffffffll) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);     // an n-link beyond int32 (GCO's EnergyTermType)
            const int wk = wk64 > 0x7fffffffll ? 0x7fffffff : (int)wk64;
            int lj = label[j];
            if (pa >= 0 && took[j]) lj = pa;
            if (lj == alpha) { S += wk; cap[k] = 0; cap[g.rev[k]] = 0; }
            else if (j < im) { if (li_m != lj) S += wk; cap[k] = wk; out += wk; if (li_m == lj) inn += wk; }
            else { const int c = (li_m == lj) ? wk : 0; cap[k] = c; out += c; inn += wk; }
        }
        S = row_sum64<LPN>(S) + cc_m;
        out = row_sum64<LPN>(out);
        inn = row_sum64<LPN>(inn);
        if (sub != 0) return;
        const long long tr = S - K_m;
        if (tr > 0x7fffffffll || -tr > 0x7fffffffll) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
        const int ex = tr > 0 ? (int)tr : 0;
        excess[im] = ex;
        sink_cap[im] = tr < 0 ? (int)(-tr) : 0;
        // first dominance test (see k_reduce): nothing is decided yet, so there is nothing to fold
        int verdict = 0;
        if (reduce_on) {
            if (tr > out) verdict = 1;
            else if (-tr > inn) verdict = 2;
        }
        decided[im] = verdict;
        // total excess of the move (the reference's flow counter is an int: Graph<int,int,int>), striped
        if (ex > 0) atomicAdd((unsigned long long*)&acc[A_EXCESS_S + (blockIdx.x % STRIPES) * STRIPE_LL], (unsigned long long)ex);
    });
}

// Dominance reduction (see the header).  net(u) = excess - sink_cap.  An undecided site first folds its
// decided neighbours into its own t-link — a source-side neighbour v delivers cap(v->u), a sink-side
// neighbour absorbs cap(u->v) — and clears both arcs, then tests
//     net >  sum of cap(u->w) over undecided w   ->  source side in every minimum cut
//    -net >  sum of cap(w->u) over undecided w   ->  residual sink capacity survives every max flow
// Strict inequalities: ties stay undecided and go to push-relabel, so the minimal sink side (BK's
// read-out, SURVEY A-1) is untouched.  Arcs between two undecided sites are never written here and
// a decided site never writes again, so rounds may run chaotically: every verdict holds given any
// subset of earlier verdicts (a stale "undecided" view only makes the tests stricter).
// The fixed point is reached inside k_solve; these launches take the bulk of the cascade off it.
// COMPACT: sites still undecided when their row finishes are appended to the core list.
template <bool COMPACT>
__global__ void __launch_bounds__(256)
k_reduce(Graph g, int L, MoveBatch b, int ROUNDS, int housekeep, int spw)
{
    const MoveCtx& c = b.c[blockIdx.y];
    const int t = c.t;
    int* cap = c.cap;
    int* excess = c.excess;
    int* sink_cap = c.sink_cap;
    int* decided = c.decided;
    int* __restrict__ flags = c.flags;
    long long* __restrict__ acc = c.acc;
    int* __restrict__ core = c.core;
    // COMPACT walks the sites in a fixed pseudo-random order (g.order).  The solver gives 64 consecutive core sites to
    // one workgroup, and the sites that are busy in a move are neighbours in the image: were they also neighbours in
    // the list (input sorted along a scan line, a Z-curve ...) a few CUs would issue all the uncoalesced requests of
    // a phase.  Measured with the core in Z-curve order: 55-60 ms of solver time per LabelingStep instead of 20.
    const int lane = threadIdx.x & 63;
    const int sub = threadIdx.x % LPN;
    const int slot = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * spw + lane;
    const int u = (lane < spw && slot < g.n) ? (COMPACT ? g.order[slot] : slot) : -1;
    __shared__ int s_skip;                               // one evaluation per workgroup: C_ERROR may be raised meanwhile
    __shared__ int s_cnt, s_base;
    __shared__ int s_list[SITES_PER_WBLOCK_MAX];
    if (threadIdx.x == 0) { s_skip = move_is_skipped(flags, t, L) ? 1 : 0; s_cnt = 0; }
    __syncthreads();
    const bool skipped = s_skip != 0;
    if (housekeep && blockIdx.x == 0 && threadIdx.x == 0) {
        // housekeeping of the move, for the launches behind this one (the first reduction launch of a move does it;
        // the core counters and the solver's barrier words are cleared by k_delta, behind the solver launch that used them)
        flags[C_PEND] = -1;                              // k_move_setup has applied it
        flags[C_TICKET] = 0;
        flags[C_TOOK_N] = 0;
        for (int s = 0; s < SUBTICKETS; ++s) flags[C_SUBTICKET + s * C_LINE] = 0;
        long long ex = 0;
        for (int s = 0; s < STRIPES; ++s) { ex += acc[A_EXCESS_S + s * STRIPE_LL]; acc[A_EXCESS_S + s * STRIPE_LL] = 0; acc[A_DELTA_S + s * STRIPE_LL] = 0; }
        if (!skipped && ex > 0x7fffffffll) flags[C_ERROR] = ERR_OVERFLOW;
    }
    if (skipped) return;
    // step one: who is still undecided; step two: LPN lanes per such site
    const bool open = u >= 0 && LD(&decided[u]) == 0;
    for_flagged(__ballot(open), [&](int m) {
        const int um = __shfl(u, m < 0 ? 0 : m);
        if (m < 0) return;
        const int k0 = g.rowptr[um], k1 = g.rowptr[um + 1];
        long long net = (long long)excess[um] - sink_cap[um];
        bool dirty = false;
        int verdict = 0;
        for (int r = 0; r < ROUNDS; ++r) {
            long long add = 0, out = 0, in = 0;
            for (int k = k0 + sub; k < k1; k += LPN) {
                const int kr = g.rev[k];
                const int co = cap[k], ci = cap[kr];
                if ((co | ci) == 0) continue;
                const int dv = LD(&decided[g.col[k]]);
                if (dv == 1) { add += ci; cap[k] = 0; cap[kr] = 0; }
                else if (dv == 2) { add -= co; cap[k] = 0; cap[kr] = 0; }
                else { out += co; in += ci; }
            }
            add = row_sum64<LPN>(add); out = row_sum64<LPN>(out); in = row_sum64<LPN>(in);
            if (add != 0) { net += add; dirty = true; }
            if (net > out) verdict = 1;
            else if (-net > in) verdict = 2;
            if (verdict) break;
        }
        if (sub == 0) {
            if (dirty) {
                if (net > 0x7fffffffll || -net > 0x7fffffffll) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
                excess[um] = net > 0 ? (int)net : 0;
                sink_cap[um] = net < 0 ? (int)(-net) : 0;
            }
            if (verdict) ST(&decided[um], verdict);
            else if (COMPACT) s_list[atomicAdd(&s_cnt, 1)] = um;
        }
    });
    if (COMPACT) {
        __syncthreads();
        const int shard = blockIdx.x % EXPAND_CORE_SHARDS;
        if (threadIdx.x == 0 && s_cnt > 0) s_base = atomicAdd(&flags[C_CORE + shard], s_cnt);
        __syncthreads();
        if ((int)threadIdx.x < s_cnt) core[(size_t)shard * g.n + s_base + threadIdx.x] = s_list[threadIdx.x];
    }
}

// DIAGNOSTIC (mh_set_tuning key 21): connected components of a move's undecided core — the sites the
// dominance reduction left to the flow solver, joined where two of them are neighbours (their n-link has capacity; links
// to decided sites were folded into t-links).  One workgroup: min-label propagation with pointer jumping to the fixed
// point, then sizes.  out[16]: {core sites, components, largest, second largest, sites in components of <= 64 / 256 / 1024 /
// 2048 / 8192 sites (cumulative), components of <= 64 / 256 / 1024 / 2048 / 8192 sites (cumulative), propagation rounds, 0}.
// comp, csize: n ints of scratch each.  Never on the product path.
__global__ void __launch_bounds__(1024)
k_core_components(Graph g, int L, int t, const int* __restrict__ decided, const int* __restrict__ flags, int* __restrict__ comp,
                  int* __restrict__ csize, int* __restrict__ out)
{
    __shared__ int s_changed, s_acc[16];
    if (threadIdx.x < 16) { s_acc[threadIdx.x] = 0; out[threadIdx.x] = 0; }
    if (move_is_skipped(flags, t, L)) return;
    for (int i = threadIdx.x; i < g.n; i += 1024) { comp[i] = decided[i] == 0 ? i : -1; csize[i] = 0; }
    __syncthreads();
    int rounds = 0;
    for (;;) {
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < g.n; i += 1024) {
            int c = comp[i];
            if (c < 0) continue;
            int m = c;
            for (int k = g.rowptr[i]; k < g.rowptr[i + 1]; ++k) { const int cj = comp[g.col[k]]; if (cj >= 0 && cj < m) m = cj; }
            if (m < c) { atomicMin(&comp[i], m); atomicMin(&comp[c], m); s_changed = 1; }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < g.n; i += 1024) {          // pointer jumping
            int c = comp[i];
            if (c < 0) continue;
            while (comp[c] < c) c = comp[c];
            comp[i] = c;
        }
        __syncthreads();
        ++rounds;
        if (!s_changed || rounds > 4096) break;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < g.n; i += 1024) if (comp[i] >= 0) { atomicAdd(&csize[comp[i]], 1); atomicAdd(&s_acc[0], 1); }
    __syncthreads();
    for (int i = threadIdx.x; i < g.n; i += 1024) {
        const int sz = csize[i];
        if (sz <= 0) continue;
        atomicAdd(&s_acc[1], 1);
        const int old = atomicMax(&s_acc[2], sz);
        atomicMax(&s_acc[3], old < sz ? old : sz);              // (a lower bound of the second largest; exact when sizes arrive in any order but ties)
        if (sz <= 64) { atomicAdd(&s_acc[4], sz); atomicAdd(&s_acc[9], 1); }
        if (sz <= 256) { atomicAdd(&s_acc[5], sz); atomicAdd(&s_acc[10], 1); }
        if (sz <= 1024) { atomicAdd(&s_acc[6], sz); atomicAdd(&s_acc[11], 1); }
        if (sz <= 2048) { atomicAdd(&s_acc[7], sz); atomicAdd(&s_acc[12], 1); }
        if (sz <= 8192) { atomicAdd(&s_acc[8], sz); atomicAdd(&s_acc[13], 1); }
    }
    __syncthreads();
    if (threadIdx.x < 16) out[threadIdx.x] = threadIdx.x == 14 ? rounds : s_acc[threadIdx.x];
}

// Energy difference of the candidate labeling (sites with decided == 1 take alpha) and, by the last
// workgroup to finish, the verdict of the move: accept iff the energy strictly decreases (:1259).
__global__ void __launch_bounds__(256)
k_delta(Graph g, const int* __restrict__ cost, int L, int potts,
        const int* __restrict__ label, const int* __restrict__ cur_cost, MoveBatch b, int spw)
{
    const MoveCtx& c = b.c[blockIdx.y];
    const int alpha = c.alpha, t = c.t;
    const int* __restrict__ decided = c.decided;
    unsigned char* __restrict__ took = c.took;
    int* __restrict__ flags = c.flags;
    long long* acc = c.acc;
    __shared__ long long s[256];
    __shared__ int s_last;
    if (threadIdx.x == 0) s_last = move_is_skipped(flags, t, L) ? 1 : 0;
    __syncthreads();
    if (s_last) return;
    // step one: every site records whether it moves; step two: the sites that move walk their arcs.  A pair of
    // neighbours changes its Potts term only if one of them moves: it is counted from the moving end, or — both
    // moving — from the end with the larger index.
    const int lane = threadIdx.x & 63;
    const int sub = threadIdx.x % LPN;
    const int s0 = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * spw;
    const int i = s0 + lane;
    long long mine = 0;
    int oi = 0;
    bool ti = false;
    if (lane < spw && i < g.n) {
        oi = label[i];
        ti = decided[i] == 1;
        took[i] = ti ? 1 : 0;
        if (ti) mine += (long long)cost[(size_t)i * L + alpha] - cur_cost[i];
    }
    if (c.took_list) {                                   // (wave-uniform) the moving sites as a list, for k_commit
        const unsigned long long tb = __ballot(ti);
        if (tb) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&flags[C_TOOK_N], (int)__popcll(tb));
            base = __shfl(base, 0);
            if (ti) c.took_list[base + (int)__popcll(tb & ((1ull << lane) - 1ull))] = i;
        }
    }
    for_flagged(__ballot(ti), [&](int m) {
        const int oi_m = __shfl(oi, m < 0 ? 0 : m);
        if (m < 0) return;
        const int im = s0 + m;
        for (int k = g.rowptr[im] + sub; k < g.rowptr[im + 1]; k += LPN) {
            const int j = g.col[k];
            const bool tj = decided[j] == 1;
            if (tj && j > im) continue;
            const int oj = label[j];
            const int nj = tj ? alpha : oj;
            const int dn = (alpha != nj) - (oi_m != oj);
            mine += (long long)dn * g.w[k] * potts;
        }
    });
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s[0] != 0) atomicAdd((unsigned long long*)&acc[A_DELTA_S + (blockIdx.x % STRIPES) * STRIPE_LL], (unsigned long long)s[0]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // my sum has landed before my ticket
        // two-level ticket: the last of my sub-ticket's workgroups takes a top ticket, the last of those finishes the move
        const int st = (int)(blockIdx.x % SUBTICKETS);
        const int members = ((int)gridDim.x - st + SUBTICKETS - 1) / SUBTICKETS;
        int last = 0;
        if (atomicAdd(&flags[C_SUBTICKET + st * C_LINE], 1) == members - 1) {
            const int used = (int)gridDim.x < SUBTICKETS ? (int)gridDim.x : SUBTICKETS;
            last = atomicAdd(&flags[C_TICKET], 1) == used - 1;
        }
        s_last = last;
    }
    __syncthreads();
    if (s_last && threadIdx.x < 64) {
        long long d = (int)threadIdx.x < STRIPES ? LD(&acc[A_DELTA_S + threadIdx.x * STRIPE_LL]) : 0ll;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
        if (threadIdx.x == 0 && d < 0) {
            flags[C_TLAST] = t;
            flags[C_PEND] = alpha;
            flags[C_ACCEPTED] += 1;
        }
        if (threadIdx.x == 0) {
            flags[C_MOVES_RUN] += 1;
            // for the next move: the core list is empty again, the solver's barrier words are clear
            for (int s = 0; s < EXPAND_CORE_SHARDS; ++s) flags[C_CORE + s] = 0;
            for (int s = C_XCD; s < C_TOP + C_LINE; ++s) flags[s] = 0;
            flags[C_ARRIVE] = 0;
        }
    }
}

// The labels of a pending accepted move, when no k_move_setup follows (end of a cycle).
__global__ void __launch_bounds__(256)
k_apply_pending(int n, const int* __restrict__ cost, int L, int* __restrict__ label,
                int* __restrict__ cur_cost, const unsigned char* __restrict__ took,
                const int* __restrict__ flags, int /* in_front_of_a_batch */)
{
    const int pa = flags[C_PEND];
    if (pa < 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && took[i]) {                                      // applyNewLabeling, :423-441
        label[i] = pa;
        cur_cost[i] = cost[(size_t)i * L + pa];
    }
}


// ---------------------------------------------------------------------------
// r06: CONCURRENT ALPHA-MOVES.  oneExpansionIteration (GCoptimization.cpp:1278-1289) runs the expansions on alpha = 0, 1, ...
// one after the other, each on the labeling its predecessor left.  Here K consecutive moves are solved TOGETHER on the same
// labeling f (one launch of each move kernel, context = blockIdx.y), and k_batch_commit then walks them in the reference's order
// and keeps a move's result only when it is provably what the sequential order would have given:
//
//   Let the accepted predecessors of move beta in this batch have changed the sites S (f -> f').  Write W_p = potts * sum_q w_pq
//   and call p UNARY-KEPT for beta under a labeling g when  D_beta(p) - D_{g_p}(p) > W_p  (or g_p = beta: p is not a variable
//   of the move at all): switching p to beta costs more in its data term than all its n-links together can return, so p keeps
//   its label in EVERY minimum cut.  If every p in S u N(S) is unary-kept for beta under f AND under f', then in both problems
//   — beta on f, beta on f' — those sites stay, the sites outside S u N(S) see the same unary terms, the same n-links among
//   themselves and the same (unchanged) labels on the N(S) side of their other n-links: the two problems have the same set of
//   minimum cuts, hence the same canonical one (the read-out is BK's minimal sink side, SURVEY A-1), the same sites take beta,
//   and — every term that changes touches only sites whose labels agree in f and f' — the same energy gain, so the same verdict.
//   A move that fails the test is not kept: it becomes the first move of the next batch, solved on the labeling as it then stands.
//   The test for (j, k) reads the labeling the batch started from, j's list of moving sites and the two labels — not which other
//   moves are accepted — so k_batch_check evaluates all pairs in parallel and k_batch_commit only walks a K x K bit table.
//
// A move that was skipped as idempotent when the batch began (move_is_skipped: nothing accepted since its label's last
// expansion) stays skipped only while no predecessor in its batch is accepted; otherwise it is re-run too.  Labels, energies and
// cycle counts are therefore the sequential ones (every parity test, golden file and stress tool runs through this path).
// ---------------------------------------------------------------------------

// In front of a batch: the contexts beyond 0 see the control words context 0 — the global ones — holds now.
__global__ void k_batch_prep(MoveBatch b, int* __restrict__ bctl)
{
    int* G = b.c[0].flags;
    const int k = threadIdx.x;
    if (k == 0) { bctl[B_TLAST0] = G[C_TLAST]; G[C_PEND] = -1; }      // (whatever was pending has been applied: k_apply_pending, or k_batch_commit)
    if (k < EXPAND_MAX_CTX) bctl[B_BAD + k] = 0;
    if (k >= 1 && k < b.count) {
        int* f = b.c[k].flags;
        f[C_TLAST] = G[C_TLAST];
        f[C_PEND] = -1;
        f[C_ERROR] = G[C_ERROR];
    }
}

__device__ __forceinline__ bool batch_move_skipped(const MoveCtx& c, int tlast0, int L)
{
    return c.flags[C_ERROR] != 0 || (c.t >= L && tlast0 <= c.t - L);           // what every launch of this move evaluated
}

// Behind a batch's k_delta, in parallel over everything: for every move j of the batch that would be accepted and every LATER move
// k, does k pass the test above against what j changes?  The test looks only at the labeling the batch started from, at j's took
// list and at the two labels — nothing in it depends on which other moves end up accepted — so all pairs are checked at once:
// bit k of bctl[B_BAD + j] = "move k must not be kept if move j is".  Context blockIdx.y = j; 16 lanes per site of j's list walk
// the site and its neighbours.  (The labels of the batch are consecutive, so a site's costs for all later moves are contiguous.)
__global__ void __launch_bounds__(256)
k_batch_check(Graph g, const int* __restrict__ cost, int L, int potts, const int* __restrict__ label, const int* __restrict__ cur_cost,
              MoveBatch b, int* __restrict__ bctl)
{
    const int j = blockIdx.y;
    if (j + 1 >= b.count) return;                        // nothing comes behind the last move
    const MoveCtx& cj = b.c[j];
    const int tlast0 = bctl[B_TLAST0];
    if (batch_move_skipped(cj, tlast0, L) || cj.flags[C_PEND] < 0) return;       // skipped or rejected: it changes nothing
    const int nt = cj.flags[C_TOOK_N];
    const int sub = threadIdx.x % LPN;
    const int alpha_j = cj.alpha, later = b.count - 1 - j;
    unsigned bad = 0;
    for (int idx = blockIdx.x * SITES_PER_BLOCK + (int)threadIdx.x / LPN; idx < nt; idx += gridDim.x * SITES_PER_BLOCK) {
        const int p = cj.took_list[idx];
        const int k0 = g.rowptr[p], k1 = g.rowptr[p + 1];
        // lane `sub` serves the neighbours k0 + sub, k0 + sub + 16, ...; lane 0 also the site itself (slot -1)
        for (int a = k0 + sub - (sub == 0 ? 1 : 0); a < k1; a = (a < k0 ? k0 : a + LPN)) {
            const int s_ = a < k0 ? p : g.col[a];
            const long long W = (long long)potts * g.wsum[s_];
            const int lb = label[s_];
            const long long Dl = cur_cost[s_];
            const int* row = cost + (size_t)s_ * L + (alpha_j + 1);
            const long long Dj = a < k0 ? (long long)cost[(size_t)s_ * L + alpha_j] : 0;
            for (int q = 0; q < later; ++q) {
                const long long Db = row[q];
                bool ok = lb == alpha_j + 1 + q || Db - Dl > W;                    // under the labeling the batch started from
                if (ok && a < k0) ok = Db - Dj > W;                               // the changed site itself: also under its new label
                if (!ok) bad |= 1u << (j + 1 + q);
            }
        }
    }
    // (moves skipped when the batch began have no verdict to keep: k_batch_commit handles them)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad |= (unsigned)__shfl_xor((int)bad, m, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr((unsigned*)&bctl[B_BAD + j], bad);
}

// ... then the commit, in the reference's order (see above): every workgroup derives the same decisions from the same words —
// none of which is written before all workgroups have read them — and applies its share of the accepted moves' took lists
// (applyNewLabeling, :423-441); the LAST workgroup to finish records the outcome in the global control words, publishes it to the
// host and prepares the contexts for the next batch.
struct CtxFlags { int* p[EXPAND_MAX_CTX]; };       // the control words of ALL contexts of the engine (a batch may use fewer)
__global__ void __launch_bounds__(256)
k_batch_commit(const int* __restrict__ cost, int L, int* __restrict__ label, int* __restrict__ cur_cost, MoveBatch b,
               int* __restrict__ bctl, int* __restrict__ h_batch, CtxFlags all_flags, int n_ctx_all)
{
    __shared__ int s_first, s_err, s_last_t, s_n_acc;
    __shared__ unsigned s_acc;
    // the words the walk below looks at, fetched by one lane per move (the walk itself is sequential: on one lane's own loads it
    // cost a memory round trip per move and word, 12 us for sixteen moves)
    __shared__ int s_ek[EXPAND_MAX_CTX], s_pend[EXPAND_MAX_CTX], s_nt[EXPAND_MAX_CTX];
    __shared__ unsigned s_bad[EXPAND_MAX_CTX];
    __shared__ int s_g[5];                               // B_TLAST0, the global C_ERROR / C_TLAST / C_ACCEPTED, B_SEQ: written by this launch's LAST workgroup only
    if ((int)threadIdx.x < b.count) {
        const int* f = b.c[threadIdx.x].flags;
        s_ek[threadIdx.x] = f[C_ERROR];
        s_pend[threadIdx.x] = f[C_PEND];
        s_nt[threadIdx.x] = f[C_TOOK_N];
        s_bad[threadIdx.x] = (unsigned)bctl[B_BAD + threadIdx.x];
    } else if (threadIdx.x >= 64 && threadIdx.x < 69) {
        const int q = threadIdx.x - 64;
        const int* G = b.c[0].flags;
        s_g[q] = q == 0 ? bctl[B_TLAST0] : q == 1 ? G[C_ERROR] : q == 2 ? G[C_TLAST] : q == 3 ? G[C_ACCEPTED] : bctl[B_SEQ];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tlast0 = s_g[0];
        unsigned accepted = 0;
        int first_invalid = b.count, err = 0, last_t = -1, n_acc = 0;
        for (int k = 0; k < b.count; ++k) {
            const MoveCtx& c = b.c[k];
            const int ek = s_ek[k];
            const bool skipped = ek != 0 || (c.t >= L && tlast0 <= c.t - L);
            bool valid = true;
            if (accepted) {
                if (skipped) valid = false;                  // no longer idempotent: something in front of it changed the labeling
                else
                    for (int j = 0; j < k; ++j)
                        if ((accepted >> j & 1u) && (s_bad[j] >> k & 1u)) valid = false;
            }
            if (!valid) { first_invalid = k; break; }
            // a move's error counts only when the move is kept: one that is thrown away was solved on a labeling the sequential
            // order never offered it (its error is cleared below with the contexts behind it, and it heads the next batch)
            if (ek) err = ek;
            if (!skipped && s_pend[k] >= 0) { accepted |= 1u << k; last_t = c.t; ++n_acc; }
        }
        s_first = first_invalid; s_err = err; s_acc = accepted; s_last_t = last_t; s_n_acc = n_acc;
    }
    __syncthreads();
    const unsigned accepted = s_acc;
    for (int k = 0; k < b.count; ++k) {
        if (!(accepted >> k & 1u)) continue;
        const MoveCtx& c = b.c[k];
        const int nt = s_nt[k], a = c.alpha;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < nt; i += gridDim.x * 256) {
            const int p = c.took_list[i];
            label[p] = a;
            cur_cost[p] = cost[(size_t)p * L + a];
        }
    }
    // The global control words, the publication and the next batch's preparation are the LAST workgroup's to write: every workgroup
    // has derived its decisions from those words and must have finished reading them.
    __shared__ int s_is_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        s_is_last = atomicAdd(&bctl[B_TICKET], 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (s_is_last && threadIdx.x == 0) {
        bctl[B_TICKET] = 0;
        int* G = b.c[0].flags;
        // (the global words as they stood when the launch began — nobody but this thread writes them in it)
        const int g_err = s_g[1] ? s_g[1] : s_err;
        // (context 0's k_delta wrote the global words for its own move itself: count the others)
        const int g_tlast = s_last_t > s_g[2] ? s_last_t : s_g[2];
        const int seq = s_g[4] + 1;
        if (g_err != s_g[1]) G[C_ERROR] = g_err;
        if (g_tlast != s_g[2]) G[C_TLAST] = g_tlast;
        G[C_ACCEPTED] = s_g[3] + s_n_acc - (int)(accepted & 1u);
        bctl[B_SEQ] = seq;
        h_batch[HB_FIRST_INVALID] = s_first;
        h_batch[HB_TLAST] = g_tlast;
        h_batch[HB_ERROR] = g_err;
        h_batch[HB_ACCEPTED_HERE] = s_n_acc;
        h_batch[HB_DIRTY] = 0;
        // the host POLLS the sequence word (run_expansion): everything above — and every label the other workgroups wrote, which
        // their fences ordered before their tickets — is visible to it before the word changes
        __threadfence_system();
        __hip_atomic_store(&h_batch[HB_SEQ], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        // ... and what k_batch_prep would do in front of the NEXT batch, whatever that batch will hold (every context, not just the
        // ones it uses): a batch that follows a commit directly needs no launch of its own for it.  This also clears C_ERROR of the
        // first invalid context and of those behind it: what their solves raised belongs to problems no longer posed
        bctl[B_TLAST0] = g_tlast;
        G[C_PEND] = -1;
        for (int k = 0; k < EXPAND_MAX_CTX; ++k) bctl[B_BAD + k] = 0;
        for (int k = 1; k < n_ctx_all; ++k) {
            int* f = all_flags.p[k];
            f[C_TLAST] = g_tlast;
            f[C_PEND] = -1;
            f[C_ERROR] = g_err;
        }
    }
}

// The solver's statistics of the contexts beyond 0 into context 0's words (which k_publish mirrors to the host).  One thread
// per word, the contexts in sequence.
__global__ void k_stats_merge(MoveBatch b)
{
    const int t = threadIdx.x;
    int* G = b.c[0].flags;
    long long* A = b.c[0].acc;
    const int fw[5] = { C_FLOW_MOVES, C_MOVES_SOLVED, C_MOVES_RUN, C_CORE_MAX, C_XCD_USED };
    if (t < 5) {
        const int w = fw[t];
        int v = G[w];
        for (int k = 1; k < b.count; ++k) {
            int* f = b.c[k].flags;
            if (t < 3) v += f[w]; else if (f[w] > v) v = f[w];
            f[w] = 0;
        }
        G[w] = v;
    } else if (t >= 8 && t - 8 + A_CORE_SUM < A_COUNT) {
        const int w = t - 8 + A_CORE_SUM;
        long long v = A[w];
        for (int k = 1; k < b.count; ++k) {
            long long* a = b.c[k].acc;
            if (w == A_MAX_WAIT) { if (a[w] > v) v = a[w]; } else v += a[w];
            a[w] = 0;
        }
        A[w] = v;
    }
}

// compute_energy = data + smooth (:953-956; giveSmoothEnergyInternal :267-286)
__global__ void __launch_bounds__(256)
k_energy(Graph g, int potts, const int* __restrict__ label, const int* __restrict__ cur_cost,
         int* __restrict__ flags, long long* __restrict__ acc)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[C_PEND] = -1;     // k_apply_pending ran in front of this launch
    const int i = blockIdx.x * SITES_PER_BLOCK + threadIdx.x / LPN;
    const int sub = threadIdx.x % LPN;
    long long mine = 0;
    if (i < g.n) {
        if (sub == 0) mine = cur_cost[i];
        const int li = label[i];
        for (int k = g.rowptr[i] + sub; k < g.rowptr[i + 1]; k += LPN) {
            const int j = g.col[k];
            if (j < i && label[j] != li) mine += (long long)g.w[k] * potts;
        }
    }
    __shared__ long long s[256];
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        atomicAdd((unsigned long long*)&acc[A_ENERGY_S + (blockIdx.x % STRIPES) * STRIPE_LL], (unsigned long long)s[0]);
}

hipError_t launch_init_labeling(const int* cost, int L, int n, const int* init, int* label,
                                int* cur_cost, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_labeling, dim3((n + 255) / 256), dim3(256), 0, s, cost, L, n, init,
                       label, cur_cost);
    return hipGetLastError();
}

hipError_t launch_argmin_labels(const int* cost, int L, int n, int* label, long long* acc,
                                hipStream_t s)
{
    hipLaunchKernelGGL(k_argmin_labels, dim3((n + 255) / 256), dim3(256), 0, s, cost, L, n, label,
                       acc);
    return hipGetLastError();
}

// Control words travel to the host through device-mapped pinned memory: one 1-wave kernel copies
// them (no hipMemcpy calls, which cost tens of microseconds each for a few bytes), then the host
// waits for the stream.
__global__ void k_publish(const int* __restrict__ flags, long long* __restrict__ acc,
                          int* __restrict__ h_flags, long long* __restrict__ h_acc)
{
    const int t = threadIdx.x;
    if (t < EXPAND_HOST_WORDS) h_flags[t] = flags[t];
    long long en = t < STRIPES ? acc[A_ENERGY_S + t * STRIPE_LL] : 0ll;      // k_energy's (or k_argmin_labels') stripes
    if (t < STRIPES) acc[A_ENERGY_S + t * STRIPE_LL] = 0;                     // the next k_energy accumulates from zero
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) en += __shfl_xor(en, m, 64);
    if (t < A_COUNT) h_acc[t] = t == A_ENERGY ? en : acc[t];
}

namespace {

ExpandResult hip_failed(hipError_t e) { return ExpandResult{ ExpandStatus::hip_error, e }; }
#define RET_IF(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_failed(e_); } while (0)

// Every launch of an expansion goes through here, which is where ExpandStats::launches is counted.  A move alone costs FOUR
// launches (k_move_setup, k_reduce<true>, k_solve, k_delta; five with the second reduction launch of key 7), a batch of any
// size those plus k_batch_check and k_batch_commit (and k_batch_prep, or k_apply_pending, in front of it when the batch does
// not follow a commit directly); a cycle ends with k_apply_pending, k_energy, k_stats_merge (several contexts) and k_publish.
// Not counted, as they never were: the diagnostic k_core_components (`uncounted`) and what is launched outside this file's
// schedule (launch_init_labeling in front of an expansion, launch_argmin_labels for a graph without arcs); the memsets of the
// batch control words and of the key-40 hook are not kernels.  k_ctl_init is launch 1, the first k_energy and the k_publish
// behind it 2 and 3 (fetch counts its own k_publish and a host wait).
struct Launcher {
    hipStream_t s;
    ExpandStats& stats;
    template <class... P, class... A>
    void operator()(void (*k)(P...), dim3 grid, dim3 blk, A&&... a) { ++stats.launches; uncounted(k, grid, blk, a...); }
    template <class... P, class... A>
    void uncounted(void (*k)(P...), dim3 grid, dim3 blk, A&&... a) { hipLaunchKernelGGL(k, grid, blk, 0, s, a...); }
    void solve(const SolveLaunch& sl, const Graph& g, int L, const MoveBatch& b, const SolveParams& sp)
    {
        ++stats.launches;
        launch_solve(sl, g, L, b, sp, s);
    }
};

// Context 0's control words and accumulators to the host, and the host waits for them.
hipError_t fetch(const ExpandWork& w, Launcher& launch)
{
    ++launch.stats.host_syncs;
    launch(k_publish, dim3(1), dim3(64), w.ctx[0].flags, w.ctx[0].acc, w.h_flags_dev, w.h_acc_dev);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipStreamSynchronize(launch.s);
}

// The host needs four words of a batch's commit before it can enqueue the next batch.  Waiting for the stream costs 15-20 us
// a time (a thousand times per Process() on the reference's route); the commit writes its words to mapped host memory
// and the sequence number last, behind a system-scope fence, so the host polls that word instead — for at most 2 ms
// (a batch with large cores), then it waits for the stream as before.  Launches stay ordered by the stream either way.
hipError_t await_commit(const int* h_batch, int batch_seq, hipStream_t s)
{
    const volatile int* seq_word = h_batch + HB_SEQ;
    const auto t_poll = std::chrono::steady_clock::now();
    bool seen = false;
    for (int spin = 0;; ++spin) {
        if (*seq_word == batch_seq) { seen = true; break; }
        if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t_poll > std::chrono::milliseconds(2)) break;
    }
    if (seen) std::atomic_thread_fence(std::memory_order_acquire);
    else if (hipError_t e = hipStreamSynchronize(s); e != hipSuccess) return e;
    return h_batch[HB_SEQ] == batch_seq ? hipSuccess : hipErrorUnknown;   // (cannot happen: the commit always publishes)
}

ExpandStatus status_of(int err_word)
{
    return err_word == ERR_OVERFLOW ? ExpandStatus::overflow : err_word == ERR_BARRIER_TIMEOUT ? ExpandStatus::barrier_timeout
                                                                                               : ExpandStatus::no_convergence;
}

} // namespace

ExpandResult run_expansion(const Graph& g, const int* cost, int L, int potts, ExpandWork& w,
                           int max_cycles, ExpandStats* st, hipStream_t s)
{
    const ExpandTuning& tu = w.tune;
    const dim3 grid1((g.n + 255) / 256), blk(256);                          // one thread per site
    const dim3 grid((g.n + SITES_PER_BLOCK - 1) / SITES_PER_BLOCK);        // LPN lanes per site, 256 threads
    // whole-graph launches of a move: one lane per site first (spw sites per wave), then LPN lanes for the sites that need them
    // (setup and reduction: a wave with many sites to walk serves them four at a time, so more sites per wave pay only once the
    // launch would otherwise need several rounds of residency — 16 moves x 50 000 sites at 16 per wave are 50 000 waves, six
    // rounds: loop of the reference's route at configs[4] 0.363 -> 0.349 s with 64; at 20 000 sites no difference.  0 = by size)
    auto spw_for = [&](int count) {
        if (tu.batch_spw == 16 || tu.batch_spw == 32 || tu.batch_spw == 64) return tu.batch_spw;
        const long long site_moves = (long long)count * g.n;
        return site_moves > (1ll << 19) ? 64 : site_moves > (1ll << 18) ? 32 : 16;
    };
    ExpandStats stats = {};
    Launcher launch{ s, stats };
    auto ended = [&](ExpandStatus status) { if (st) *st = stats; return ExpandResult{ status, hipSuccess }; };
    const int n_ctx = std::max(1, std::min(w.n_ctx, EXPAND_MAX_CTX));
    MoveBatch all{};
    all.count = n_ctx;
    CtxFlags all_flags{};
    for (int k = 0; k < n_ctx; ++k) {
        const ExpandWork::Ctx& x = w.ctx[k];
        MoveCtx& c = all.c[k];
        c.cap = x.cap; c.sent = x.sent; c.excess = x.excess; c.sink_cap = x.sink_cap; c.height = x.height; c.decided = x.decided;
        c.took = x.took; c.core = x.core; c.flags = x.flags; c.acc = x.acc; c.took_list = x.took_list;
        all_flags.p[k] = x.flags;
    }
    const ExpandWork::Ctx& ctx0 = w.ctx[0];              // the global control words, the published accumulators (expand_ctl.hpp)
    launch(k_ctl_init, dim3(n_ctx), dim3(64), all);
    RET_IF(hipGetLastError());
    auto finish_cycle = [&]() -> hipError_t {             // the contexts' solver statistics, then the control words to the host
        if (n_ctx > 1) launch(k_stats_merge, dim3(1), dim3(64), all);
        return fetch(w, launch);
    };

    if (g.nnz == 0) {                                  // solveSpecialCases, :470-491
        RET_IF(launch_argmin_labels(cost, L, g.n, w.label, ctx0.acc, s));
        RET_IF(fetch(w, launch));
        stats.energy = w.h_acc[A_ENERGY];
        return ended(ExpandStatus::ok);
    }

    long long energy = 0, old_energy = 0;
    launch(k_energy, grid, blk, g, potts, w.label, w.cur_cost, ctx0.flags, ctx0.acc);     // :1036
    RET_IF(fetch(w, launch));
    energy = w.h_acc[A_ENERGY];
    if (energy > 0x7fffffffll)                         // GCO's EnergyType is int: it would compare wrapped energies from here on
        return ended(ExpandStatus::overflow);

    const SolveParams sp{ tu.reduce_rounds, tu.relax_rounds, tu.push_cycles, tu.push_phases, tu.push_mult > 0 ? tu.push_mult : 1, 1 << 20, tu.cascade_iters,
                          tu.barrier_timeout_ticks > 0 ? (unsigned long long)tu.barrier_timeout_ticks : 300000000ull,
                          tu.barrier_first_timeout_ticks > 0 ? (unsigned long long)tu.barrier_first_timeout_ticks : 300000000ull };
    SolveLaunch sl;
    RET_IF(prepare_solve(g.n, tu.solve_grid > 0 ? tu.solve_grid : 128, &sl));
    if (!sl.fits) return ExpandResult{ ExpandStatus::too_many_sites, hipSuccess };

    // The launches of `count` consecutive moves (labels alpha0 ..., move indices t0 ...) solved on the same labeling, contexts
    // 0 .. count - 1.  count == 1: a move alone, the sequential form.
    bool prepared = false;       // the contexts beyond 0 hold the global control words as they stand (nothing but batches has run since)
    int group = 0;               // groups of moves enqueued (batches and moves alone), for the test hook of key 40
    int injected_ctx = -1;       // the context of the current group whose solve the hook marked failed, -1 none
    auto enqueue_moves = [&](int alpha0, int t0, int count, int cycle) -> hipError_t {
        MoveBatch b = all;
        b.count = count;
        for (int k = 0; k < count; ++k) {
            MoveCtx& c = b.c[k];
            c.alpha = alpha0 + k;
            c.t = t0 + k;
            c.trace = (w.trace && c.t < w.trace_moves) ? w.trace : nullptr;
            c.detail = (w.trace && c.t == w.detail_move) ? w.trace + 8 * (size_t)w.trace_moves : nullptr;
            c.saved_flow = w.saved_flow ? w.saved_flow + (size_t)c.alpha * g.nnz : nullptr;
            c.saved_sink = w.saved_flow ? w.saved_sink + (size_t)c.alpha * g.n : nullptr;
            c.warm = (w.saved_flow && cycle > 1) ? 1 : 0;
            if (count == 1) c.took_list = nullptr;             // a move alone: nobody walks the list
        }
        const int spw = count > 1 ? spw_for(count) : SPW;
        const int spw_d = count > 1 ? SPW_MAX : SPW;                  // k_delta: few sites move, every lane looks at one
        const dim3 grid_w((unsigned)((g.n + 4 * spw - 1) / (4 * spw)), (unsigned)count);
        const dim3 grid_d((unsigned)((g.n + 4 * spw_d - 1) / (4 * spw_d)), (unsigned)count);
        // (a batch right behind another batch's commit finds the contexts prepared by that commit)
        if (count > 1 && !prepared) launch(k_batch_prep, dim3(1), dim3(64), b, w.bctl);
        prepared = count > 1;
        launch(k_move_setup, grid_w, blk, g, cost, L, potts, tu.reduce_rounds > 0 ? 1 : 0, w.label, w.cur_cost, b, spw);
        if (tu.reduce_launches > 1) launch(k_reduce<false>, grid_w, blk, g, L, b, tu.reduce_rounds, 1, spw);
        launch(k_reduce<true>, grid_w, blk, g, L, b, tu.reduce_rounds, tu.reduce_launches > 1 ? 0 : 1, spw);
        if (tu.reduce_rounds > 0) stats.reduce_launches += tu.reduce_launches > 1 ? 2 : 1;
        if (count == 1 && w.comp_out && t0 < w.comp_moves)             // diagnostic: components of the core the reduction left
            launch.uncounted(k_core_components, dim3(1), dim3(1024), g, L, t0, ctx0.decided, ctx0.flags, w.comp_scratch,
                             w.comp_scratch + g.n, w.comp_out + 16 * (size_t)t0);
        launch.solve(sl, g, L, b, sp);
        injected_ctx = -1;
        if (++group == w.hooks.inject_group && w.hooks.inject_ctx < count) {        // test hook (mh_set_tuning key 40): the solve "did not converge"
            if (hipError_t e = hipMemsetD32Async((hipDeviceptr_t)(b.c[w.hooks.inject_ctx].flags + C_ERROR), ERR_NO_CONVERGENCE, 1, s); e != hipSuccess) return e;
            injected_ctx = w.hooks.inject_ctx;
        }
        launch(k_delta, grid_d, blk, g, cost, L, potts, w.label, w.cur_cost, b, spw_d);
        if (count > 1) {
            launch(k_batch_check, dim3(32, (unsigned)count), blk, g, cost, L, potts, w.label, w.cur_cost, b, w.bctl);
            launch(k_batch_commit, dim3(32), blk, cost, L, w.label, w.cur_cost, b, w.bctl, w.h_batch_dev, all_flags, n_ctx);
        }
        return hipGetLastError();
    };

    // Batches: only with contexts to run them in, a label set worth it (the planner's rule), and none of the per-move
    // diagnostics that look at context 0's state between the launches of a move.
    const bool can_batch = n_ctx > 1 && w.bctl && w.h_batch && L >= 2 && !w.comp_out;
    if (can_batch) {
        RET_IF(hipMemsetAsync(w.bctl, 0, sizeof(int) * B_WORDS, s));
        w.h_batch[HB_SEQ] = 0;                          // (no commit of an earlier expansion is in flight: each one ends behind a stream wait)
    }
    ExpandPlan plan(L, can_batch ? n_ctx : 1, tu.batch_min_labels);
    int batch_seq = 0;                                  // batches enqueued = the sequence number the next commit publishes (bctl[B_SEQ] starts at 0)
    for (;;) {
        old_energy = energy;
        while (!plan.cycle_done()) {
            const ExpandPlan::Step step = plan.next();
            if (step.kind == ExpandPlan::Kind::skip_rest) {
                stats.moves += step.count; stats.host_skipped += step.count;
                continue;
            }
            if (step.kind == ExpandPlan::Kind::solo) {
                RET_IF(enqueue_moves(step.alpha, step.t, 1, plan.cycle()));
                ++stats.moves; ++stats.solo_moves;
                continue;
            }
            // the batch's moves all read the labeling: it is brought up to date first
            if (step.apply_pending) launch(k_apply_pending, grid1, blk, g.n, cost, L, w.label, w.cur_cost, ctx0.took, ctx0.flags, 1);
            RET_IF(enqueue_moves(step.alpha, step.t, step.count, plan.cycle()));
            ++stats.batches;
            ++stats.host_syncs;
            RET_IF(await_commit(w.h_batch, ++batch_seq, s));
            if (w.h_batch[HB_ERROR]) break;                           // the cycle's end reports it
            // Move j failed its test (j < B): it heads the next batch — a batch's first move has no predecessor to be tested
            // against, so every batch keeps at least one move and no move is ever run twice in a row.  What came behind it
            // in this batch is solved again there.
            const int j = w.h_batch[HB_FIRST_INVALID];
            if (injected_ctx >= j) ++stats.injected_discarded;          // (key 40: the marked move was thrown away, not reported)
            stats.moves += j; stats.batch_committed += j;
            if (j < step.count) ++stats.batch_invalid;
            plan.committed(j, w.h_batch[HB_TLAST]);
        }
        launch(k_apply_pending, grid1, blk, g.n, cost, L, w.label, w.cur_cost, ctx0.took, ctx0.flags, 0);
        launch(k_energy, grid, blk, g, potts, w.label, w.cur_cost, ctx0.flags, ctx0.acc);
        RET_IF(finish_cycle());
        stats.cycles = plan.cycle();
        if (w.h_flags[C_ERROR]) return ended(status_of(w.h_flags[C_ERROR]));
        plan.cycle_ended(w.h_flags[C_TLAST]);
        energy = w.h_acc[A_ENERGY];
        if (energy == old_energy || plan.cycle() > max_cycles) break;               // :1045
    }
    stats.energy = energy;
    stats.accepted = w.h_flags[C_ACCEPTED];
    stats.flow_moves = w.h_flags[C_FLOW_MOVES];
    stats.moves_solved = w.h_flags[C_MOVES_SOLVED];
    stats.moves_run = w.h_flags[C_MOVES_RUN];
    stats.core_sites = w.h_acc[A_CORE_SUM];
    stats.core_max = w.h_flags[C_CORE_MAX];
    stats.outer_iterations = w.h_acc[A_OUTER];
    stats.relax_intervals = w.h_acc[A_RELAX];
    stats.push_phases = w.h_acc[A_PUSH];
    stats.barriers = w.h_acc[A_BARRIERS];
    stats.solve_ms = (double)w.h_acc[A_TICKS] * 1e-5;  // 100 MHz ticks
    stats.barrier_ms = (double)w.h_acc[A_T_BAR] * 1e-5;
    stats.relax_ms = (double)w.h_acc[A_T_RELAX] * 1e-5;
    stats.push_ms = (double)w.h_acc[A_T_PUSH] * 1e-5;
    stats.tail_ms = (double)w.h_acc[A_T_TAIL] * 1e-5;
    stats.tail_rounds = w.h_acc[A_TAIL_ROUNDS];
    stats.max_barrier_wait_ms = (double)w.h_acc[A_MAX_WAIT] * 1e-5;
    return ended(ExpandStatus::ok);
}

} // namespace mh
