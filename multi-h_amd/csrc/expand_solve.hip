// expand_solve.hip — the persistent solver of the alpha-expansion: the max-flow of a move's undecided core in ONE launch
// (k_solve), with its grid barrier.  The launches in front of and behind it, and the schedule, are expand.hip's.

#include "expand_ctl.hpp"

#include <algorithm>

namespace mh {

// ---------------------------------------------------------------------------
// k_solve — the flow problem of one move on the compacted core, in ONE launch.
//
// SLPN = 8 lanes per site, SSLOTS = 6 arcs per lane in registers (degree <= 48; larger sites walk
// their arcs in memory), 512 threads = 64 sites per workgroup, P = ceil(K / 64) workgroups take part
// (the rest of the launch returns at once).  When K exceeds what the launch can hold one site per
// row, rows walk several sites and reload them at every visit.
//
// The cost of this kernel is the number of uncoalesced agent-scope requests a CU issues per round
// (about one 64-B request per clock and CU, whatever the payload) times the rounds a move needs, so
// both phases are written as "poll ONE word per site, act only when it changed":
//   * global relabel = frontier BFS from the sink: a site whose height word dropped since it last
//     told its neighbours lowers THEIR words with atomicMin (no return value) along the arcs that
//     are residual towards it.  Idle sites cost one load per round; every height drops a few times.
//   * push: what other sites have sent to u accumulates in excess[u] (atomicAdd without return, issued
//     by the pusher); what u itself has spent — sent on or drained into the sink — is a register of
//     its owner.  An idle site polls excess[u]; only a site that owns excess loads its neighbours'
//     heights and the counters of the reverse arcs.
// Arc state is SINGLE-WRITER: arc k = (u->v) carries the cumulative counter sent[k] that only u's
// row writes, and r(u->v) = cap[k] - sent[k] + sent[rev k].  A counter read late only under-states
// the residual capacity, so a row never pushes more than an arc holds; it never pushes more than it
// owns either, because only arrivals are asynchronous.  Per cycle a site with excess pushes along
// ALL its downhill residual arcs at once (lanes share the excess through a row prefix sum) or lifts
// itself just above its lowest residual neighbour — Hong's lock-free push-relabel rule per arc.
// (Earlier versions: atomics on shared excess/capacity words with the owner's atomic -> load chain,
// 35-57 ms of solver time per LabelingStep at 50k sites; every lane loading all its neighbours'
// words every cycle, 66 ms.)
//
// Everything another row may read is written with agent-scope (sc1) stores or atomics and read with
// agent-scope loads; before a barrier every wave drains its memory operations (s_waitcnt vmcnt(0)),
// so no cache maintenance is needed (MI355X_MICROARCH.md, valid hand-off forms).  The barrier is one
// monotonic arrival counter polled by one lane per workgroup; the reductions every phase needs ("did
// any row change anything", "how many rows are active", "largest finite height") travel through a
// ring of four slots.
// ---------------------------------------------------------------------------
constexpr int SLPN = 8;
constexpr int SSLOTS = 6;
constexpr int SOLVE_THREADS = 512;
constexpr int SOLVE_ROWS = SOLVE_THREADS / SLPN;
constexpr int H_SHIFT = 24, H_MASK = (1 << H_SHIFT) - 1, H_EPOCHS = 126;   // height word = (H_EPOCHS - epoch) << 24 | height


// Grid barrier with reductions, two levels: the workgroups of one XCD meet on a line of their own, the last
// arriver of each XCD carries the XCD's reductions to the top line and arrives there, everybody polls the top
// counter.  Which XCD a workgroup runs on is read from the hardware (HW_REG_XCC_ID); the census of the first
// barrier (a flat one) tells every workgroup how many partners its XCD has.  Placement only affects speed.
struct GridBarrier {
    int* flags;
    int* s_red;          // shared int[8]: wg changed, wg active, wg hmax, out changed, out active, out hmax, abort
    int P;               // participating workgroups
    int xcd, xcd_wgs, xcds;
    unsigned seq;        // barriers passed on the two-level counters
    unsigned long long ticks;
    unsigned long long timeout;      // 100 MHz ticks a poll may last before the launch gives up (a workgroup is not resident)
    unsigned long long timeout_first;   // ... at the FIRST barrier of a launch, which waits for every workgroup to become resident: on a
                                        // shared GPU a delayed dispatch is not a missing workgroup (r04 advisor finding)
    unsigned long long max_wait;     // longest poll of this workgroup's leader so far
};

__device__ __forceinline__ bool spin_until(const int* word, int target, int* flags, unsigned long long timeout)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
    while (LD(word) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t0 > timeout) {               // a workgroup of this launch is not resident
            atomicExch(&flags[C_ERROR], ERR_BARRIER_TIMEOUT);
            return false;
        }
    }
    return true;
}

// First barrier of a launch: flat, doubles as the census.
__device__ __forceinline__ bool grid_sync_first(GridBarrier& b)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // a core of at most 64 sites: the workgroup's own barrier is the grid's.  Up to 32 workgroups: the barriers are flat (one
    // counter, no per-XCD level), so nobody needs the census, and the first barrier of the cascade orders what this one would
    if (b.P <= 32) { b.xcds = 1; b.xcd_wgs = 1; return true; }
    if (threadIdx.x == 0) {
        b.s_red[6] = 0;
        atomicAdd(&b.flags[C_XCD + b.xcd * C_LINE], 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        atomicAdd(&b.flags[C_ARRIVE], 1);
        if (!spin_until(&b.flags[C_ARRIVE], b.P, b.flags, b.timeout_first)) b.s_red[6] = 1;
        int used = 0;
        for (int x = 0; x < 8; ++x) used += LD(&b.flags[C_XCD + x * C_LINE]) > 0 ? 1 : 0;
        b.s_red[3] = used;
        b.s_red[4] = LD(&b.flags[C_XCD + b.xcd * C_LINE]);
    }
    __syncthreads();
    b.xcds = b.s_red[3];
    b.xcd_wgs = b.s_red[4];
    return b.s_red[6] == 0;
}

// c_changed: any lane of the workgroup; c_active: counted per lane (a site contributes through ONE lane);
// c_hmax: any lane (largest value wins; a scheduling hint only, so it travels outside the ordered path).
// Arrival and reductions share ONE 64-bit word per level and barrier (bits 0-15 arrivals, 16-31 workgroups that
// changed something, 32-63 active sites): a workgroup pays one returning atomic, the last of an XCD one more, and
// the load that sees the last arrival also carries the sums.
__device__ __forceinline__ bool grid_sync(GridBarrier& b, bool c_changed, bool c_active, int c_hmax,
                                          int& any_changed, int& n_active, int& hmax)
{
    typedef unsigned long long u64;
    const u64 t_in = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // every wave: my stores and atomics have landed
    if (threadIdx.x == 0) { b.s_red[0] = 0; b.s_red[1] = 0; b.s_red[2] = 0; }
    __syncthreads();
    if (__ballot(c_changed) && (threadIdx.x & 63) == 0) b.s_red[0] = 1;
    { const u64 b1 = __ballot(c_active); if (b1 && (threadIdx.x & 63) == 0) atomicAdd(&b.s_red[1], __popcll(b1)); }
    if (c_hmax > 0) atomicMax(&b.s_red[2], c_hmax);
    __syncthreads();
    if (b.P == 1) {                                             // one workgroup: nothing leaves the CU
        any_changed = b.s_red[0];
        n_active = b.s_red[1];
        hmax = b.s_red[2];
        __syncthreads();                                        // everybody has read before the next barrier clears the words
        ++b.seq;
        b.ticks += __builtin_amdgcn_s_memrealtime() - t_in;
        return true;
    }
    if (threadIdx.x == 0) {
        const int slot = (int)(b.seq & 3u), next = (int)((b.seq + 2u) & 3u);
        int* mine = b.flags + C_XCD + b.xcd * C_LINE;
        int* top = b.flags + C_TOP;
        u64* xs = (u64*)(mine + 2);
        u64* ts = (u64*)(top + 2);
        if (b.s_red[2]) {
            atomicMax(&top[10 + slot], b.s_red[2]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const u64 me = 1ull | ((u64)(b.s_red[0] ? 1 : 0) << 16) | ((u64)(unsigned)b.s_red[1] << 32);
        const bool flat = b.P <= 32;                            // few workgroups: one level is a round trip shorter
        if (flat) {
            atomicAdd(&ts[slot], me);
        } else {
            const u64 old = atomicAdd(&xs[slot], me);
            if ((int)(old & 0xffffull) + 1 == b.xcd_wgs) {      // last of my XCD: carry its sums up
                atomicAdd(&ts[slot], ((old + me) & ~0xffffull) | 1ull);
                ST(&xs[next], 0ull);                            // my XCD's word of the barrier after next
            }
        }
        const int target = flat ? b.P : b.xcds;
        u64 v = 0;
        int hm = 0;
        const u64 t0 = __builtin_amdgcn_s_memrealtime();
        const u64 limit = b.seq == 0 ? b.timeout_first : b.timeout;          // (launches of at most 32 workgroups meet here first)
        int abort = 0;
        for (;;) {
            v = LD(&ts[slot]);
            hm = LD(&top[10 + slot]);
            if ((int)(v & 0xffffull) >= target) break;
            __builtin_amdgcn_s_sleep(1);
            if (__builtin_amdgcn_s_memrealtime() - t0 > limit) {             // a workgroup of this launch is not resident
                atomicExch(&b.flags[C_ERROR], ERR_BARRIER_TIMEOUT);
                abort = 1;
                break;
            }
        }
        { const u64 waited = __builtin_amdgcn_s_memrealtime() - t0; if (b.seq != 0 && waited > b.max_wait) b.max_wait = waited; }    // (steady-state waits only)
        b.s_red[3] = (int)((v >> 16) & 0xffffull);
        b.s_red[4] = (int)(v >> 32);
        b.s_red[5] = hm;
        b.s_red[6] = abort;
        if (blockIdx.x == 0) { ST(&ts[next], 0ull); ST(&top[10 + next], 0); }
    }
    __syncthreads();
    any_changed = b.s_red[3];
    n_active = b.s_red[4];
    hmax = b.s_red[5];
    ++b.seq;
    b.ticks += __builtin_amdgcn_s_memrealtime() - t_in;
    return b.s_red[6] == 0;
}

// per-site state of the rows' sites, in LDS: [field][slot][row of the workgroup]
enum { F_SITE = 0, F_HPROP, F_SPENT, F_SC, F_HU, F_SINK0, F_FIELDS };

// The solver proper.  MULTI = false: the core fits the launch one site per row — the site stays in registers for the
// whole move and nothing below touches LDS.  MULTI = true: rows own several sites (see `cur` below).
template <bool MULTI>
__device__ __forceinline__ void
solve_body(const Graph& g, int t, int* cap, int* sent, int* excess, int* sink_cap, int* height, int* decided,
           const int* __restrict__ core, int* flags, long long* acc, int* __restrict__ trace, int* __restrict__ detail,
           int* __restrict__ saved_flow, int* __restrict__ saved_sink, int warm, int mslots, const SolveParams& sp,
           int* s_priv, int* s_red, const int (&pre)[EXPAND_CORE_SHARDS + 1], int K, int P)
{
    const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
    const unsigned long long tick0 = __builtin_amdgcn_s_memrealtime();
    const int total_rows = P * SOLVE_ROWS;
    const int lr = threadIdx.x / SLPN;               // my row inside the workgroup
    const int row = blockIdx.x * SOLVE_ROWS + lr;
    const int sub = threadIdx.x % SLPN;
    // A row owns the core sites row, row + total_rows, ...: S of them ("slots"; one when the core fits the launch).
    const int S = row < K ? (MULTI ? (K - row + total_rows - 1) / total_rows : 1) : 0;
    if ((K + total_rows - 1) / total_rows > mslots) {            // (the host sizes mslots for a core of all n sites)
        if (threadIdx.x == 0) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
        return;
    }
    const int INF = K + 1;                           // no residual path in the core is longer than K
    // HW_REG_XCC_ID (id 20), bits 3:0: the XCD this workgroup runs on
    const int xcc = (int)(__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u);
    GridBarrier bar{ flags, s_red, P, xcc, 1, 1, 0u, 0ull, sp.barrier_timeout, sp.barrier_first_timeout, 0ull };
    long long st_outer = 0, st_relax = 0, st_push = 0;
    unsigned long long tk_relax = 0, tk_push = 0, tk_tail = 0;
    long long st_tail = 0;                           // relabel/push rounds that began with fewer than 64 active rows
#define PRIV(field, slot) s_priv[((field) * mslots + (slot)) * SOLVE_ROWS + lr]
#define CUR(slot) (!MULTI || (slot) == cur)

    // ONE site at a time lives in registers (`cur` = its slot): head, then on demand neighbours, arc state and the
    // relabel mask, plus the site's scalars.  The scalars of the other slots wait in LDS; all lanes of a row hold
    // identical copies and write identical values.  Sites are polled through ONE word (height or excess) and
    // entered only when that word says there is something to do, so a row with several sites costs one load per
    // site and round like a row with one.  (The first version of the several-sites case reloaded every site at
    // every visit and gave every BFS level a grid barrier of its own: 203 ms for one 18 313-site move.)
    int cur = -1, u = -1, k0 = 0, k1 = 0, dec = 3;
    int hu = 0, sc = 0, spent = 0, hprop = 0, sink0 = 0;
    bool fast = false, nb_ok = false, arcs_ok = false, rin_ok = false, priv_live = false;
    int nb[SSLOTS], rv[SSLOTS], c0[SSLOTS], so[SSLOTS];
    unsigned rin = 0;                                // bit q: the arc nb[q] -> u is residual (relabel direction)

    auto enter = [&](int slot) {
        if (cur == slot) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the counters I stored for the site I leave are read back when I return
        if (cur >= 0 && priv_live) { PRIV(F_HPROP, cur) = hprop; PRIV(F_SPENT, cur) = spent; PRIV(F_SC, cur) = sc; PRIV(F_HU, cur) = hu; }
        cur = slot;
        const int c = row + slot * total_rows;
        int s = 0, first = 0;
#pragma unroll
        for (int q = 1; q < EXPAND_CORE_SHARDS; ++q) if (c >= pre[q]) { s = q; first = pre[q]; }
        u = core[(size_t)s * g.n + (c - first)];
        k0 = g.rowptr[u];
        k1 = g.rowptr[u + 1];
        fast = (k1 - k0) <= SLPN * SSLOTS;
        dec = LD(&decided[u]);
        nb_ok = arcs_ok = rin_ok = false;
        if (priv_live) { hprop = PRIV(F_HPROP, slot); spent = PRIV(F_SPENT, slot); sc = PRIV(F_SC, slot); hu = PRIV(F_HU, slot); sink0 = PRIV(F_SINK0, slot); }
    };
    auto need_nbrs = [&]() {
        if (nb_ok) return;
#pragma unroll
        for (int q = 0; q < SSLOTS; ++q) {
            const int k = k0 + sub + q * SLPN;
            const bool in = fast && k < k1;
            nb[q] = in ? g.col[k] : -1;
            rv[q] = in ? g.rev[k] : 0;
            c0[q] = 0; so[q] = 0;
        }
        nb_ok = true;
    };
    // capacities (final once the reduction has reached its fixed point) and the row's own counters; arcs
    // without capacity in either direction (decided neighbours) drop out
    auto need_arcs = [&]() {
        need_nbrs();
        if (arcs_ok) return;
        if (fast) {
#pragma unroll
            for (int q = 0; q < SSLOTS; ++q) {
                if (nb[q] >= 0) {
                    const int k = k0 + sub + q * SLPN;
                    c0[q] = LD(&cap[k]);
                    so[q] = LD(&sent[k]);
                    if ((c0[q] | LD(&cap[rv[q]])) == 0) nb[q] = -1;
                }
            }
        }
        arcs_ok = true;
    };
    auto need_rin = [&]() {                          // arcs residual TOWARDS me, constant between two push phases
        need_arcs();
        if (rin_ok) return;
        rin = 0;
        if (fast) {
#pragma unroll
            for (int q = 0; q < SSLOTS; ++q)
                if (nb[q] >= 0 && LD(&cap[rv[q]]) - LD(&sent[rv[q]]) + so[q] > 0) rin |= 1u << q;
        }
        rin_ok = true;
    };
#define FOR_MY_SLOTS(slot) for (int slot = 0; slot < S; ++slot)
    int site0 = -1;                                  // PRIV(F_SITE, 0): the undecided site of slot 0, or -1
#define SITE_OF(slot) ((!MULTI || (slot) == 0) ? site0 : PRIV(F_SITE, slot))

    // my arcs' flow counters start at zero (visible to everybody behind the barriers of phase 0)
    FOR_MY_SLOTS(slot) {
        enter(slot);
        if (!warm) for (int k = k0 + sub; k < k1; k += SLPN) ST(&sent[k], 0);
        if (sub == 0) ST(&height[u], 0x7fffffff);     // a word of no epoch
    }
    if (!grid_sync_first(bar)) return;

    // ---- phase 0: the reduction cascade to its fixed point (k_reduce's body on the core) -------------
    int cascade_pass = 0;
    for (;;) {
        // (a capped cascade ends with a pass that only folds: every verdict taken before it is then folded into its
        // undecided neighbours, which is what the flow phase relies on — decided sites are not part of its graph)
        const bool fold_only = sp.cascade_iters > 0 && cascade_pass + 1 >= sp.cascade_iters;
        bool changed = false;
        FOR_MY_SLOTS(slot) {
            enter(slot);
            if (MULTI) dec = LD(&decided[u]);          // (a row with one site keeps its verdict in the register)
            if (dec != 0) continue;
            long long net = (long long)LD(&excess[u]) - LD(&sink_cap[u]);
            bool dirty = false;
            int verdict = 0;
            for (int r = 0; r < sp.reduce_rounds; ++r) {
                long long add = 0, out = 0, in = 0;
                for (int k = k0 + sub; k < k1; k += SLPN) {
                    const int kr = g.rev[k];
                    const int co = LD(&cap[k]), ci = LD(&cap[kr]);
                    if ((co | ci) == 0) continue;
                    const int dv = LD(&decided[g.col[k]]);
                    if (dv == 1) { add += ci; ST(&cap[k], 0); ST(&cap[kr], 0); }
                    else if (dv == 2) { add -= co; ST(&cap[k], 0); ST(&cap[kr], 0); }
                    else { out += co; in += ci; }
                }
                add = row_sum64<SLPN>(add); out = row_sum64<SLPN>(out); in = row_sum64<SLPN>(in);
                if (add != 0) { net += add; dirty = true; changed = true; }
                if (fold_only) break;                 // the capped cascade's last pass: no new verdicts, so none is left unfolded
                if (net > out) verdict = 1;
                else if (-net > in) verdict = 2;
                if (verdict || add == 0) break;       // a round that folded nothing would repeat itself
            }
            if (sub == 0) {
                if (dirty) {
                    if (net > 0x7fffffffll || -net > 0x7fffffffll) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
                    ST(&excess[u], net > 0 ? (int)net : 0);
                    ST(&sink_cap[u], net < 0 ? (int)(-net) : 0);
                }
                if (verdict) ST(&decided[u], verdict);
            }
            if (verdict) { dec = verdict; changed = true; }
        }
        int any, nact, hm;
        if (!grid_sync(bar, changed && sub == 0, false, 0, any, nact, hm)) return;
        if (!any || sp.reduce_rounds <= 0) break;
        // The cascade is exact but optional: a site it would still decide stays in the flow problem, whose read-out gives it
        // the same side.  A cap trades its barrier-separated passes against a slightly larger flow problem.
        if (fold_only) break;
        ++cascade_pass;
    }

    // ---- flow recycling: start from what the previous expansion on this label left in the arcs ----------
    // saved_flow[k] = net flow the arc carried when that move ended, saved_sink[u] = what u drained into the sink.
    // Clipped to this move's capacities they are a feasible pseudo-flow: every arc counter lies in [0, cap], so
    // cap - sent + sent[rev] stays within the pair's total.  A site left owing flow (it sends on more than it owns)
    // gets the missing amount as source supply AND as sink capacity — the same constant on both t-links changes the
    // value of every cut alike (Kohli & Torr's reparametrisation) — so excess is never negative.  A maximum flow
    // from any feasible start has the same residual reachability, so the read-out (hence every label) is unchanged;
    // only the number of relabel/push rounds is, as later cycles re-solve almost the same problem.
    if (warm) {
        FOR_MY_SLOTS(slot) {
            enter(slot);
            if (MULTI) dec = LD(&decided[u]);
            if (dec != 0) continue;
            for (int k = k0 + sub; k < k1; k += SLPN) {
                const int f = saved_flow[k], ck = LD(&cap[k]);
                ST(&sent[k], f < ck ? f : ck);
            }
        }
        int a0, a1, a2;
        if (!grid_sync(bar, false, false, 0, a0, a1, a2)) return;
    }
    FOR_MY_SLOTS(slot) {
        enter(slot);
        if (MULTI) { dec = LD(&decided[u]); PRIV(F_SITE, slot) = dec == 0 ? u : -1; }
        else site0 = dec == 0 ? u : -1;
        if (dec != 0) continue;
        int sc_s = LD(&sink_cap[u]), spent_s = 0, sink0_s = sc_s;
        if (warm) {
            long long net = 0;                            // what my arcs carry away, net
            for (int k = k0 + sub; k < k1; k += SLPN) {
                const int kr = g.rev[k];
                if ((LD(&cap[k]) | LD(&cap[kr])) == 0) continue;      // decided neighbour: folded, and its counter is not maintained
                net += (long long)LD(&sent[k]) - LD(&sent[kr]);
            }
            net = row_sum64<SLPN>(net);
            const int sv = saved_sink[u];
            const int sf = sv < sc_s ? sv : sc_s;
            sc_s -= sf;
            long long own = (long long)sf + net;
            const long long e = (long long)LD(&excess[u]) - own;
            if (e < 0) {
                own += e;
                const long long s2 = (long long)sc_s - e;
                if (s2 > (1 << 30)) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
                sc_s = (int)s2;
            }
            spent_s = (int)own;
            sink0_s = sc_s + sf;
            if (sub == 0) ST(&sink_cap[u], sc_s);
        }
        if (MULTI) {
            PRIV(F_SC, slot) = sc_s; PRIV(F_SPENT, slot) = spent_s; PRIV(F_SINK0, slot) = sink0_s;
            PRIV(F_HPROP, slot) = INF; PRIV(F_HU, slot) = INF;
        } else {
            sc = sc_s; spent = spent_s; sink0 = sink0_s; hprop = INF; hu = INF;
        }
    }
    // from here on the scalars of the site in registers are live (written back when the row turns to another site)
    if (MULTI) {
        site0 = S > 0 ? PRIV(F_SITE, 0) : -1;
        if (cur >= 0) { hprop = PRIV(F_HPROP, cur); spent = PRIV(F_SPENT, cur); sc = PRIV(F_SC, cur); hu = PRIV(F_HU, cur); sink0 = PRIV(F_SINK0, cur); }
        priv_live = true;
    }
    arcs_ok = rin_ok = false;
    if (!MULTI && site0 >= 0) need_arcs();

    // ---- phase 1: global relabel <-> push until no site with excess can reach the sink ---------------
    int outer = 0, epoch = 0, hprev = 4;
    for (;; ++outer) {
        if (outer >= sp.max_outer) { if (leader) atomicExch(&flags[C_ERROR], ERR_NO_CONVERGENCE); break; }
        ++st_outer;
        const unsigned long long tr0 = __builtin_amdgcn_s_memrealtime();
        // Global relabel.  Height words carry the relabel's epoch in their top bits, newer epochs SMALLER: a word of
        // an older epoch reads as "unreachable" and loses against any atomicMin of the running epoch, so a relabel
        // needs no pass that resets the words, and the sites next to the sink enter with an atomicMin of their own.
        if (++epoch > H_EPOCHS) {                      // out of epochs (never seen): start over behind two barriers
            int a0, a1, a2;
            if (!grid_sync(bar, false, false, 0, a0, a1, a2)) return;
            FOR_MY_SLOTS(slot) { const int us = SITE_OF(slot); if (us >= 0 && sub == 0) ST(&height[us], 0x7fffffff); }
            if (!grid_sync(bar, false, false, 0, a0, a1, a2)) return;
            epoch = 1;
        }
        const int ebits = (H_EPOCHS - epoch) << H_SHIFT;
        rin_ok = false;                                // the pushes since the last relabel moved the residual capacities
        FOR_MY_SLOTS(slot) {
            const int us = SITE_OF(slot);
            if (us < 0) continue;
            const int sc_s = CUR(slot) ? sc : PRIV(F_SC, slot);
            if (sc_s > 0 && sub == 0) atomicMin(&height[us], ebits | 1);
            if (CUR(slot)) hprop = INF; else PRIV(F_HPROP, slot) = INF;      // nothing told to the neighbours yet
        }
        // the site in registers has its relabel mask ready before the frontier arrives (a mask computed on arrival
        // puts a dozen dependent loads between hearing and telling: every BFS level took twice as long)
        if (MULTI ? (cur >= 0 && SITE_OF(cur) >= 0) : (site0 >= 0)) need_rin();
        int any, nact, hmax;
        // (the frontier advances one level per round: a few rounds more than the last relabel was deep)
        int relax_rounds = hprev + 12;
        if (relax_rounds > sp.relax_rounds) relax_rounds = sp.relax_rounds;
        // ... then the frontier runs: a site whose word dropped since it last spoke lowers its upstream
        // neighbours' words to its height + 1.  Words only decrease and every value is realised by a residual
        // path, so any schedule converges to the BFS distances; an interval without a single announcement is
        // the fixed point (all atomics of earlier intervals had landed before it began).
        for (;;) {
            ++st_relax;
            bool spoke = false, active = false;
            int my_h = 0;
            for (int r = 0; r < relax_rounds; ++r) {
                bool settled = true;                  // every site of mine next to the sink and announced: final
                FOR_MY_SLOTS(slot) {
                    const int us = SITE_OF(slot);
                    if (us < 0) continue;
                    const int w = LD(&height[us]);
                    const int h = (w >> H_SHIFT) == (ebits >> H_SHIFT) ? (w & H_MASK) : INF;
                    const int hp = CUR(slot) ? hprop : PRIV(F_HPROP, slot);
                    if (h < hp) {
                        if (MULTI) { enter(slot); need_rin(); }
                        if (fast) {
#pragma unroll
                            for (int q = 0; q < SSLOTS; ++q)
                                if (rin & (1u << q)) atomicMin(&height[nb[q]], ebits | (h + 1));
                        } else {
                            for (int k = k0 + sub; k < k1; k += SLPN) {
                                const int kr = g.rev[k];
                                const int ckr = LD(&cap[kr]);
                                if ((LD(&cap[k]) | ckr) == 0) continue;      // folded arc: the neighbour is decided, its counter is stale
                                if (ckr - LD(&sent[kr]) + LD(&sent[k]) > 0) atomicMin(&height[g.col[k]], ebits | (h + 1));
                            }
                        }
                        hprop = h;
                        spoke = true;
                        settled = false;
                    } else if (h > 1) settled = false;
                    if (CUR(slot)) hu = h; else PRIV(F_HU, slot) = h;
                }
                if (settled) break;
            }
            FOR_MY_SLOTS(slot) {
                const int us = SITE_OF(slot);
                if (us < 0) continue;
                const int h = CUR(slot) ? hu : PRIV(F_HU, slot);
                if (h < INF) {
                    if (h > my_h) my_h = h;
                    if (sub == 0 && LD(&excess[us]) - (CUR(slot) ? spent : PRIV(F_SPENT, slot)) > 0) active = true;
                }
            }
            if (!grid_sync(bar, spoke, active, my_h, any, nact, hmax)) return;
            // no announcement in a whole interval: the distances are exact.  Otherwise every finite height is still
            // realised by a residual path, which is all the pushes need: go on as soon as somebody can push.
            if (!any || nact) break;
        }
        hprev = hmax;
        tk_relax += __builtin_amdgcn_s_memrealtime() - tr0;
        if (detail && leader && outer < 2048) {
            int* d = detail + 4 * (size_t)outer;
            d[0] = nact; d[1] = hmax; d[2] = (int)st_relax; d[3] = (int)(__builtin_amdgcn_s_memrealtime() - tick0);
        }
        if (nact == 0) break;                          // (then exact) finished: nobody with excess reaches the sink
        const bool tail_round = nact < 64;
        if (outer == 0 && leader) atomicAdd(&flags[C_FLOW_MOVES], 1);

        // lock-free push-relabel (see the header of this kernel); a wave of pushes needs about as many cycles
        // as the longest residual path is long
        const unsigned long long tp0 = __builtin_amdgcn_s_memrealtime();
        int cycles = sp.push_mult * (hmax + 3);
        if (cycles > sp.push_cycles) cycles = sp.push_cycles;
        for (int phase = 0; phase < sp.push_phases; ++phase) {
            ++st_push;
            bool active = false;
            FOR_MY_SLOTS(slot) {                      // my words as the last announcements left them
                const int us = SITE_OF(slot);
                if (us < 0) continue;
                const int w = LD(&height[us]);
                const int h = (w >> H_SHIFT) == (ebits >> H_SHIFT) ? (w & H_MASK) : INF;
                if (CUR(slot)) hu = h; else PRIV(F_HU, slot) = h;
            }
            for (int cyc = 0; cyc < cycles; ++cyc) {
                bool alive = false;                   // somebody of mine can still reach the sink
                FOR_MY_SLOTS(slot) {
                    const int us = SITE_OF(slot);
                    if (us < 0) continue;
                    if ((CUR(slot) ? hu : PRIV(F_HU, slot)) >= INF) continue;
                    alive = true;
                    const int x = LD(&excess[us]);
                    if (x > (1 << 30)) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
                    if (x - (CUR(slot) ? spent : PRIV(F_SPENT, slot)) <= 0) continue;      // idle: poll again
                    if (MULTI) { enter(slot); need_arcs(); }
                    int e = x - spent;
                    if (sc > 0) {                                   // t-link: h(t) = 0, h(u) >= 1
                        const int d = e < sc ? e : sc;
                        sc -= d; spent += d; e -= d;
                        if (sub == 0) ST(&sink_cap[u], sc);
                    }
                    if (e <= 0) continue;
                    if (fast) {
                        int r[SSLOTS], hq[SSLOTS];
#pragma unroll
                        for (int q = 0; q < SSLOTS; ++q) {          // one level of independent loads
                            r[q] = nb[q] >= 0 ? LD(&sent[rv[q]]) : 0;
                            hq[q] = nb[q] >= 0 ? LD(&height[nb[q]]) : 0;
                        }
#pragma unroll
                        for (int q = 0; q < SSLOTS; ++q)
                            hq[q] = (hq[q] >> H_SHIFT) == (ebits >> H_SHIFT) ? (hq[q] & H_MASK) : INF;
                        int D = 0;                                  // what my downhill residual arcs can take
#pragma unroll
                        for (int q = 0; q < SSLOTS; ++q) {
                            r[q] = nb[q] >= 0 ? c0[q] - so[q] + r[q] : 0;
                            if (r[q] > 0 && hq[q] < hu) D += r[q];
                        }
                        static_assert(SLPN == 8, "the prefix below is row_shr 1, 2, 4: complete for rows of 8 lanes only (16 would need a row_shr 8 step)");
                        // (the lanes of a row are convergent here and at every row_min / row_sum: the DPP moves use bound_ctrl,
                        // a lane switched off by EXEC would read as 0)
                        int incl = D;                               // prefix over the row's lanes: row_shr 1, 2, 4
                        { const int y = dpp_mov<0x111>(incl); if (sub >= 1) incl += y; }
                        { const int y = dpp_mov<0x112>(incl); if (sub >= 2) incl += y; }
                        { const int y = dpp_mov<0x114>(incl); if (sub >= 4) incl += y; }
                        const int tot = row_sum<SLPN>(D);
                        if (tot > 0) {
                            int budget = e - (incl - D);            // the lanes in front of me are served first
                            if (budget > D) budget = D;
#pragma unroll
                            for (int q = 0; q < SSLOTS; ++q) {
                                if (budget > 0 && r[q] > 0 && hq[q] < hu) {
                                    const int d = r[q] < budget ? r[q] : budget;
                                    so[q] += d;
                                    budget -= d;
                                    ST(&sent[k0 + sub + q * SLPN], so[q]);
                                    atomicAdd(&excess[nb[q]], d);
                                    if (so[q] > (1 << 30)) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
                                }
                            }
                            spent += e < tot ? e : tot;
                        } else {                                    // nothing downhill: lift just above the lowest residual neighbour
                            int hmin = INF;
#pragma unroll
                            for (int q = 0; q < SSLOTS; ++q) if (r[q] > 0 && hq[q] < hmin) hmin = hq[q];
                            hmin = row_min<SLPN>(hmin);
                            hu = hmin >= INF ? INF : hmin + 1;
                            if (sub == 0) ST(&height[u], ebits | hu);
                        }
                    } else {                                        // any degree: one arc per cycle, arcs walked in memory
                        long long key = 0x7fffffffffffffffll;       // (height << 32) | arc
                        for (int k = k0 + sub; k < k1; k += SLPN) {
                            // An arc whose pair has no capacity left leads to a neighbour decided in this move: it is not in
                            // the graph, and neither its counter (last written in an earlier move) nor its height word
                            // (another move's epoch numbering) means anything here.
                            const int ck = LD(&cap[k]), kr = g.rev[k];
                            if ((ck | LD(&cap[kr])) == 0) continue;
                            if (ck - LD(&sent[k]) + LD(&sent[kr]) > 0) {
                                const int w = LD(&height[g.col[k]]);
                                const int hv = (w >> H_SHIFT) == (ebits >> H_SHIFT) ? (w & H_MASK) : INF;
                                const long long cand = ((long long)hv << 32) | (unsigned int)k;
                                if (cand < key) key = cand;
                            }
                        }
                        key = row_min64<SLPN>(key);
                        if (key == 0x7fffffffffffffffll) {          // no way out at all
                            hu = INF;
                            if (sub == 0) ST(&height[u], ebits | hu);
                            continue;
                        }
                        const int hmin = (int)(key >> 32), kmin = (int)(key & 0xffffffffll);
                        if (hu > hmin) {
                            const int a = LD(&sent[kmin]);
                            const int rr = LD(&cap[kmin]) - a + LD(&sent[g.rev[kmin]]);
                            const int d = e < rr ? e : rr;
                            if (sub == 0) {
                                ST(&sent[kmin], a + d);
                                atomicAdd(&excess[g.col[kmin]], d);
                                if (a + d > (1 << 30)) atomicExch(&flags[C_ERROR], ERR_OVERFLOW);
                            }
                            spent += d;
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the next cycle reads the counter back
                        } else {
                            hu = hmin + 1;
                            if (hu > INF) hu = INF;
                            if (sub == 0) ST(&height[u], ebits | hu);
                        }
                    }
                }
                if (!alive) break;
            }
            FOR_MY_SLOTS(slot) {
                const int us = SITE_OF(slot);
                if (us < 0) continue;
                if (sub == 0 && (CUR(slot) ? hu : PRIV(F_HU, slot)) < INF &&
                    LD(&excess[us]) - (CUR(slot) ? spent : PRIV(F_SPENT, slot)) > 0) active = true;
            }
            // this barrier also separates the pushes from the next relabel (the counters are final behind it)
            if (!grid_sync(bar, false, active, 0, any, nact, hmax)) return;
            if (nact == 0) break;
        }
        tk_push += __builtin_amdgcn_s_memrealtime() - tp0;
        if (tail_round) { tk_tail += __builtin_amdgcn_s_memrealtime() - tr0; ++st_tail; }
    }

    // ---- read-out: whoever cannot reach the sink takes alpha ---------------------------------------
    FOR_MY_SLOTS(slot) {
        const int us = SITE_OF(slot);
        if (us < 0) continue;
        const int h = CUR(slot) ? hu : PRIV(F_HU, slot);
        if (sub == 0) ST(&decided[us], h >= INF ? 1 : 2);
        if (saved_flow) {                                 // for the next expansion on this label (the counters are final)
            enter(slot);
            for (int k = k0 + sub; k < k1; k += SLPN) {
                const int kr = g.rev[k];
                int f = 0;
                if ((LD(&cap[k]) | LD(&cap[kr])) != 0) f = LD(&sent[k]) - LD(&sent[kr]);
                saved_flow[k] = f > 0 ? f : 0;
            }
            if (sub == 0) saved_sink[u] = sink0 - sc;
        }
    }
#undef FOR_MY_SLOTS
#undef SITE_OF
#undef CUR
#undef PRIV
    if (leader) {
        atomicAdd(&flags[C_MOVES_SOLVED], 1);
        atomicMax(&flags[C_CORE_MAX], K);
        atomicAdd((unsigned long long*)&acc[A_CORE_SUM], (unsigned long long)K);
        atomicAdd((unsigned long long*)&acc[A_OUTER], (unsigned long long)st_outer);
        atomicAdd((unsigned long long*)&acc[A_RELAX], (unsigned long long)st_relax);
        atomicAdd((unsigned long long*)&acc[A_PUSH], (unsigned long long)st_push);
        atomicAdd((unsigned long long*)&acc[A_BARRIERS], (unsigned long long)bar.seq);
        atomicAdd((unsigned long long*)&acc[A_TICKS], __builtin_amdgcn_s_memrealtime() - tick0);
        atomicAdd((unsigned long long*)&acc[A_T_BAR], bar.ticks);
        atomicAdd((unsigned long long*)&acc[A_T_RELAX], tk_relax);
        atomicAdd((unsigned long long*)&acc[A_T_PUSH], tk_push);
        atomicAdd((unsigned long long*)&acc[A_T_TAIL], tk_tail);
        atomicAdd((unsigned long long*)&acc[A_TAIL_ROUNDS], (unsigned long long)st_tail);
        atomicMax((unsigned long long*)&acc[A_MAX_WAIT], bar.max_wait);
        atomicMax(&flags[C_XCD_USED], bar.xcds);
        if (trace) {
            int* tr = trace + 8 * (size_t)t;
            tr[0] = K; tr[1] = P; tr[2] = (int)st_outer; tr[3] = (int)st_relax; tr[4] = (int)st_push; tr[5] = (int)bar.seq;
            tr[6] = (int)(__builtin_amdgcn_s_memrealtime() - tick0); tr[7] = (int)bar.ticks;
        }
    }
}

__global__ void __launch_bounds__(SOLVE_THREADS)
k_solve(Graph g, int L, MoveBatch b, int mslots, SolveParams sp)
{
    const MoveCtx& c = b.c[blockIdx.y];
    const int t = c.t, warm = c.warm;
    int* cap = c.cap;
    int* sent = c.sent;
    int* excess = c.excess;
    int* sink_cap = c.sink_cap;
    int* height = c.height;
    int* decided = c.decided;
    const int* __restrict__ core = c.core;
    int* flags = c.flags;
    long long* acc = c.acc;
    int* __restrict__ trace = c.trace;
    int* __restrict__ detail = c.detail;
    int* __restrict__ saved_flow = c.saved_flow;
    int* __restrict__ saved_sink = c.saved_sink;
    extern __shared__ int s_priv[];                  // F_FIELDS x mslots x SOLVE_ROWS
    __shared__ int s_red[8];
    __shared__ int s_skip;
    if (threadIdx.x == 0) s_skip = move_is_skipped(flags, t, L) ? 1 : 0;
    __syncthreads();
    if (s_skip) return;
    if (g.n >= H_MASK) { if (threadIdx.x == 0) atomicExch(&flags[C_ERROR], ERR_OVERFLOW); return; }   // heights carry 24 bits
    int pre[EXPAND_CORE_SHARDS + 1];
    pre[0] = 0;
#pragma unroll
    for (int s = 0; s < EXPAND_CORE_SHARDS; ++s) pre[s + 1] = pre[s] + flags[C_CORE + s];
    const int K = pre[EXPAND_CORE_SHARDS];
    if (K == 0) return;
    int P = (K + SOLVE_ROWS - 1) / SOLVE_ROWS;
    if (P > (int)gridDim.x) P = (int)gridDim.x;
    if ((int)blockIdx.x >= P) return;
    if (K <= P * SOLVE_ROWS) solve_body<false>(g, t, cap, sent, excess, sink_cap, height, decided, core, flags, acc, trace, detail,
                                                saved_flow, saved_sink, warm, mslots, sp, s_priv, s_red, pre, K, P);
    else solve_body<true>(g, t, cap, sent, excess, sink_cap, height, decided, core, flags, acc, trace, detail,
                          saved_flow, saved_sink, warm, mslots, sp, s_priv, s_red, pre, K, P);
}

hipError_t solver_blocks_per_cu(int* blocks)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, (const void*)k_solve, SOLVE_THREADS, sizeof(int) * F_FIELDS * SOLVE_ROWS);
}

hipError_t prepare_solve(int n, int solve_grid, SolveLaunch* sl)
{
    sl->grid = solve_grid;
    sl->mslots = std::max(1, (n + solve_grid * SOLVE_ROWS - 1) / (solve_grid * SOLVE_ROWS));
    sl->lds = sizeof(int) * F_FIELDS * (size_t)sl->mslots * SOLVE_ROWS;
    sl->fits = sl->lds <= 128 * 1024;                           // > 1.3 M sites at 256 workgroups
    if (sl->fits && sl->lds > 48 * 1024)
        return hipFuncSetAttribute((const void*)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl->lds);
    return hipSuccess;
}

void launch_solve(const SolveLaunch& sl, const Graph& g, int L, const MoveBatch& b, const SolveParams& sp, hipStream_t s)
{
    hipLaunchKernelGGL(k_solve, dim3((unsigned)sl.grid, (unsigned)b.count), dim3(SOLVE_THREADS), sl.lds, s, g, L, b, sl.mslots, sp);
}

} // namespace mh
