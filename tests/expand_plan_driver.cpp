// Drives the alpha-expansion's move planner (csrc/expand_plan.hpp, nothing else) with seeded outcomes and prints every decision
// for tests/test_expand_plan_cpu.py.  No GPU, no HIP.
//
//   expand_plan_driver L contexts batch_min_labels seed p1 p2 ...      (p_c: per cent of the moves of cycle c that are accepted;
//                                                                        the last one holds for every later cycle)
// Lines:
//   config L contexts min_labels cycles
//   skip  cycle t alpha count | fresh known_tlast
//   solo  cycle t alpha       | fresh known_tlast
//   batch cycle t alpha B apply_pending | fresh known_tlast bsize
//   commit first_invalid tlast | bsize
//   end   cycle tlast
// `fresh known_tlast bsize` are the planner's state BEFORE the decision.  The driver plays the device: a move that is
// idempotent (t >= L and nothing accepted since t - L) is never accepted; a batch of B keeps a first_invalid drawn from 1..B.
#include "expand_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int L = std::atoi(argv[1]), contexts = std::atoi(argv[2]), min_labels = std::atoi(argv[3]);
    unsigned long long rng = std::strtoull(argv[4], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    std::vector<int> pct;
    for (int i = 5; i < argc; ++i) pct.push_back(std::atoi(argv[i]));
    const int cycles = (int)pct.size() + 2;
    auto draw = [&](int below) {          // xorshift64*
        rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
        return (int)(((rng * 0x2545F4914F6CDD1Dull) >> 33) % (unsigned long long)below);
    };
    std::printf("config %d %d %d %d\n", L, contexts, min_labels, cycles);
    mh::ExpandPlan plan(L, contexts, min_labels);
    int tlast = -1;                       // the device's C_TLAST
    auto run_move = [&](int t, int p) {   // one move on the device
        const bool idempotent = t >= L && tlast <= t - L;
        if (!idempotent && draw(100) < p) tlast = t;
    };
    while (plan.cycle() <= cycles) {
        const int cycle = plan.cycle();
        const int p = pct[std::min<size_t>(cycle - 1, pct.size() - 1)];
        while (!plan.cycle_done()) {
            const int fresh = plan.fresh() ? 1 : 0, known = plan.known_tlast(), bsize = plan.bsize();
            const mh::ExpandPlan::Step s = plan.next();
            if (s.kind == mh::ExpandPlan::Kind::skip_rest) {
                std::printf("skip %d %d %d %d | %d %d\n", cycle, s.t, s.alpha, s.count, fresh, known);
            } else if (s.kind == mh::ExpandPlan::Kind::solo) {
                std::printf("solo %d %d %d | %d %d\n", cycle, s.t, s.alpha, fresh, known);
                run_move(s.t, p);
            } else {
                std::printf("batch %d %d %d %d %d | %d %d %d\n", cycle, s.t, s.alpha, s.count, s.apply_pending ? 1 : 0, fresh, known, bsize);
                const int j = 1 + draw(s.count);
                for (int k = 0; k < j; ++k) run_move(s.t + k, p);
                plan.committed(j, tlast);
                std::printf("commit %d %d | %d\n", j, tlast, plan.bsize());
            }
        }
        std::printf("end %d %d\n", cycle, tlast);
        plan.cycle_ended(tlast);
    }
    return 0;
}
