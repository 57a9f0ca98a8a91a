// expand_plan.hpp — the move schedule of an alpha-expansion as host arithmetic alone (no device header: the planner is tested
// on a machine without a GPU, tests/expand_plan_driver.cpp).  run_expansion (expand.hip) asks next() what to enqueue, tells the
// planner what a batch's commit published, and what the control words held at the end of a cycle.
//
// Moves are numbered t = 0, 1, ... over the whole expansion; move t expands label alpha = t % L, and L moves make a cycle.
//   * TLAST is the index of the last accepted move.  The planner's copy is exact ("fresh") right behind a commit or a cycle's
//     end and unknown once a move has been enqueued on its own since.  A move t >= L with TLAST <= t - L is idempotent: nothing
//     has changed since the last expansion on its label.  When the planner can tell, the rest of the cycle is not launched at
//     all — nothing can be accepted in between — and a batch is cut in front of the first move known to be idempotent.
//   * Batches run only with at least two contexts and two labels: from the first cycle on when L >= batch_min_labels (a first
//     cycle from a cold start rewrites the labeling wholesale: with a handful of labels every accepted move touches its
//     successor's sites and nothing validates), from the second cycle on otherwise.
//   * A batch of B keeps its first j moves (1 <= j <= B); move j heads the next batch.  A batch that kept little was mostly
//     wasted work: when 2 j < B the next batches are half as large (never below 2); a batch of the full size that is kept whole
//     doubles them (never above the contexts).
#pragma once

#include <algorithm>

namespace mh {

class ExpandPlan {
public:
    enum class Kind { skip_rest, solo, batch };
    struct Step {
        Kind kind;
        int alpha, t;          // the first move of the step
        int count;             // skip_rest: the moves left in the cycle, none of them launched; solo: 1; batch: B
        bool apply_pending;    // batch: a move enqueued on its own may have left its labels pending, k_apply_pending runs first
    };

    ExpandPlan(int L, int contexts, int batch_min_labels)
        : L_(L), contexts_(contexts), can_batch_(contexts > 1 && L >= 2), batching_(can_batch_ && L >= batch_min_labels),
          bsize_(std::max(contexts, 1)) {}

    int cycle() const { return cycle_; }                 // counted from 1
    bool cycle_done() const { return alpha_ >= L_; }
    int bsize() const { return bsize_; }
    bool fresh() const { return fresh_; }
    int known_tlast() const { return tlast_; }           // (meaningful while fresh())

    Step next()
    {
        if (fresh_ && t_ >= L_ && tlast_ <= t_ - L_) {   // idempotent from here to the end of the cycle
            const Step s{ Kind::skip_rest, alpha_, t_, L_ - alpha_, false };
            t_ += s.count; alpha_ = L_;
            return s;
        }
        int B = std::min(bsize_, L_ - alpha_);
        if (fresh_ && t_ + B > tlast_ + L_ && tlast_ + L_ > t_ && t_ >= L_) B = tlast_ + L_ - t_;   // stop in front of the first idempotent move
        if (!batching_ || B < 2) {
            const Step s{ Kind::solo, alpha_, t_, 1, false };
            ++alpha_; ++t_;
            fresh_ = false;
            return s;
        }
        in_flight_ = B;
        return Step{ Kind::batch, alpha_, t_, B, !fresh_ };
    }

    // behind the batch next() returned: its first `first_invalid` moves are kept, the last accepted move is `tlast`
    void committed(int first_invalid, int tlast)
    {
        const int j = first_invalid, B = in_flight_;
        tlast_ = tlast;
        fresh_ = true;
        alpha_ += j; t_ += j;
        if (j < B) { if (2 * j < B) bsize_ = std::max(2, bsize_ / 2); }
        else if (B == bsize_) bsize_ = std::min(contexts_, 2 * bsize_);
    }

    void cycle_ended(int tlast)
    {
        tlast_ = tlast;
        fresh_ = true;
        alpha_ = 0;
        if (++cycle_ >= 2 && can_batch_) batching_ = true;
    }

private:
    int L_, contexts_;
    bool can_batch_, batching_;
    int bsize_;                    // moves of the next batch
    int alpha_ = 0, t_ = 0, cycle_ = 1;
    int tlast_ = -1;
    bool fresh_ = true;
    int in_flight_ = 0;            // B of the batch whose commit is awaited
};

} // namespace mh
