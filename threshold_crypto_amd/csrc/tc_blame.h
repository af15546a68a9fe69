// Blame by bisection: which live shares of a failed job are bad, found with range checks instead of one pairing check per
// share (pass 2 of the robust combiners, tc_api.hip).  Host C++ only -- no HIP, no device code: g++ compiles
// it for tests/blame/, as tc_robust.h is for tests/robust/.  The caller owns the oracle: plan() names the ranges of one
// round, the caller answers each with one verdict byte (1 = the range check passed), apply() takes them.
//
// THE RULE (the tests count checks exactly):
//   * A slot is LIVE when it is present, its share decoded, (checked-input / wire mode) is a group member and the job's own
//     operands are valid.  A present slot that is not live is bad without any check; an absent slot is ignored.
//   * A work item is a range [lo, hi) that is `unknown` or `failing` (known to hold a bad live share).  Start: (0, N, unknown).
//   * One round = the checks of every pending item, answered together.
//       - an unknown range without a live slot passes without a check;
//       - any other unknown range gets ONE check: passed (dropped) or failing;
//       - a failing range of length 1 sets that slot's bad bit;
//       - a longer failing range splits at mid = lo + ((hi - lo + 1) >> 1) and its LEFT half is checked first:
//           left passes, or holds no live slot  ->  the right half is failing by inference, no check;
//           left fails                          ->  the left half is failing, the right half becomes unknown (checked in
//                                                   the next round, beside the left half's own children).
//   * BOUNDS, with d = ceil(log2 N) and k = bad live shares:  checks <= min(1 + 2 k d, 2 N - 1),  rounds <= 2 d + 1
//     (the root, then per level at most the left check and, a round later, the right one).
// A range check that wrongly passes (probability <= 2^-63 each, the scalars being secret) can leave a bad share unmarked
// and, through the inference step, mark an honest one; a range that is failing by inference but holds no live slot is dropped.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace tc {

struct BlameRange {
  uint32_t lo, hi;
};

class BlameSearch {
 public:
  uint64_t checks = 0, rounds = 0;

  // present / live: N bytes each (live implies present); bad: N bytes, written here and by apply()
  void start(uint32_t N, const uint8_t* present, const uint8_t* live, uint8_t* bad) {
    n_ = N;
    bad_ = bad;
    checks = rounds = 0;
    pre_.assign((size_t)N + 1, 0);
    for (uint32_t i = 0; i < N; i++) {
      const bool l = live[i] != 0 && present[i] != 0;
      pre_[i + 1] = pre_[i] + (l ? 1u : 0u);
      bad[i] = (present[i] != 0 && !l) ? 1 : 0;
    }
    work_.clear();
    wait_.clear();
    if (N) work_.push_back(Item{0, N, kUnknown});
  }
  // the checks of the next round, appended to `out` in the order apply() reads their verdicts; returns how many (0: done)
  size_t plan(std::vector<BlameRange>& out) {
    wait_.clear();
    // (expanding an item may make further items that need no check: the list is worked until only checks are left)
    for (size_t w = 0; w < work_.size(); w++) {
      const Item it = work_[w];
      if (!has_live(it.lo, it.hi)) continue;  // unknown: passes unchecked; failing by a wrong inference: dropped
      if (it.state == kUnknown) {
        wait_.push_back(Wait{it.lo, it.hi, it.hi, false});
        out.push_back(BlameRange{it.lo, it.hi});
      } else if (it.hi - it.lo == 1) {
        bad_[it.lo] = 1;
      } else {
        const uint32_t mid = it.lo + ((it.hi - it.lo + 1) >> 1);
        if (!has_live(it.lo, mid)) {
          work_.push_back(Item{mid, it.hi, kFailing});
        } else {
          wait_.push_back(Wait{it.lo, mid, it.hi, true});
          out.push_back(BlameRange{it.lo, mid});
        }
      }
    }
    work_.clear();
    if (!wait_.empty()) {
      checks += wait_.size();
      rounds++;
    }
    return wait_.size();
  }
  // pass[i] != 0: check i of the last plan() passed
  void apply(const uint8_t* pass) {
    for (size_t i = 0; i < wait_.size(); i++) {
      const Wait& w = wait_[i];
      const bool ok = pass[i] != 0;
      if (!w.left) {
        if (!ok) work_.push_back(Item{w.lo, w.mid, kFailing});
      } else if (ok) {
        work_.push_back(Item{w.mid, w.hi, kFailing});
      } else {
        work_.push_back(Item{w.lo, w.mid, kFailing});
        work_.push_back(Item{w.mid, w.hi, kUnknown});
      }
    }
    wait_.clear();
  }

 private:
  enum : uint8_t { kUnknown = 0, kFailing = 1 };
  struct Item {
    uint32_t lo, hi;
    uint8_t state;
  };
  struct Wait {  // a check in flight: [lo, mid) -- a whole unknown range (mid == hi), or the left half of failing [lo, hi)
    uint32_t lo, mid, hi;
    bool left;
  };
  bool has_live(uint32_t lo, uint32_t hi) const { return pre_[hi] != pre_[lo]; }
  uint32_t n_ = 0;
  uint8_t* bad_ = nullptr;
  std::vector<uint32_t> pre_;  // live slots before slot i
  std::vector<Item> work_;
  std::vector<Wait> wait_;
};

}  // namespace tc
