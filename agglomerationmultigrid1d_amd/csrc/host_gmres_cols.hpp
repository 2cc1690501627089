// GmresSlots: the slot bookkeeping of K GMRES recurrences in lockstep (aggmg_fgmres_multi_dev), on the host (no HIP:
// tests/host/test_host_gmres_cols.cpp compiles it alone).  Slot s < active() of the work matrices holds column
// column(s); a finished column leaves and the last active slot's state moves into its place, so the active slots stay
// contiguous and no launch carries a finished column.  The class decides which moves a set of finishes implies and
// counts the column-V-cycles run; the caller carries the state (basis vectors, scalars) a move names.
#pragma once
#include <cstdint>
#include <vector>

class GmresSlots {
 public:
  explicit GmresSlots(int K) : col_((size_t)K), n_(K) {
    for (int j = 0; j < K; ++j) col_[(size_t)j] = j;
  }
  int active() const { return n_; }
  int column(int slot) const { return col_[(size_t)slot]; }
  // the slot -> column map: entries [0, active()) are the active columns, the entries behind them the columns that
  // have left (most recent first); always a permutation of 0 .. K - 1
  const int* map() const { return col_.data(); }
  int size() const { return (int)col_.size(); }

  // one K-column cycle was run on the active slots
  void count_cycle() { work_ += n_; }
  int64_t work_cols() const { return work_; }

  // drops the slots flagged in finished[0 .. active() - 1], from the highest slot down; for every drop that is not the
  // last active slot, move(dst, src) is called BEFORE the map changes and must carry slot src's state to slot dst
  // (src is then the last active slot, and it is never a finished one: those above dst have already left).  A
  // non-zero return of move stops the walk and is returned.
  template <class F>
  int finish(const std::vector<char>& finished, F&& move) {
    for (int s = n_ - 1; s >= 0; --s) {
      if (!finished[(size_t)s]) continue;
      const int last = n_ - 1;
      const int gone = col_[(size_t)s];
      if (s != last) {
        if (int st = move(s, last)) return st;
        col_[(size_t)s] = col_[(size_t)last];
      }
      col_[(size_t)last] = gone;
      --n_;
    }
    return 0;
  }

 private:
  std::vector<int> col_;
  int n_;
  int64_t work_ = 0;
};
