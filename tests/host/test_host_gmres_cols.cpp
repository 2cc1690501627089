// Host unit test of GmresSlots (csrc/host_gmres_cols.hpp), the slot bookkeeping of aggmg_fgmres_multi_dev: a model of
// the lockstep loop in which column c finishes after want[c] iterations (0: at the start of the first restart cycle)
// and every slot carries a token that only the moves the class asks for can carry along.  Checked after every finish:
// the active slots hold exactly the unfinished columns, each with its own token; the map is a permutation; and at the
// end work_cols is the sum of the per-column iteration counts.
#include <cstdio>
#include <vector>

#include "../../agglomerationmultigrid1d_amd/csrc/host_gmres_cols.hpp"

static int g_fail = 0;
#define EXPECT(c)                                             \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                               \
    }                                                         \
  } while (0)

static void check_state(const GmresSlots& sl, const std::vector<int>& token, const std::vector<char>& gone) {
  const int K = sl.size();
  std::vector<int> seen((size_t)K, 0);
  for (int s = 0; s < K; ++s) {
    const int c = sl.map()[s];
    EXPECT(c >= 0 && c < K);
    if (c >= 0 && c < K) seen[(size_t)c] += 1;
  }
  for (int c = 0; c < K; ++c) EXPECT(seen[(size_t)c] == 1);   // a permutation
  int left = 0;
  for (int c = 0; c < K; ++c) left += gone[(size_t)c] ? 0 : 1;
  EXPECT(sl.active() == left);
  for (int s = 0; s < sl.active(); ++s) {
    EXPECT(!gone[(size_t)sl.column(s)]);
    EXPECT(token[(size_t)s] == 1000 + sl.column(s));   // the slot's state is its column's
  }
  for (int s = sl.active(); s < K; ++s) EXPECT(gone[(size_t)sl.map()[s]]);
}

// runs the model; expect_moves < 0: not checked
static void run(const char* name, const std::vector<int>& want, int expect_moves) {
  const int K = (int)want.size();
  GmresSlots sl(K);
  std::vector<int> token((size_t)K), iters((size_t)K, 0);
  std::vector<char> gone((size_t)K, 0), fin((size_t)K, 0);
  for (int s = 0; s < K; ++s) token[(size_t)s] = 1000 + s;
  int moves = 0;
  auto move = [&](int dst, int src) {
    EXPECT(src == sl.active() - 1);        // the last active slot moves
    EXPECT(dst < src);
    EXPECT(fin[(size_t)dst] && gone[(size_t)sl.column(dst)]);
    EXPECT(!gone[(size_t)sl.column(src)]);   // never a finished column's state
    token[(size_t)dst] = token[(size_t)src];
    ++moves;
    return 0;
  };
  auto drop = [&]() {
    bool any = false;
    for (int s = 0; s < sl.active(); ++s) any = any || fin[(size_t)s];
    if (!any) return;
    for (int s = 0; s < sl.active(); ++s)
      if (fin[(size_t)s]) gone[(size_t)sl.column(s)] = 1;
    EXPECT(sl.finish(fin, move) == 0);
    check_state(sl, token, gone);
  };
  check_state(sl, token, gone);
  for (int s = 0; s < sl.active(); ++s) fin[(size_t)s] = want[(size_t)sl.column(s)] == 0;   // the test at entry
  drop();
  int it = 0;
  while (sl.active() > 0) {
    sl.count_cycle();
    ++it;
    for (int s = 0; s < sl.active(); ++s) {
      const int c = sl.column(s);
      iters[(size_t)c] = it;
      fin[(size_t)s] = want[(size_t)c] == it;
    }
    drop();
    if (it > 1000) {
      std::printf("the model does not end\n");
      ++g_fail;
      break;
    }
  }
  long long sum = 0;
  for (int c = 0; c < K; ++c) {
    EXPECT(iters[(size_t)c] == want[(size_t)c]);
    sum += want[(size_t)c];
  }
  EXPECT(sl.work_cols() == sum);
  if (expect_moves >= 0) EXPECT(moves == expect_moves);
  if (g_fail) std::printf("  (in case %s)\n", name);
}

// a move that fails stops the walk and its status comes back
static void failing_move() {
  GmresSlots sl(4);
  std::vector<char> fin = {1, 0, 0, 0};
  EXPECT(sl.finish(fin, [](int, int) { return 7; }) == 7);
}

int main() {
  run("one column finishes alone", {5, 2, 5, 5}, 1);
  run("the last slot finishes: no move", {5, 5, 5, 2}, 0);
  run("all finish at once", {3, 3, 3, 3, 3}, 0);
  run("several in one iteration, the last slot among them", {2, 6, 2, 6, 6, 2}, 2);
  run("several in one iteration, neighbours", {4, 1, 1, 1, 4, 4, 4}, 3);
  run("a finish at iteration 0", {0, 3, 0, 3, 5}, -1);
  run("all at iteration 0", {0, 0, 0}, 0);
  run("K = 1", {4}, 0);
  run("K = 1 at iteration 0", {0}, 0);
  run("every column its own count, descending", {9, 8, 7, 6, 5, 4, 3, 2, 1}, 0);
  run("every column its own count, ascending", {1, 2, 3, 4, 5, 6, 7, 8, 9}, -1);
  run("mixed", {7, 0, 3, 3, 12, 1, 7, 0, 2, 12, 5}, -1);
  failing_move();
  if (g_fail) {
    std::printf("host_gmres_cols FAILED: %d\n", g_fail);
    return 1;
  }
  std::printf("host_gmres_cols OK\n");
  return 0;
}
