// Host-compiled test of the layout of a dictionary stage of the coarsest solve (agglomerationmultigrid1d_amd/csrc/host_plan.hpp:
// cr_dict_plan, cr_dict_pack_odd; AGGMG_OPT_COARSE_DICTIONARY) under AddressSanitizer + UBSan: no device, no HIP.  For
// block sizes 1 and 2 and stages of 1 .. kCrMaxStageLevels levels: the table's offsets stand on 16 bytes and the levels'
// record ranges are disjoint and fill the table; the class indices of the levels are disjoint and cover what a chunk has;
// table and indices lie behind the stage's vectors and inside lds_bytes; the plan says no one class over the cap, one
// byte over the LDS limit, for a level without classes and for another block size; the largest cap fits the launch's
// LDS at the largest plan and one more class per level would not; an odd record holds its arrays' bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../agglomerationmultigrid1d_amd/csrc/host_plan.hpp"

using namespace aggmg;

static int failures = 0;
#define EXPECT(cond, ...)                    \
  do {                                       \
    if (!(cond)) {                           \
      ++failures;                            \
      std::printf("FAIL %s: ", #cond);       \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
    }                                        \
  } while (0)

static int stage_lds_total(int q, int m) {
  CrStagePlan S;
  S.q = q;
  cr_plan_steps(&S, m);
  return S.lds_total;
}

static void check_layout(int m, int q, const std::vector<int>& ne, const std::vector<int>& no, int cap) {
  const int lds_total = stage_lds_total(q, m);
  const CrDictPlan P = cr_dict_plan(m, q, lds_total, ne.data(), no.data(), cap);
  EXPECT(P.take, "m %d q %d", m, q);
  if (!P.take) return;
  // the table: even records of level 0, odd records of level 0, even records of level 1, ... back to back
  int at = 0;
  for (int l = 0; l < q; ++l) {
    EXPECT(P.tab_e[l] == at && P.tab_e[l] % 2 == 0, "m %d q %d level %d: even records at %d, expected %d", m, q, l, P.tab_e[l], at);
    at += ne[l] * cr_dict_even_words(m);
    EXPECT(P.tab_o[l] == at && P.tab_o[l] % 2 == 0, "m %d q %d level %d: odd records at %d, expected %d", m, q, l, P.tab_o[l], at);
    at += no[l] * cr_dict_odd_words(m);
  }
  EXPECT(P.tab_words == at && at % 2 == 0, "m %d q %d: table of %d words, expected %d", m, q, P.tab_words, at);
  // the class indices: 2^(q-l-1) + 1 even and 2^(q-l-1) odd rows of local level l, every one marked exactly once
  std::vector<int> seen((size_t)P.idx_count, 0);
  for (int l = 0; l < q; ++l) {
    const int cnt = 1 << (q - l - 1);
    for (int t = 0; t <= cnt; ++t) ++seen[(size_t)(P.idx_e[l] + t)];
    for (int t = 0; t < cnt; ++t) ++seen[(size_t)(P.idx_o[l] + t)];
  }
  int used = 0;
  for (int v : seen) {
    EXPECT(v <= 1, "m %d q %d: an index slot used %d times", m, q, v);
    used += v;
  }
  EXPECT(used == (2 << q) - 2 + q && P.idx_count == cr_dict_index_count(q) && P.idx_count % 8 == 0 && P.idx_count - used < 8,
         "m %d q %d: %d indices in %d slots", m, q, used, P.idx_count);
  // behind the vectors, 16-byte aligned, inside the launch's LDS
  EXPECT(P.tab_off >= lds_total && P.tab_off % 2 == 0 && P.idx_off == P.tab_off + P.tab_words, "m %d q %d: offsets %d %d", m, q, P.tab_off, P.idx_off);
  EXPECT(P.lds_bytes == (size_t)P.idx_off * 8 + (size_t)P.idx_count * 2 && P.lds_bytes <= kCrLdsBudgetBytes, "m %d q %d: %zu bytes", m, q, P.lds_bytes);
  // one byte over the limit: no
  EXPECT(cr_dict_plan(m, q, lds_total, ne.data(), no.data(), cap, P.lds_bytes).take, "m %d q %d: the exact limit", m, q);
  EXPECT(!cr_dict_plan(m, q, lds_total, ne.data(), no.data(), cap, P.lds_bytes - 1).take, "m %d q %d: one byte less", m, q);
}

int main() {
  static_assert(cr_dict_even_words(1) == 2 && cr_dict_even_words(2) == 8, "fe pair");
  static_assert(cr_dict_odd_words(1) == 4 && cr_dict_odd_words(2) == 14, "fo pair, lu, perm, padded to 16 bytes");
  static_assert(cr_dict_index_count(12) == 8208, "a chunk of 2^12 blocks");
  for (int m : {1, 2})
    for (int q = 1; q <= kCrMaxStageLevels; ++q) {
      std::vector<int> ne((size_t)q), no((size_t)q);
      for (int l = 0; l < q; ++l) ne[(size_t)l] = 1 + (l * 7 + q) % 24, no[(size_t)l] = 1 + (l * 5 + m) % 16;
      check_layout(m, q, ne, no, 24);
      // a level one class over the cap, of either kind; a level without classes; a cap of 0
      for (int l = 0; l < q; ++l) {
        const int lds_total = stage_lds_total(q, m);
        std::vector<int> e2 = ne, o2 = no;
        e2[(size_t)l] = 25;
        EXPECT(!cr_dict_plan(m, q, lds_total, e2.data(), no.data(), 24).take, "m %d q %d level %d: 25 even classes", m, q, l);
        o2[(size_t)l] = 25;
        EXPECT(!cr_dict_plan(m, q, lds_total, ne.data(), o2.data(), 24).take, "m %d q %d level %d: 25 odd classes", m, q, l);
        e2[(size_t)l] = 24, o2[(size_t)l] = 24;
        EXPECT(cr_dict_plan(m, q, lds_total, e2.data(), o2.data(), 24).take, "m %d q %d level %d: at the cap", m, q, l);
        o2[(size_t)l] = 0;
        EXPECT(!cr_dict_plan(m, q, lds_total, ne.data(), o2.data(), 24).take, "m %d q %d level %d: no odd class", m, q, l);
      }
      EXPECT(!cr_dict_plan(m, q, stage_lds_total(q, m), ne.data(), no.data(), 0).take, "m %d q %d: cap 0", m, q);
    }
  // other block sizes, other stage lengths
  {
    const int one[kCrMaxStageLevels + 1] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    for (int m : {0, 3, 4, 8}) EXPECT(!cr_dict_plan(m, 4, 64, one, one, 8).take, "block size %d", m);
    EXPECT(!cr_dict_plan(2, 0, 64, one, one, 8).take && !cr_dict_plan(2, kCrMaxStageLevels + 1, 64, one, one, 8).take, "stage lengths");
  }
  // the largest cap: every level of the largest plan full, and one class more per level does not fit
  {
    const int q = kCrMaxStageLevels;
    std::vector<int> full((size_t)q, kCrDictMaxClasses), more((size_t)q, kCrDictMaxClasses + 1);
    check_layout(2, q, full, full, kCrDictMaxClasses);
    check_layout(1, q, full, full, kCrDictMaxClasses);
    EXPECT(!cr_dict_plan(2, q, stage_lds_total(q, 2), more.data(), more.data(), kCrDictMaxClasses + 1).take, "cap + 1 at the largest plan");
  }
  // an odd record: fo, lu, perm in that order, the pad zero
  for (int m : {1, 2}) {
    const int nc = 3, mm = m * m, w = cr_dict_odd_words(m);
    std::vector<double> fo((size_t)nc * 2 * mm), lu((size_t)nc * mm), rec((size_t)nc * w, -1.0);
    std::vector<int32_t> pm((size_t)nc * m);
    for (size_t i = 0; i < fo.size(); ++i) fo[i] = 1.5 + (double)i;
    for (size_t i = 0; i < lu.size(); ++i) lu[i] = -2.25 - (double)i;
    for (size_t i = 0; i < pm.size(); ++i) pm[i] = (int32_t)((i * 7 + 1) % (size_t)m);
    cr_dict_pack_odd(m, nc, fo.data(), lu.data(), pm.data(), rec.data());
    for (int c = 0; c < nc; ++c) {
      const double* r = rec.data() + (size_t)c * w;
      EXPECT(!std::memcmp(r, fo.data() + (size_t)c * 2 * mm, (size_t)2 * mm * 8), "m %d class %d: fo", m, c);
      EXPECT(!std::memcmp(r + 2 * mm, lu.data() + (size_t)c * mm, (size_t)mm * 8), "m %d class %d: lu", m, c);
      EXPECT(!std::memcmp(r + 3 * mm, pm.data() + (size_t)c * m, (size_t)m * 4), "m %d class %d: perm", m, c);
      const unsigned char* tail = reinterpret_cast<const unsigned char*>(r + 3 * mm) + m * 4;
      const unsigned char* end = reinterpret_cast<const unsigned char*>(r + w);
      for (; tail < end; ++tail) EXPECT(*tail == 0, "m %d class %d: pad", m, c);
    }
  }
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("cr_dict_plan OK\n");
  return 0;
}
