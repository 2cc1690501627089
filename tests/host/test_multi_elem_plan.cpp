// Host-compiled test of the tile a K-column element-thread launch runs (aggmg_multi_element_tile_plan, launch_multi_elem:
// agglomerationmultigrid1d_amd/csrc/host_plan.hpp, fused_tile_plan on 256 elements with fused_tile_subset's tiles) under
// AddressSanitizer + UBSan: no device, no HIP.  For halos 0 .. 140 and agglomeration ratios 1 .. 16: the owned elements
// are floor((256 - 2 halo) / rho) rho, whole agglomerates that fit the tile beside the two halos, zero exactly where the
// halo leaves less than one agglomerate; and for level sizes around the tile's the tiles cover every element once, the
// first element of a tile's slab is never past the level, and every coarse element belongs to one tile.
#include <cstdint>
#include <cstdio>
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

int main() {
  constexpr int TE = 256;   // kElemThreads
  long plans = 0, levels = 0;
  for (int halo = 0; halo <= 140; ++halo)
    for (int rho = 1; rho <= 16; ++rho) {
      const FusedTilePlan p = fused_tile_plan(TE, halo, rho, false, -1);
      ++plans;
      const int room = TE - 2 * halo;
      const int want = room >= rho ? (room / rho) * rho : 0;
      EXPECT(p.owned == want, "halo %d rho %d: owned %d, want %d", halo, rho, p.owned, want);
      EXPECT(p.owned % rho == 0 && p.owned >= 0, "halo %d rho %d: owned %d", halo, rho, p.owned);
      EXPECT(p.halo_left == halo && p.agg_shift == -1, "halo %d rho %d: halo_left %d shift %d", halo, rho, p.halo_left, p.agg_shift);
      EXPECT(p.owned == 0 || p.halo_left + p.owned + halo <= TE, "halo %d rho %d: the slab overflows the tile", halo, rho);
      if (p.owned == 0) continue;
      for (int64_t nec : {int64_t(1), int64_t(p.owned / rho), int64_t(p.owned / rho) + 1, int64_t(3 * (p.owned / rho)), int64_t(1000)}) {
        const int64_t ne = nec * rho;
        const TileSubset sub = fused_tile_subset(ne, p.owned, 0, 0, 0);
        ++levels;
        EXPECT(sub.split == 0 && sub.skip == 0, "all tiles: split %d skip %lld", sub.split, (long long)sub.skip);
        EXPECT(sub.ntiles * p.owned >= ne && (sub.ntiles - 1) * (int64_t)p.owned < ne, "ne %lld owned %d: %lld tiles", (long long)ne,
               p.owned, (long long)sub.ntiles);
        std::vector<int> hits((size_t)ne, 0), chits((size_t)nec, 0);
        const int ncoarse = p.owned / rho;
        for (int64_t t = 0; t < sub.ntiles; ++t) {
          const int64_t e0 = t * p.owned - p.halo_left;   // the kernel's element at x = 0
          EXPECT(ne - 1 - e0 >= 0, "tile %lld starts past the level", (long long)t);
          for (int x = p.halo_left; x < p.halo_left + p.owned; ++x)
            if (e0 + x < ne) ++hits[(size_t)(e0 + x)];
          for (int j = 0; j < ncoarse; ++j)
            if (t * ncoarse + j < nec) ++chits[(size_t)(t * ncoarse + j)];
        }
        for (int64_t e = 0; e < ne; ++e) EXPECT(hits[(size_t)e] == 1, "element %lld owned %d times", (long long)e, hits[(size_t)e]);
        for (int64_t j = 0; j < nec; ++j) EXPECT(chits[(size_t)j] == 1, "coarse element %lld restricted %d times", (long long)j, chits[(size_t)j]);
      }
    }
  // the halves of the cycles the GPU tests run
  EXPECT(fused_tile_plan(TE, 4, 4, false, -1).owned == 248, "V(3,.) descent");
  EXPECT(fused_tile_plan(TE, 9, 4, false, -1).owned == 236, "V(8,.) descent");
  EXPECT(fused_tile_plan(TE, 3, 1, false, -1).owned == 250, "V(.,3) ascent");
  EXPECT(fused_tile_plan(TE, 128, 4, false, -1).owned == 0, "no tile");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("multi_elem_plan OK: %ld plans, %ld levels\n", plans, levels);
  return 0;
}
