// Host-compiled test of the tile planner of the K-column multiplicative patch sweeps
// (agglomerationmultigrid1d_amd/csrc/host_plan.hpp: patch_gs_multi_tile_plan, patch_gs_multi_max_sweeps, chunking through
// patch_chunks) under AddressSanitizer + UBSan: no device, no HIP.  For m = 2, 4, column groups of 1, 2, 4, 8 and
// S = 1 .. 8: the owned elements and the two halos make up the tile, the halo is 2 S + 1, the LDS fits a compute unit (and
// two workgroups of the largest group do), a launch takes at least one sweep, the tiles cover the sizes the GPU test
// sweeps exactly once, launch_has_tile agrees with the plan, and the chunks of a run of sweeps add up.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
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
  constexpr size_t kLdsBytes = 160 * 1024;   // of a gfx950 compute unit
  for (int m : {2, 4}) {
    const int smax = patch_gs_multi_max_sweeps(m);
    EXPECT(smax >= 1 && smax <= kPatchMaxSweeps, "m %d smax %d", m, smax);
    for (int kb : {1, 2, 4, 8})
      for (int S = 1; S <= 8; ++S) {
        const PatchTilePlan p = patch_gs_multi_tile_plan(m, S, kb);
        EXPECT(p.te == 256 / m && p.te == patch_gs_multi_tile_elems(m), "m %d kb %d S %d te %d", m, kb, S, p.te);
        EXPECT(p.halo == 2 * S + 1 && p.halo == patch_gs_halo(S), "m %d kb %d S %d halo %d", m, kb, S, p.halo);
        EXPECT(p.owned >= 0, "m %d kb %d S %d owned %d", m, kb, S, p.owned);
        if (p.owned > 0) EXPECT(p.owned + 2 * p.halo == p.te, "m %d kb %d S %d owned %d", m, kb, S, p.owned);
        EXPECT(p.lds_bytes == (size_t)2 * kb * (p.te + 2) * m * 8 && p.lds_bytes <= kLdsBytes, "m %d kb %d S %d lds %zu", m, kb, S,
               p.lds_bytes);
        EXPECT(2 * p.lds_bytes <= kLdsBytes, "m %d kb %d S %d: two workgroups do not fit a compute unit (%zu bytes each)", m, kb, S,
               p.lds_bytes);
        if (S <= smax) EXPECT(p.owned >= 1, "m %d kb %d S %d <= smax %d has no tile", m, kb, S, smax);
        if (S <= smax && S > 1) EXPECT(2 * p.owned >= p.te, "m %d kb %d S %d: halos take more than half the tile", m, kb, S);
        TileQuery q;
        q.launch = kTilePatchGsMulti;
        q.te = patch_gs_multi_tile_elems(m);
        q.halo = S;
        EXPECT(launch_has_tile(q) == (p.owned > 0), "m %d kb %d S %d", m, kb, S);
        if (p.owned <= 0) continue;
        // the sizes of the GPU test: 2, 3, 5, own - 1, own, own + 1, 2 own + 1
        std::set<int64_t> sizes = {2, 3, 5, p.owned - 1, p.owned, p.owned + 1, 2 * (int64_t)p.owned + 1};
        for (int64_t ne : sizes) {
          if (ne < 2) continue;
          const int64_t nt = patch_tiles(ne, p.owned);
          std::vector<int> cover((size_t)ne, 0);
          for (int64_t t = 0; t < nt; ++t) {
            const int64_t e0 = t * p.owned - p.halo;   // element at x = 0 (the kernel's arithmetic)
            EXPECT(t * p.owned < ne, "m %d S %d ne %lld: tile %lld owns nothing", m, S, (long long)ne, (long long)t);
            for (int x = p.halo; x < p.halo + p.owned; ++x) {
              EXPECT(x >= 0 && x < p.te, "owned x %d outside the tile", x);
              const int64_t e = e0 + x;
              if (e >= 0 && e < ne) ++cover[(size_t)e];
            }
          }
          for (int64_t e = 0; e < ne; ++e)
            if (cover[(size_t)e] != 1) {
              EXPECT(false, "m %d S %d ne %lld: element %lld covered %d times", m, S, (long long)ne, (long long)e, cover[(size_t)e]);
              break;
            }
        }
      }
    // chunking: launches of at most smax sweeps, none empty, adding up, each with a tile
    for (int n = 0; n <= 40; ++n) {
      const int nc = patch_chunks(n, smax);
      int sum = 0;
      for (int c = 0; c < nc; ++c) {
        const int s = patch_chunk_sweeps(n, smax, c);
        EXPECT(s >= 1 && s <= smax && patch_gs_multi_tile_plan(m, s, 8).owned > 0, "m %d n %d chunk %d takes %d", m, n, c, s);
        sum += s;
      }
      EXPECT(sum == n, "m %d: chunks of %d sweeps add up to %d", m, n, sum);
    }
  }
  // outside the coverage: no tile, and launch_has_tile says so
  for (int m : {0, 1, 3, 5, 8}) {
    EXPECT(patch_gs_multi_tile_plan(m, 1, 8).owned == 0 && patch_gs_multi_max_sweeps(m) == 0, "m %d has a tile", m);
    TileQuery q;
    q.launch = kTilePatchGsMulti;
    q.te = patch_gs_multi_tile_elems(m);
    q.halo = 1;
    EXPECT(!launch_has_tile(q), "m %d", m);
  }
  for (int kb : {0, 3, 5, 16}) EXPECT(patch_gs_multi_tile_plan(4, 1, kb).owned == 0, "kb %d has a tile", kb);
  EXPECT(patch_gs_multi_tile_plan(4, 0, 8).owned == 0 && patch_gs_multi_tile_plan(4, 9, 8).owned == 0,
         "sweep counts outside 1 .. 8 have no tile");
  if (failures) {
    std::printf("patch_multi_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("patch_multi_plan OK\n");
  return 0;
}
