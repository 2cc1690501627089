// Host-compiled test of the tile planner of the K-column hybrid / additive patch sweeps
// (agglomerationmultigrid1d_amd/csrc/host_plan.hpp: patch_schwarz_multi_tile_plan, patch_schwarz_multi_max_sweeps, chunking
// through patch_chunks) under AddressSanitizer + UBSan: no device, no HIP.  For every m of multi_block_size, column groups
// of 1, 2, 4, 8 and S = 1 .. 8: the slab is 256 / m elements, the halo is 2 S a side, owned = te - 4 S and positive
// exactly up to max_sweeps = min(8, te / 8), the LDS is two padded planes per column and fits a compute unit (four
// workgroups of the largest group do), the tiles cover the sizes the GPU test sweeps exactly once, launch_has_tile of the
// new kind agrees with the plan, and the chunks of a run of sweeps add up.  Other m, other kb and sweeps 0 and 9: no tile.
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

static bool has_tile(int m, int S) {
  TileQuery q;
  q.launch = kTilePatchSchwarzMulti;
  q.te = patch_schwarz_multi_tile_elems(m);
  q.halo = S;
  return launch_has_tile(q);
}

int main() {
  constexpr size_t kLdsBytes = 160 * 1024;   // of a gfx950 compute unit
  int covered = 0;
  for (int m = 0; m <= 16; ++m) {
    if (!multi_block_size(m)) continue;
    ++covered;
    const int te = patch_schwarz_multi_tile_elems(m);
    const int smax = patch_schwarz_multi_max_sweeps(m);
    EXPECT(te == 256 / m, "m %d te %d", m, te);
    EXPECT(smax == std::min(kPatchMaxSweeps, te / 8) && smax >= 1, "m %d smax %d", m, smax);
    for (int kb : {1, 2, 4, 8})
      for (int S = 1; S <= 8; ++S) {
        const PatchTilePlan p = patch_schwarz_multi_tile_plan(m, S, kb);
        EXPECT(p.te == te, "m %d kb %d S %d te %d", m, kb, S, p.te);
        EXPECT(p.halo == 2 * S, "m %d kb %d S %d halo %d", m, kb, S, p.halo);
        EXPECT(p.owned == std::max(0, te - 4 * S), "m %d kb %d S %d owned %d", m, kb, S, p.owned);
        EXPECT((p.owned > 0) == (S <= smax), "m %d kb %d S %d owned %d smax %d", m, kb, S, p.owned, smax);
        if (p.owned > 0) EXPECT(p.owned + 2 * p.halo == p.te, "m %d kb %d S %d owned %d", m, kb, S, p.owned);
        if (S <= smax) EXPECT(2 * p.owned >= p.te, "m %d kb %d S %d: halos take more than half the tile", m, kb, S);
        EXPECT(p.lds_bytes == (size_t)2 * kb * (te + 2) * m * 8, "m %d kb %d S %d lds %zu", m, kb, S, p.lds_bytes);
        EXPECT(4 * p.lds_bytes <= kLdsBytes, "m %d kb %d S %d: four workgroups do not fit a compute unit (%zu bytes each)", m, kb, S,
               p.lds_bytes);
        EXPECT(has_tile(m, S) == (p.owned > 0), "m %d kb %d S %d", m, kb, S);
        if (p.owned <= 0) continue;
        // the sizes of the GPU test (2, 3, 130, 270) and the tile boundaries
        std::set<int64_t> sizes = {2, 3, 5, 130, 270, p.owned - 1, p.owned, p.owned + 1, 2 * (int64_t)p.owned + 1};
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
    // sweeps 0 and 9: no tile, whatever the group
    for (int kb : {1, 2, 4, 8})
      for (int S : {0, 9, -1})
        EXPECT(patch_schwarz_multi_tile_plan(m, S, kb).owned == 0 && !has_tile(m, S), "m %d kb %d S %d has a tile", m, kb, S);
    // other groups: no tile
    for (int kb : {0, 3, 5, 6, 7, 16, -1}) EXPECT(patch_schwarz_multi_tile_plan(m, 1, kb).owned == 0, "m %d kb %d has a tile", m, kb);
    // chunking: launches of at most smax sweeps, none empty, adding up, each with a tile
    for (int n = 0; n <= 40; ++n) {
      const int nc = patch_chunks(n, smax);
      int sum = 0;
      for (int c = 0; c < nc; ++c) {
        const int s = patch_chunk_sweeps(n, smax, c);
        EXPECT(s >= 1 && s <= smax && patch_schwarz_multi_tile_plan(m, s, 8).owned > 0 && has_tile(m, s), "m %d n %d chunk %d takes %d", m, n, c, s);
        sum += s;
      }
      EXPECT(sum == n, "m %d: chunks of %d sweeps add up to %d", m, n, sum);
    }
  }
  EXPECT(covered == 2, "multi_block_size covers %d sizes", covered);
  // the tiles of the GPU test's table
  EXPECT(patch_tiles(130, patch_schwarz_multi_tile_plan(4, 1, 8).owned) == 3 && patch_tiles(130, patch_schwarz_multi_tile_plan(4, 8, 8).owned) == 5,
         "m 4 ne 130");
  EXPECT(patch_tiles(270, patch_schwarz_multi_tile_plan(2, 1, 8).owned) == 3 && patch_tiles(270, patch_schwarz_multi_tile_plan(2, 8, 8).owned) == 3,
         "m 2 ne 270");
  // outside the coverage: no tile, and launch_has_tile says so
  for (int m = -1; m <= 16; ++m) {
    if (multi_block_size(m)) continue;
    EXPECT(patch_schwarz_multi_tile_elems(m) == 0 && patch_schwarz_multi_max_sweeps(m) == 0, "m %d has a slab", m);
    for (int kb : {1, 2, 4, 8})
      for (int S = 1; S <= 8; ++S) EXPECT(patch_schwarz_multi_tile_plan(m, S, kb).owned == 0 && !has_tile(m, S), "m %d kb %d S %d has a tile", m, kb, S);
  }
  if (failures) {
    std::printf("patch_schwarz_multi_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("patch_schwarz_multi_plan OK\n");
  return 0;
}
