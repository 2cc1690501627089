// Host-compiled test of the element-patch Schwarz tile planner (agglomerationmultigrid1d_amd/csrc/host_plan.hpp:
// patch_tile_plan, patch_max_sweeps, patch_tiles, patch_chunks) under AddressSanitizer + UBSan: no device, no HIP.
// For m = 1 .. 8 and S = 1 .. 8: owned + halos fit the tile and the LDS of a compute unit; the tiles cover [0, ne)
// exactly once for ne = 1 .. three tiles + 1, and every element a tile reads lies inside the tile; the chunking of a run
// of sweeps adds up.  `query m S` prints the plan for the tests that need the boundaries.
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

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "query")) {
    const int m = std::atoi(argv[2]), S = std::atoi(argv[3]);
    const PatchTilePlan p = patch_tile_plan(m, S);
    std::printf("te %d halo %d owned %d lds %zu smax %d\n", p.te, p.halo, p.owned, p.lds_bytes, patch_max_sweeps(m));
    return 0;
  }
  constexpr size_t kLdsBytes = 160 * 1024;   // of a gfx950 compute unit
  for (int m = 1; m <= 8; ++m) {
    const int smax = patch_max_sweeps(m);
    EXPECT(smax >= 1 && smax <= kPatchMaxSweeps, "m %d smax %d", m, smax);
    EXPECT(patch_tile_elems(m) == (256 / m) * patch_slabs(m), "m %d", m);
    for (int S = 1; S <= 8; ++S) {
      const PatchTilePlan p = patch_tile_plan(m, S);
      EXPECT(p.te == patch_tile_elems(m), "m %d S %d", m, S);
      EXPECT(p.halo == 2 * S, "m %d S %d halo %d", m, S, p.halo);
      EXPECT(p.owned >= 0 && (p.owned == 0 || p.owned + 2 * p.halo == p.te), "m %d S %d owned %d", m, S, p.owned);
      EXPECT(p.lds_bytes == (size_t)3 * (p.te + 2) * m * 8 && p.lds_bytes <= kLdsBytes, "m %d S %d lds %zu", m, S, p.lds_bytes);
      EXPECT((size_t)p.te * m <= 256 * (size_t)patch_slabs(m), "m %d: more rows than threads x slabs", m);
      if (S <= smax) EXPECT(p.owned >= 1, "m %d S %d <= smax %d has no tile", m, S, smax);
      if (S <= smax && S > 1) EXPECT(2 * p.owned >= p.te || p.te < 8, "m %d S %d: halos take more than half the tile", m, S);
      TileQuery q;
      q.launch = kTilePatch;
      q.te = p.te;
      q.halo = S;
      EXPECT(launch_has_tile(q) == (p.owned > 0), "m %d S %d", m, S);
      if (p.owned <= 0) continue;
      for (int64_t ne = 1; ne <= 3 * (int64_t)p.owned + 1; ++ne) {
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
          // what the owned elements read after S sweeps: 2 S elements either side, all held by the tile
          EXPECT(p.halo - 2 * S >= 0 && p.halo + p.owned - 1 + 2 * S < p.te, "m %d S %d: reach leaves the tile", m, S);
        }
        for (int64_t e = 0; e < ne; ++e)
          if (cover[(size_t)e] != 1) {
            EXPECT(false, "m %d S %d ne %lld: element %lld covered %d times", m, S, (long long)ne, (long long)e, cover[(size_t)e]);
            break;
          }
      }
    }
    // chunking: launches of at most smax sweeps, none empty, adding up
    for (int n = 0; n <= 40; ++n) {
      const int nc = patch_chunks(n, smax);
      int sum = 0;
      for (int c = 0; c < nc; ++c) {
        const int s = patch_chunk_sweeps(n, smax, c);
        EXPECT(s >= 1 && s <= smax, "m %d n %d chunk %d takes %d", m, n, c, s);
        sum += s;
      }
      EXPECT(sum == n, "m %d: chunks of %d sweeps add up to %d", m, n, sum);
      EXPECT(n == 0 ? nc == 0 : nc == (n + smax - 1) / smax, "m %d n %d chunks %d", m, n, nc);
    }
  }
  EXPECT(patch_tile_plan(4, 0).owned == 0 && patch_tile_plan(4, 9).owned == 0, "sweep counts outside 1 .. 8 have no tile");
  EXPECT(patch_tile_elems(0) == 0 && patch_max_sweeps(0) == 0, "m = 0");
  if (failures) {
    std::printf("patch_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("patch_plan OK\n");
  return 0;
}
