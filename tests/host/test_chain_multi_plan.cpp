// Host-compiled test of the tile planner of the K-column chain launches
// (agglomerationmultigrid1d_amd/csrc/host_plan.hpp: chain_multi_tile_plan, chain_multi_max_sweeps, launch_has_tile with
// kTileChainMulti) under AddressSanitizer + UBSan: no device, no HIP.  For block sizes 1 .. 8, 0 .. 9 sweeps, the three
// kinds of launch end (no restriction, chain, agglomerating), agglomeration ratios 1 .. 300 and column groups 1, 2, 4, 8
// (and 3, which has no kernel): the owned blocks and the two halos fit the tile, the owned blocks are whole agglomerates,
// launch_has_tile agrees with the plan, a launch of up to max_sweeps sweeps always has a tile at ratio 1, the LDS fits a
// workgroup's 64 KiB, and the tiles cover a level exactly once.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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
  constexpr size_t kLdsLimit = 64 * 1024;
  long tiles = 0;
  for (int m = 1; m <= 8; ++m) {
    const bool covered = m == 1 || m == 2 || m == 4;
    const int smax = chain_multi_max_sweeps(m);
    EXPECT(covered ? (smax >= 1 && smax <= 8) : smax == 0, "m %d smax %d", m, smax);
    EXPECT(chain_multi_tile_blocks(m) == (covered ? 256 / m : 0), "m %d te %d", m, chain_multi_tile_blocks(m));
    for (int S = 0; S <= 9; ++S)
      for (int kind : {0, 1, 2})
        for (int rho : {1, 2, 3, 4, 16, 60, 300})
          for (int kb : {1, 2, 4, 8, 3}) {
            const ChainMultiPlan p = chain_multi_tile_plan(m, S, kind, rho, kb);
            const int align = kind == kChainToAgg ? rho : 1;
            EXPECT(p.owned >= 0, "m %d S %d kind %d rho %d kb %d owned %d", m, S, kind, rho, kb, p.owned);
            EXPECT(p.owned % align == 0, "m %d S %d kind %d rho %d kb %d owned %d", m, S, kind, rho, kb, p.owned);
            EXPECT(p.owned == 0 || p.halo_left + p.owned + p.halo_right <= p.te, "m %d S %d kind %d rho %d kb %d: %d + %d + %d > %d", m, S, kind,
                   rho, kb, p.halo_left, p.owned, p.halo_right, p.te);
            TileQuery q;
            q.launch = kTileChainMulti;
            q.te = m;
            q.halo = S;
            q.restrict_kind = kind;
            q.align = rho;
            q.kb = kb;
            EXPECT(launch_has_tile(q) == (p.owned > 0), "m %d S %d kind %d rho %d kb %d", m, S, kind, rho, kb);
            if (!covered || kb == 3 || S > 8) EXPECT(p.owned == 0, "m %d S %d kb %d has a tile", m, S, kb);
            if (p.owned == 0) continue;
            ++tiles;
            // the halos of the single-column launch
            EXPECT(p.halo_left == S + (kind ? 1 : 0) + (kind == kChainToChain ? 1 : 0), "m %d S %d kind %d hl %d", m, S, kind, p.halo_left);
            EXPECT(p.halo_right == S + (kind ? 1 : 0) + (kind == kChainToAgg ? 1 : 0), "m %d S %d kind %d hr %d", m, S, kind, p.halo_right);
            EXPECT(p.te == 256 / m, "m %d te %d", m, p.te);
            EXPECT(p.owned == chain_tile_owned(p.te, p.halo_left, p.halo_right, align), "m %d S %d kind %d rho %d owned %d", m, S, kind, rho, p.owned);
            for (bool dict : {false, true}) {
              const ChainMultiPlan d = chain_multi_tile_plan(m, S, kind, rho, kb, dict);
              EXPECT(d.lds_bytes == (size_t)2 * kb * (p.te + 2) * m * 8 + (dict ? (size_t)(p.te + 2) * 2 : 0) && d.lds_bytes <= kLdsLimit,
                     "m %d kb %d dict %d lds %zu", m, kb, (int)dict, d.lds_bytes);
              EXPECT(d.owned == p.owned && d.halo_left == p.halo_left, "the dictionary moves no tile");
            }
            // the tiles cover a level exactly once (the kernel's arithmetic: block at x = 0 is tile * owned - halo_left)
            for (int64_t ne : {(int64_t)1, (int64_t)p.owned - 1, (int64_t)p.owned, (int64_t)p.owned + 1, 2 * (int64_t)p.owned + 1}) {
              if (ne < 1) continue;
              const int64_t nt = (ne + p.owned - 1) / p.owned;
              std::vector<int> cover((size_t)ne, 0);
              for (int64_t t = 0; t < nt; ++t) {
                const int64_t e0 = t * p.owned - p.halo_left;
                for (int x = p.halo_left; x < p.halo_left + p.owned; ++x) {
                  EXPECT(x >= 0 && x < p.te, "owned x %d outside the tile", x);
                  const int64_t e = e0 + x;
                  if (e >= 0 && e < ne) ++cover[(size_t)e];
                }
              }
              for (int64_t e = 0; e < ne; ++e)
                if (cover[(size_t)e] != 1) {
                  EXPECT(false, "m %d S %d kind %d rho %d ne %lld: block %lld covered %d times", m, S, kind, rho, (long long)ne, (long long)e,
                         cover[(size_t)e]);
                  break;
                }
            }
          }
    // a launch of up to max_sweeps sweeps always has a tile (ratio 1)
    for (int S = 0; covered && S <= smax; ++S)
      for (int kind : {0, 1, 2})
        for (int kb : {1, 2, 4, 8})
          EXPECT(chain_multi_tile_plan(m, S, kind, 1, kb).owned > 0, "m %d S %d kind %d kb %d: no tile within max_sweeps", m, S, kind, kb);
  }
  EXPECT(tiles > 0, "no launch had a tile");
  // the fine descent of the config-5 shape, V(3,3): 64 blocks less 5 on the left and 4 on the right
  EXPECT(chain_multi_tile_plan(4, 3, kChainToChain, 1, 8).owned == 55, "owned %d", chain_multi_tile_plan(4, 3, kChainToChain, 1, 8).owned);
  // outside the coverage: no tile
  EXPECT(chain_multi_tile_plan(4, -1, 0, 1, 8).owned == 0 && chain_multi_tile_plan(4, 3, 3, 1, 8).owned == 0 &&
             chain_multi_tile_plan(4, 3, -1, 1, 8).owned == 0 && chain_multi_tile_plan(4, 3, 2, 0, 8).owned == 0 &&
             chain_multi_tile_plan(0, 3, 0, 1, 8).owned == 0 && chain_multi_tile_plan(4, 3, 0, 1, 16).owned == 0,
         "arguments outside the coverage have a tile");
  if (failures) {
    std::printf("chain_multi_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("chain_multi_plan OK\n");
  return 0;
}
