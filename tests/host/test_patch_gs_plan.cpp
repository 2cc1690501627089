// Host-compiled test of the tile planner of the multiplicative two-colour patch sweeps
// (agglomerationmultigrid1d_amd/csrc/host_plan.hpp: patch_gs_tile_plan, patch_gs_max_sweeps, chunking through
// patch_chunks) under AddressSanitizer + UBSan: no device, no HIP.  For m = 1 .. 8 and S = 1 .. 8: owned > 0 where a
// launch is offered, the halo is at least the reach of S sweeps -- computed here by walking the definition's dependences,
// both directions, both parities -- the LDS fits a compute unit, the tiles cover [0, ne) exactly once, and the chunks of a
// run of sweeps add up.
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

// The elements the value of element `at` depends on after S sweeps on a level of ne elements, as [lo, hi]: a half-sweep
// of colour c gives an element covered by a patch {p, p + 1}, p = c (mod 2), the residuals of p and p + 1, i.e. the
// values of p - 1 .. p + 2 (inside the level); an element no patch of the colour covers keeps its own.
static void reach(int ne, int S, bool reverse, int at, int* lo, int* hi) {
  std::vector<int> L(ne), H(ne), L2(ne), H2(ne);
  for (int e = 0; e < ne; ++e) L[e] = H[e] = e;
  for (int s = 0; s < S; ++s)
    for (int h = 0; h < 2; ++h) {
      const int c = reverse ? 1 - h : h;
      for (int e = 0; e < ne; ++e) {
        int p = -1;   // the patch of colour c covering e
        if (e % 2 == c && e <= ne - 2) p = e;
        else if (e % 2 != c && e >= 1) p = e - 1;
        L2[e] = L[e];
        H2[e] = H[e];
        if (p < 0) continue;
        for (int q = std::max(0, p - 1); q <= std::min(ne - 1, p + 2); ++q) {
          L2[e] = std::min(L2[e], L[q]);
          H2[e] = std::max(H2[e], H[q]);
        }
      }
      L = L2;
      H = H2;
    }
  *lo = L[at];
  *hi = H[at];
}

int main() {
  constexpr size_t kLdsBytes = 160 * 1024;   // of a gfx950 compute unit
  // the reach of S sweeps, well inside a long level: the most over both parities and both directions
  int reach_of[kPatchMaxSweeps + 1] = {0};
  for (int S = 1; S <= kPatchMaxSweeps; ++S)
    for (int reverse = 0; reverse < 2; ++reverse)
      for (int at = 40; at < 42; ++at) {
        int lo, hi;
        reach(81, S, reverse != 0, at, &lo, &hi);
        reach_of[S] = std::max({reach_of[S], at - lo, hi - at});
      }
  EXPECT(reach_of[1] == 3 && reach_of[2] == 5, "reach of one / two sweeps: %d / %d", reach_of[1], reach_of[2]);

  for (int m = 1; m <= 8; ++m) {
    const int smax = patch_gs_max_sweeps(m);
    EXPECT(smax >= 1 && smax <= kPatchMaxSweeps, "m %d smax %d", m, smax);
    for (int S = 1; S <= 8; ++S) {
      const PatchTilePlan p = patch_gs_tile_plan(m, S);
      EXPECT(p.te == patch_tile_elems(m), "m %d S %d", m, S);
      EXPECT(p.halo == patch_gs_halo(S) && p.halo >= reach_of[S], "m %d S %d halo %d reach %d", m, S, p.halo, reach_of[S]);
      EXPECT(p.halo <= 3 * S, "m %d S %d halo %d", m, S, p.halo);
      EXPECT(p.owned >= 0 && (p.owned == 0 || p.owned + 2 * p.halo == p.te), "m %d S %d owned %d", m, S, p.owned);
      EXPECT(p.lds_bytes == (size_t)2 * (p.te + 2) * m * 8 && p.lds_bytes <= kLdsBytes, "m %d S %d lds %zu", m, S, p.lds_bytes);
      if (S <= smax) EXPECT(p.owned >= 1, "m %d S %d <= smax %d has no tile", m, S, smax);
      if (S <= smax && S > 1) EXPECT(2 * p.owned >= p.te, "m %d S %d: halos take more than half the tile", m, S);
      if (S == smax && S < kPatchMaxSweeps)
        EXPECT(2 * patch_gs_owned(p.te, S + 1) < p.te, "m %d: smax %d could be larger", m, smax);
      TileQuery q;
      q.launch = kTilePatchGs;
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
          // what the owned elements read after S sweeps, all held by the tile
          EXPECT(p.halo - reach_of[S] >= 0 && p.halo + p.owned - 1 + reach_of[S] < p.te, "m %d S %d: reach leaves the tile", m, S);
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
        EXPECT(s >= 1 && s <= smax && patch_gs_tile_plan(m, s).owned > 0, "m %d n %d chunk %d takes %d", m, n, c, s);
        sum += s;
      }
      EXPECT(sum == n, "m %d: chunks of %d sweeps add up to %d", m, n, sum);
    }
  }
  // short levels and the level's ends: the reach never exceeds the halo there either
  for (int ne = 2; ne <= 24; ++ne)
    for (int S = 1; S <= 4; ++S)
      for (int reverse = 0; reverse < 2; ++reverse)
        for (int at = 0; at < ne; ++at) {
          int lo, hi;
          reach(ne, S, reverse != 0, at, &lo, &hi);
          EXPECT(at - lo <= patch_gs_halo(S) && hi - at <= patch_gs_halo(S), "ne %d S %d at %d: [%d, %d]", ne, S, at, lo, hi);
        }
  EXPECT(patch_gs_tile_plan(4, 0).owned == 0 && patch_gs_tile_plan(4, 9).owned == 0, "sweep counts outside 1 .. 8 have no tile");
  EXPECT(patch_gs_max_sweeps(0) == 0, "m = 0");
  if (failures) {
    std::printf("patch_gs_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("patch_gs_plan OK\n");
  return 0;
}
