// Host-only unit test of the library's planning arithmetic (agglomerationmultigrid1d_amd/csrc/host_plan.hpp), built with
// g++ -fsanitize=address,undefined and run by tests/test_sanitizers_cpu.py -- no device, no HIP.  Every check is a
// property the kernels rely on: LDS regions that do not overlap and fit the CU, tile subsets that cover every tile
// exactly once, copy slices that partition the byte range, one chunk route for all ranks.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../agglomerationmultigrid1d_amd/csrc/host_plan.hpp"

using namespace aggmg;

static int failures = 0;
#define EXPECT(c)                                                          \
  do {                                                                     \
    if (!(c)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #c); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static void check_stage(const CrStagePlan& S, int m) {
  EXPECT(S.nsteps >= (S.q > 0 ? 1 : 0) && S.nsteps <= kCrMaxSteps);
  EXPECT(S.step_a[0] == 0 && S.step_a[S.nsteps] == S.q);
  const int Q = m <= 4 ? 3 : 2;
  std::vector<char> used((size_t)S.lds_total, 0);
  auto claim = [&](int off, int cnt) {
    EXPECT(off >= 0 && off + cnt <= S.lds_total);
    for (int i = off; i < off + cnt && i < S.lds_total; ++i) {
      EXPECT(!used[(size_t)i]);
      used[(size_t)i] = 1;
    }
  };
  for (int s = 1; s <= S.nsteps; ++s) {
    EXPECT(S.step_a[s] - S.step_a[s - 1] >= 1 && S.step_a[s] - S.step_a[s - 1] <= Q);
    const int cnt = ((1 << (S.q - S.step_a[s])) + 1) * m;
    claim(S.lds_off[s], 2 * cnt);   // right-hand sides of the step's output level (two per block)
    claim(S.lds_xoff[s], cnt);      // its solution
  }
  for (char u : used) EXPECT(u);    // no holes either
  EXPECT((size_t)S.lds_total * sizeof(double) <= kCrLdsBudgetBytes);   // what a launch may ask for (the CU's 160 KB)
  int64_t prev_end = 0;
  for (int s = 0; s < S.nsteps; ++s) {
    EXPECT(S.mid_off[s] == prev_end && (S.mid_off[s] & 1) == 0);   // regions back to back, 16-byte aligned
    const int qs = S.step_a[s + 1] - S.step_a[s];
    const int64_t need = ((S.n_in >> S.step_a[s + 1]) + 1) * (((int64_t)1 << (qs - 1)) - 1) * m;
    const int64_t end = s + 1 < S.nsteps ? S.mid_off[s + 1] : S.mid_total;
    EXPECT(end - S.mid_off[s] >= need);
    prev_end = end;
  }
}

static void test_cr_plans() {
  for (int m = 1; m <= 8; ++m)
    for (int q = 1; q <= cr_max_stage_levels(m); ++q) {   // (the planner keeps q within the LDS budget)
      CrStagePlan S;
      S.q = q;
      S.n_in = ((int64_t)1 << q) * 37 + 5;
      S.n_out = S.n_in >> q;
      cr_plan_steps(&S, m);
      check_stage(S, m);
    }
  // whole solves: the systems of the benchmarked hierarchies and awkward sizes
  const int64_t sizes[] = {1, 2, 3, 255, 256, 257, 1000, 4096, 4097, 65536, 1 << 20, (1 << 20) + 17, 1 << 24, (1 << 24) - 1};
  for (int m : {1, 2, 3, 4, 8})
    for (int64_t n0 : sizes)
      for (int max_q : {1, 4, 10, 12})
        for (int tail_rows : {8, 64, 4096}) {
          std::vector<int64_t> ln;
          for (int64_t n = n0; n > 1; n = (n + 1) / 2) ln.push_back(n);   // n -> even rows ceil(n / 2)
          CrSolvePlan P;
          const bool ok = cr_plan_solve(ln, m, tail_rows, max_q, 12, 256, &P);
          if (!ok) continue;
          int l = 0;
          for (const CrStagePlan& S : P.stages) {
            EXPECT(S.l0 == l && S.q >= 1 && S.q <= max_q && S.q <= cr_max_stage_levels(m));
            EXPECT(S.n_in == (l < (int)ln.size() ? ln[(size_t)l] : 1));
            l += S.q;
            EXPECT(S.n_out == (l < (int)ln.size() ? ln[(size_t)l] : 1));
            check_stage(S, m);
          }
          EXPECT(P.tail.l0 == l && P.tail.q == (int)ln.size() - l && P.tail.q <= kCrMaxStageLevels);
          EXPECT(P.tail.n_in * m <= tail_rows || P.tail.n_in == 1);
          check_stage(P.tail, m);
        }
}

// the per-solve buffers of a plan: one column as set-up allocates them, a group of columns in one allocation
static void test_cr_buffers() {
  struct Case {
    int64_t n0;
    int m, tail_rows, max_q, stages;   // stages < 0: whatever the planner gives, at least one
  };
  const Case cases[] = {{4096, 2, 4096, 12, 1},            // one stage + tail
                        {1000, 1, 4096, 12, 0},            // tail only
                        {4096, 1, 16, 3, 3},               // three stages
                        {3000, 3, 4096, 12, 1},            // a block count that is no power of two
                        {5000, 3, 16, 3, -1},       {(1 << 14) + 7, 2, 32, 4, -1}, {1 << 15, 1, 64, 5, -1},
                        {5000, 8, 16, 3, -1},       {(1 << 16) + 1, 8, 4096, 12, -1}};
  for (const Case& c : cases) {
    std::vector<int64_t> ln;
    for (int64_t n = c.n0; n > 1; n = (n + 1) / 2) ln.push_back(n);
    CrSolvePlan P;
    EXPECT(cr_plan_solve(ln, c.m, c.tail_rows, c.max_q, 12, 256, &P));
    EXPECT(c.stages < 0 ? !P.stages.empty() : (int)P.stages.size() == c.stages);
    const int64_t m = c.m;
    // one column: the expressions set-up allocated by before there was a function for them
    for (const CrStagePlan& S : P.stages) {
      const CrStageBuffers b = cr_stage_buffers(S, c.m);
      EXPECT(b.part == ((S.n_out * m + 31) & ~(int64_t)31));
      EXPECT(b.part >= S.n_out * m && b.part % 32 == 0);
      EXPECT(b.stack == (S.stack_stride > 0 ? (S.n_out + 1) * (int64_t)S.stack_stride : 0));
      EXPECT(b.mid == S.mid_total);
    }
    EXPECT(cr_stage_buffers(P.tail, c.m).mid == P.tail.mid_total);
    // a group: regions back to back in the order part, stack, mid of every stage, then the tail's mid; every per-column
    // stride even and large enough for the column's buffer
    for (int64_t cols : {1, 3, 8}) {
      std::vector<CrMultiStage> st;
      CrMultiStage tail;
      const int64_t total = cr_multi_layout(P.stages, P.tail, c.m, cols, &st, &tail);
      EXPECT(st.size() == P.stages.size());
      int64_t o = 0;
      auto region = [&](int64_t stride, int64_t off, int64_t need) {
        EXPECT(off == o && stride % 2 == 0 && stride >= need && stride <= need + 1);
        o += cols * stride;
      };
      for (size_t s = 0; s < st.size() && s < P.stages.size(); ++s) {
        const CrStagePlan& S = P.stages[s];
        region(st[s].part, st[s].part_off, 3 * ((S.n_out * m + 31) & ~(int64_t)31));
        region(st[s].stack, st[s].stack_off, S.stack_stride > 0 ? (S.n_out + 1) * (int64_t)S.stack_stride : 0);
        region(st[s].mid, st[s].mid_off, S.mid_total);
      }
      EXPECT(tail.part == 0 && tail.stack == 0);
      region(tail.mid, tail.mid_off, P.tail.mid_total);
      EXPECT(o == total);
    }
  }
}

static void test_lds_cap() {
  EXPECT(cr_max_stage_levels(1) == 12 && cr_max_stage_levels(2) == 12 && cr_max_stage_levels(4) == 12);
  for (int m = 5; m <= 8; ++m) EXPECT(cr_max_stage_levels(m) == 11);   // 2^12-block chunks would ask for 164 ... 262 KB
  for (int m = 1; m <= 8; ++m) {
    const int q = cr_max_stage_levels(m);
    EXPECT(cr_stage_lds_bytes(q, m) <= kCrLdsBudgetBytes);
    EXPECT(q == kCrMaxStageLevels || cr_stage_lds_bytes(q + 1, m) > kCrLdsBudgetBytes);
  }
}

static void test_row_blocks() {
  // row-length patterns: uniform short rows (DG / CG operators), one long row among short ones, empty rows, growing rows
  unsigned seed = 12345u;
  auto rnd = [&](unsigned mod) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % mod; };
  for (int pattern = 0; pattern < 6; ++pattern)
    for (int64_t nrows : {(int64_t)1, (int64_t)7, (int64_t)1000, (int64_t)5000, (int64_t)70000}) {
      std::vector<int32_t> rp((size_t)nrows + 1, 0);
      for (int64_t i = 0; i < nrows; ++i) {
        int len = 0;
        switch (pattern) {
          case 0: len = 6; break;
          case 1: len = (i == nrows / 2) ? 10000 : 5; break;
          case 2: len = (int)rnd(3) == 0 ? 0 : 9; break;
          case 3: len = 1 + (int)(i % 40); break;
          case 4: len = (int)rnd(30); break;
          default: len = (i % 97 == 0) ? 5000 : 12; break;
        }
        rp[(size_t)i + 1] = rp[(size_t)i] + len;
      }
      const int max_nnz = 4096, max_rows = 1024;
      // (4096 / 1024: the r03 block shape; 1536 / 256: what csr_stream_kernel takes since r04 -- one row per thread)
      for (const auto& shape : {std::pair<int, int>{4096, 1024}, std::pair<int, int>{1536, 256}}) {
        const std::vector<int32_t> blk = stream_row_blocks(rp.data(), nrows, shape.first, shape.second);
        EXPECT(blk.front() == 0 && blk.back() == nrows);
        for (size_t k = 0; k + 1 < blk.size(); ++k) {
          const int r0 = blk[k], r1 = blk[k + 1];
          EXPECT(r1 > r0 && r1 - r0 <= shape.second);                                 // a partition into non-empty runs
          EXPECT(rp[(size_t)r1] - rp[(size_t)r0] <= shape.first || r1 == r0 + 1);     // that fit the LDS stage, or one long row
        }
      }
      // csr_band_kernel's tiles since r04 (setup.hip): S = 1 + 32 / bw sweeps at most 8, a block's rows plus (S - 1) bw halo
      // rows per side are at most 256 rows (window = 256 + 2 bw in band_row_blocks' terms) holding at most 2048 entries
      for (int bw : {1, 4, 7, 16, 32}) {
        const int S = std::max(2, std::min(8, 1 + 32 / bw));
        std::vector<int32_t> bb;
        if (!band_row_blocks(rp.data(), nrows, bw, S, 2048, 256 + 2 * bw, 256, &bb)) continue;
        EXPECT(bb.front() == 0 && bb.back() == nrows);
        const int64_t H = (int64_t)(S - 1) * bw;
        for (size_t k = 0; k + 1 < bb.size(); ++k) {
          const int64_t r0 = bb[k], r1 = bb[k + 1];
          EXPECT(r1 > r0);
          const int64_t lo = std::max<int64_t>(0, r0 - H), hi = std::min<int64_t>(nrows, r1 + H);
          EXPECT(hi - lo <= 256);                                    // one row of the tile per thread
          EXPECT(rp[(size_t)hi] - rp[(size_t)lo] <= 2048);           // 8 entries per thread in registers
        }
      }
      for (int bw : {1, 5, 32})
        for (int sweeps : {1, 4}) {
          const int window = 4 * 256 + 2 * 4 * 32;
          std::vector<int32_t> bb;
          const bool ok = band_row_blocks(rp.data(), nrows, bw, sweeps, max_nnz, window, max_rows, &bb);
          if (!ok) continue;
          EXPECT(bb.front() == 0 && bb.back() == nrows);
          const int64_t H = (int64_t)(sweeps - 1) * bw;
          for (size_t k = 0; k + 1 < bb.size(); ++k) {
            const int64_t r0 = bb[k], r1 = bb[k + 1];
            EXPECT(r1 > r0 && r1 - r0 <= max_rows);
            const int64_t lo = std::max<int64_t>(0, r0 - H), hi = std::min<int64_t>(nrows, r1 + H);
            EXPECT(rp[(size_t)hi] - rp[(size_t)lo] <= max_nnz);                     // block + halo rows fit the product stage
            EXPECT((r1 - r0) + 2 * (int64_t)sweeps * bw <= window);                 // and the window of x its LDS array
          }
        }
    }
}

static void test_tile_subsets() {
  for (int64_t ne : {1, 7, 100, 101, 1000, 4096, 100000})
    for (int owned : {1, 3, 64, 100, 122})
      for (int64_t head : {(int64_t)-5, (int64_t)0, (int64_t)1, (int64_t)80, ne / 2, ne, ne + 9})
        for (int64_t tail : {(int64_t)0, ne / 2, ne - 80, ne - 1, ne, ne + 3}) {
          const TileSubset all = fused_tile_subset(ne, owned, 0, head, tail);
          const TileSubset ends = fused_tile_subset(ne, owned, 1, head, tail);
          const TileSubset mid = fused_tile_subset(ne, owned, 2, head, tail);
          EXPECT(all.ntiles == (ne + owned - 1) / owned && all.split == 0 && all.skip == 0);
          std::multiset<int64_t> seen;
          for (const TileSubset* t : {&ends, &mid})
            for (int64_t b = 0; b < t->ntiles; ++b) seen.insert(b + (b >= t->split ? t->skip : 0));
          EXPECT((int64_t)seen.size() == all.ntiles);          // ends + middle = every tile ...
          int64_t want = 0;
          for (int64_t tile : seen) EXPECT(tile == want++);     // ... exactly once
          // the interface elements are in the "ends" launch
          const int64_t h = std::min(std::max<int64_t>(head, 0), ne), tl = std::min(std::max(tail, h), ne);
          std::set<int64_t> e;
          for (int64_t b = 0; b < ends.ntiles; ++b) e.insert(b + (b >= ends.split ? ends.skip : 0));
          for (int64_t x : {(int64_t)0, h - 1, tl, ne - 1})
            if (x >= 0 && x < ne && (x < h || x >= tl)) EXPECT(e.count(x / owned) == 1);
        }
}

// the tile constants the library uses (BtdTile<M>::TE for M = 1 .. 9, the K-column tiles, the two-level tiles) and a few others
static const int kSingleTE[] = {512, 128, 255, 153, 126, 108, 64, 56, 32, 17, 1000};
static const int kRatios[] = {2, 3, 4, 5, 7, 8, 12, 13, 16, 31, 32, 60, 64};

// ceil(ne / own) tiles of `own` elements cover [0, ne): back to back, the last one clipped
static void check_cover(int64_t ne, int own) {
  const int64_t ntiles = (ne + own - 1) / own;
  int64_t at = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    EXPECT(t * own == at && at < ne);
    at = std::min<int64_t>((t + 1) * own, ne);
  }
  EXPECT(at == ne);
}

static void test_fused_tile_plan() {
  for (int te : kSingleTE)
    for (int ns = 0; ns <= 8; ++ns)
      for (int halo : {ns, ns + 1, 2 * ns, 2 * ns + 1}) {   // sweeps (+ a residual), Gauss-Seidel: two half-sweeps each
        for (int rho : kRatios) {   // restriction to uniform agglomerates
          const FusedTilePlan p = fused_tile_plan(te, halo, rho, false, -1);
          EXPECT(p.owned >= 0 && p.agg_shift == -1);
          if (p.owned > 0) {
            EXPECT(p.owned % rho == 0 && p.halo_left == halo && p.halo_left + p.owned + halo <= te);
            for (int64_t ne : {(int64_t)rho, (int64_t)rho * 37, (int64_t)rho * 4096}) check_cover(ne, p.owned);
          }
          EXPECT(multi_tile_owned(te, halo, rho) == p.owned);   // the K-column tile: the same arithmetic
        }
        for (int shift = -1; shift <= 9; ++shift) {   // agglomerates of different sizes, the largest of shift + 1 elements
          const FusedTilePlan p = fused_tile_plan(te, halo, 1, true, shift);
          EXPECT(p.owned >= 0 && (p.agg_shift == -1 || p.agg_shift == shift));
          if (p.owned == 0) continue;
          EXPECT(p.halo_left >= halo && p.halo_left + p.owned + halo <= te);
          // moved onto agglomerate boundaries: a tile may start up to `shift` elements early and still owns half of itself
          if (p.agg_shift >= 0) EXPECT(p.halo_left == halo + shift && p.owned >= te / 2 - 1);
          else EXPECT(p.halo_left == halo);
          for (int64_t ne : {(int64_t)1, (int64_t)777, (int64_t)100000}) check_cover(ne, p.owned);
        }
        EXPECT(fused_tile_plan(te, halo, 1, false, 3).agg_shift == -1);   // no shift without such agglomerates
      }
  EXPECT(fused_tile_plan(16, 8, 1, false, -1).owned == 0 && fused_tile_plan(16, 9, 2, false, -1).owned == 0);   // no room: no tile
}

static void test_pair_plans() {
  const std::pair<int, int> tiles[] = {{256, 128}, {384, 256}, {512, 256}, {128, 128}, {100, 40}};   // (TEA, TEB); the first: the library's
  for (auto [tea, teb] : tiles)
    for (int ns = 0; ns <= 8; ++ns)
      for (int ra : kRatios)
        for (int rb : kRatios) {
          const PairTilePlan d = pair_down_plan(ns, ra, rb, tea, teb);
          const int hh = ns + 1;   // the sweeps and the residual
          EXPECT(d.own >= 0);
          if (d.own == 0) {
            EXPECT(d.te_a == 0 && d.te_b == 0);   // "no tile" never looks like a size
          } else {
            EXPECT(d.own % rb == 0 && d.te_a <= tea && d.te_b <= teb);
            EXPECT(d.te_b >= d.own + 2 * hh && d.te_a >= d.te_b * ra + 2 * hh);   // B's tile with its halo, A's around B's
            check_cover((int64_t)rb * 1000, d.own);
          }
          const PairTilePlan u = pair_up_plan(ns, ra, tea, teb);
          EXPECT(u.own >= 0);
          if (u.own == 0) {
            EXPECT(u.te_a == 0 && u.te_b == 0);
            continue;
          }
          EXPECT(u.own % ra == 0 && u.te_a <= tea && u.te_b <= teb && u.hb * ra >= ns);
          EXPECT(u.te_a >= u.own + 2 * ns && u.te_b >= u.own / ra + 2 * u.hb + 2 * ns);
          check_cover((int64_t)ra * rb * 300, u.own);
          // the ascent in two parts around the ghosts of the coarsest level
          if (tea > 384) continue;   // (the library's tiles and one other pair: the check below walks every tile)
          for (int64_t nec : {(int64_t)1, (int64_t)2, (int64_t)9, (int64_t)40}) {
            const int64_t ne_b = nec * rb, ne = ne_b * ra;
            for (int64_t gh_lo : {(int64_t)0, (int64_t)1, (int64_t)3, nec})
              for (int64_t gh_hi : {(int64_t)0, (int64_t)1, (int64_t)4, nec}) {
                PairTilePlan s = u;
                pair_up_split(&s, ns, ra, rb, ne, nec, gh_lo, gh_hi);
                EXPECT(s.all == (ne + s.own - 1) / s.own && s.tA >= 0 && s.tB >= 0 && s.tA + s.tB <= s.all);
                // parts 1 and 2 as the launch numbers them: workgroup b runs tile b + (b >= split ? skip : 0)
                std::multiset<int64_t> seen;
                for (int64_t b = 0; b < s.tA + s.tB; ++b) seen.insert(b + (b >= s.tA ? s.all - s.tA - s.tB : 0));
                for (int64_t b = 0; b < s.all - s.tA - s.tB; ++b) seen.insert(b + s.tA);
                EXPECT((int64_t)seen.size() == s.all);
                int64_t want = 0;
                for (int64_t tile : seen) EXPECT(tile == want++);
                // no part-2 tile reads a ghost: from the definition, element by element of the tile's window of B
                for (int64_t t = s.tA; t < s.all - s.tB; ++t) {
                  const int64_t e0 = t * s.own / ra - s.hb - ns;
                  for (int64_t e = e0; e < e0 + s.te_b; ++e) {
                    const int64_t j = std::min(std::max<int64_t>(e, 0), ne_b - 1) / rb;
                    EXPECT(j >= gh_lo && j < nec - gh_hi);
                  }
                }
              }
          }
        }
  // the library's tiles (256, 128): ratios (4, 16, 16) at V(3,3) -- levels 1 and 2 both agglomerate by 16 -- and equal
  // ratios of 13 and above at 3 sweeps, of 9 and above at 8, have no descent tile
  EXPECT(pair_down_plan(3, 16, 16, 256, 128).own == 0);
  for (int r = 13; r <= 64; ++r) EXPECT(pair_down_plan(3, r, r, 256, 128).own == 0);
  for (int r = 9; r <= 64; ++r) EXPECT(pair_down_plan(8, r, r, 256, 128).own == 0);
  EXPECT(pair_down_plan(3, 4, 4, 256, 128).own > 0 && pair_down_plan(3, 2, 2, 256, 128).own > 0);   // the benchmarked ratios have one
}

// "does this launch have a tile" (launch_has_tile, what the callers that choose a launch ask) against the planner the
// launcher runs, over every launch kind; and the ratios the library's tiles have none for, pinned
static void test_launch_has_tile() {
  for (int te : kSingleTE)
    for (int halo = 0; halo <= 17; ++halo)
      for (int align = 1; align <= te + 1; ++align) {
        TileQuery q;
        q.te = te;
        q.halo = halo;
        q.align = align;
        EXPECT(launch_has_tile(q) == (fused_tile_plan(te, halo, align, false, -1).owned > 0));
        EXPECT(launch_has_tile(q) == (te - 2 * halo >= align));   // room for one agglomerate between the halos
        q.launch = kTileMulti;
        EXPECT(launch_has_tile(q) == (multi_tile_owned(te, halo, align) > 0));
        if (align > 10) continue;
        q.launch = kTileFused;
        q.align = 1;
        q.var_agg = true;
        q.agg_shift = align - 2;   // -1 .. 8
        EXPECT(launch_has_tile(q) == (fused_tile_plan(te, halo, 1, true, align - 2).owned > 0));
      }
  const std::pair<int, int> tiles[] = {{256, 128}, {384, 256}, {128, 128}, {100, 40}};
  for (auto [tea, teb] : tiles)
    for (int ns = 0; ns <= 9; ++ns)
      for (int ra = 1; ra <= 66; ++ra)
        for (int rb = 1; rb <= 66; ++rb) {
          TileQuery q;
          q.launch = kTilePairDown;
          q.te = tea;
          q.te_b = teb;
          q.halo = ns;
          q.align = ra;
          q.rho_bc = rb;
          EXPECT(launch_has_tile(q) == (pair_down_plan(ns, ra, rb, tea, teb).own > 0));
          q.launch = kTilePairUp;
          EXPECT(launch_has_tile(q) == (pair_up_plan(ns, ra, tea, teb).own > 0));
        }
  // the library's two-level tiles (256, 128): descents without a tile at V(3,3) -- te_b < 2 (nPre + 1) makes the plan's
  // numerator negative for (32, 2) -- and the ones that lose theirs at 8 sweeps
  auto down = [](int ns, int ra, int rb) {
    TileQuery q;
    q.launch = kTilePairDown;
    q.te = 256;
    q.te_b = 128;
    q.halo = ns;
    q.align = ra;
    q.rho_bc = rb;
    return launch_has_tile(q);
  };
  const std::pair<int, int> none3[] = {{16, 8}, {16, 16}, {13, 13}, {12, 16}, {8, 32}, {4, 64}, {31, 2}, {32, 2}};
  for (auto [ra, rb] : none3) EXPECT(!down(3, ra, rb));
  const std::pair<int, int> none8[] = {{12, 2}, {5, 32}, {3, 64}};
  for (auto [ra, rb] : none8) EXPECT(down(3, ra, rb) && !down(8, ra, rb));
  EXPECT(down(3, 12, 12) && down(3, 8, 8) && down(3, 4, 4) && down(3, 2, 2));
  {  // ... while the ascent of (16, 16) has one: the two directions are decided apart
    TileQuery q;
    q.launch = kTilePairUp;
    q.te = 256;
    q.te_b = 128;
    q.halo = 3;
    q.align = 16;
    EXPECT(launch_has_tile(q));
  }
  // single-level launches: ratio 128 never fits the 128-element tile; ratio 52 fits the 64-element tile of block size 8
  // in a V(3,3) descent (halo 4) and not in the launch between two cycles (halo 7)
  auto fused = [](int te, int halo, int rho) {
    TileQuery q;
    q.te = te;
    q.halo = halo;
    q.align = rho;
    return launch_has_tile(q);
  };
  EXPECT(!fused(128, 4, 128) && !fused(128, 0, 129) && fused(128, 4, 120));
  EXPECT(fused(64, 4, 52) && !fused(64, 7, 52));
}

// Room for the partial sums of checkpoint launches (fused_chk_reserve / chain_chk_reserve): no launch the reservation
// was made for runs more tiles.  The formulas they replace -- 2 ne / TE + 2 and 4 ne / TE + 2, i.e. "a tile owns at
// least half (a quarter) of itself" -- are swept alongside: the first must be seen to fall short (a ratio just under
// TE / 2 - halo leaves a tile ONE agglomerate), or this test would not have caught the defect it was written for.
static void test_chk_reserve() {
  struct Shipped { int m, te; };
  const Shipped btd[] = {{1, 512}, {2, 128}, {3, 255}, {4, 128}, {5, 153}, {6, 126}, {7, 108}, {8, 64}, {9, 56}};   // BtdTile<M>::TE
  int64_t old_short = 0;
  bool shown = false;
  for (const Shipped& t : btd) {
    const int smax = std::min(8, t.te / 8);   // sweeps of one launch (btd_max_sweeps)
    for (int sweeps = 1; sweeps <= smax; ++sweeps)
      for (int align = 1; align <= t.te; ++align) {
        const int own_min = fused_tile_plan(t.te, sweeps + 1, align, false, -1).owned;
        for (int64_t ne : {(int64_t)1, (int64_t)own_min - 1, (int64_t)own_min, (int64_t)own_min + 1, (int64_t)align * 37,
                           (int64_t)1920, (int64_t)7680, (int64_t)align * 4099, (int64_t)1 << 24}) {
          if (ne < 1) continue;
          const int64_t reserved = fused_chk_reserve(ne, t.te, sweeps + 1, align, false, -1);
          const int64_t old_reserved = 2 * ne / t.te + 2;
          EXPECT(reserved >= 1);
          for (int halo = 1; halo <= sweeps + 1; ++halo)     // any launch with at most these sweeps (+ 1: residual rows)
            for (int a : {align, 1}) {                       // the one between two cycles restricts, the others do not
              const int owned = fused_tile_plan(t.te, halo, a, false, -1).owned;
              if (owned <= 0) continue;                      // no tile: the callers take the unfused sequence
              const int64_t ntiles = fused_tile_subset(ne, owned, 0, 0, 0).ntiles;
              EXPECT(ntiles <= reserved);
              if (ntiles > old_reserved) {
                ++old_short;
                if (!shown && t.te == 128 && halo == 7 && a == 60 && ne == 7680) {
                  std::printf("chk reserve, former formula 2 ne / TE + 2: TE %d halo %d ratio %d ne %lld -> %lld tiles > %lld reserved\n",
                              t.te, halo, a, (long long)ne, (long long)ntiles, (long long)old_reserved);
                  shown = true;
                }
              }
            }
        }
      }
    // agglomerates of different sizes: the owned size is not monotone in the halo (a tile that can no longer afford the
    // shift drops it)
    for (int sweeps = 1; sweeps <= smax; ++sweeps)
      for (int shift = -1; shift <= 8; ++shift)
        for (int64_t ne : {(int64_t)1, (int64_t)777, (int64_t)100000}) {
          const int64_t reserved = fused_chk_reserve(ne, t.te, sweeps + 1, 1, true, shift);
          for (int halo = 1; halo <= sweeps + 1; ++halo) {
            const int owned = fused_tile_plan(t.te, halo, 1, true, shift).owned;
            if (owned > 0) EXPECT(fused_tile_subset(ne, owned, 0, 0, 0).ntiles <= reserved);
          }
        }
  }
  EXPECT(old_short > 0 && shown);   // p = 3, ratios (60, 2), n = 7680: 128 tiles against 122
  EXPECT(fused_tile_subset(7680, fused_tile_plan(128, 7, 60, false, -1).owned, 0, 0, 0).ntiles == 128);
  EXPECT(fused_chk_reserve(7680, 128, 7, 60, false, -1) >= 128);
  // the default ratios reserve no more than before
  EXPECT(fused_chk_reserve((int64_t)1 << 24, 128, 7, 4, false, -1) <= 2 * ((int64_t)1 << 24) / 128 + 2);

  // the chain kernel (CgtTile<M>::TE, point-Jacobi): hl + hr = 2 sweeps + 2 (checkpoint after the last sweep) or + 3
  // (residual and restriction); owned = chain_tile_owned, the launcher's own arithmetic
  const Shipped cgt[] = {{1, 256}, {2, 128}, {3, 85}, {4, 64}, {5, 153}, {6, 126}, {7, 108}, {8, 64}};
  int64_t old_chain_short = 0;
  for (const Shipped& t : cgt) {
    const int smax = std::max(1, std::min(8, t.te / 8));
    for (int sweeps = 1; sweeps <= smax; ++sweeps)
      for (int align = 1; align <= t.te; ++align)
        for (int64_t ne : {(int64_t)1, (int64_t)align, (int64_t)align * 37, (int64_t)7680, (int64_t)align * 4099, (int64_t)1 << 24}) {
          const int64_t reserved = chain_chk_reserve(ne, t.te, 2 * sweeps + 3, align);
          for (int s = 1; s <= sweeps; ++s)
            for (int extra : {2, 3})
              for (int a : {align, 1}) {
                const int hs = 2 * s + extra;
                for (int hl : {hs / 2, hs - hs / 2}) {   // the odd block goes left (chain) or right (agglomerating)
                  const int owned = chain_tile_owned(t.te, hl, hs - hl, a);
                  if (owned <= 0) continue;
                  const int64_t ntiles = (ne + owned - 1) / owned;
                  EXPECT(ntiles <= reserved);
                  if (ntiles > 4 * ne / t.te + 2) ++old_chain_short;
                }
              }
        }
  }
  std::printf("chk reserve, former chain formula 4 ne / TE + 2: short in %lld swept launches\n", (long long)old_chain_short);
}

static void test_lane_ranges() {
  for (size_t bytes : {(size_t)0, (size_t)1, (size_t)4095, (size_t)4096, (size_t)(16u << 20), (size_t)134217728, (size_t)134217729})
    for (int lanes = 1; lanes <= 8; ++lanes) {
      size_t at = 0;
      for (int t = 0; t < lanes; ++t) {
        size_t lo = 0, hi = 0;
        stage_lane_range(bytes, lanes, t, &lo, &hi);
        EXPECT(lo <= hi && hi <= bytes);
        if (hi > lo) {
          EXPECT(lo == at);               // slices back to back
          EXPECT(t == 0 || lo % 4096 == 0);   // on page boundaries
          at = hi;
        }
      }
      EXPECT(at == bytes);
    }
}

static void test_chunk_route() {
  // an even partition into whole chunks: every rank says "chunked"
  for (int world : {1, 2, 3, 4, 8})
    for (int q : {1, 4, 10}) {
      const int64_t per = ((int64_t)1 << q) * 3, ne = per * world;
      for (int r = 0; r < world; ++r) EXPECT(dist_chunk_route(q, 2, ne, 2, ne, world, r, r * per, (r + 1) * per) == 1);
      // same level, ranks owning 4, 3, 5 ... chunks: the ranks off the pattern are refused, none silently gathers
      if (world >= 2) {
        EXPECT(dist_chunk_route(q, 2, ne, 2, ne, world, 0, 0, per + ((int64_t)1 << q)) == -1);
        EXPECT(dist_chunk_route(q, 2, ne, 2, ne, world, 1, per + ((int64_t)1 << q), 2 * per) == -1);
      }
      // no plan, another block size, a level that does not divide: every rank gathers, whatever it owns
      for (int r = 0; r < world; ++r) {
        EXPECT(dist_chunk_route(-1, 2, ne, 2, ne, world, r, r * per, (r + 1) * per) == 0);
        EXPECT(dist_chunk_route(q, 1, ne, 2, ne, world, r, r * per, (r + 1) * per) == 0);
        EXPECT(dist_chunk_route(q, 2, ne + 1, 2, ne + 1, world, r, r * per, (r + 1) * per) == 0 || world == 1);
        EXPECT(dist_chunk_route(q + 3, 2, ne, 2, ne, world, r, r * per, (r + 1) * per) == 0);   // fewer than one chunk per rank / not whole
      }
    }
}

// forms.hpp: the dispatchers call f exactly once, with the run-time form, for every form of the predicate and never else
static void test_form_dispatch() {
  for (int m = -1; m <= kMaxBlock + 2; ++m) {
    for (int cmp = 0; cmp <= 1; ++cmp) {
      int calls = 0, gm = 0, gc = -1;
      const bool hit = with_form<patch_form>(m, cmp != 0, [&](auto f) {
        ++calls;
        gm = decltype(f)::kM;
        gc = decltype(f)::kCmp ? 1 : 0;
      });
      EXPECT(hit == patch_form(m, cmp != 0) && calls == (hit ? 1 : 0) && (!hit || (gm == m && gc == cmp)));
    }
    int calls = 0, gm = 0;
    const bool hit = with_block_size<chain_dict_form>(m, [&](auto n) {
      ++calls;
      gm = decltype(n)::value;
    });
    EXPECT(hit == chain_dict_form(m) && calls == (hit ? 1 : 0) && (!hit || gm == m));
  }
  for (int ceiling : {1, 2, 4, 8})
    for (int kc = 1; kc <= ceiling; ++kc) {
      int kb = 0;
      with_col_group(kc, ceiling, [&](auto g) { kb = decltype(g)::value; });
      EXPECT(kb == col_group(kc, ceiling) && kb >= kc && kb <= ceiling && is_col_group(kb) && (kb == 1 || kb / 2 < kc));
    }
}

int main() {
  test_cr_plans();
  test_cr_buffers();
  test_lds_cap();
  test_row_blocks();
  test_tile_subsets();
  test_fused_tile_plan();
  test_pair_plans();
  test_launch_has_tile();
  test_chk_reserve();
  test_lane_ranges();
  test_chunk_route();
  test_form_dispatch();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("host_plan OK");
  return 0;
}
