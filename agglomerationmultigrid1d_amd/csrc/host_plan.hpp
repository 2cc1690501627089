// Host-only planning arithmetic of libaggmg_hip.so -- no HIP types, no device calls: the pieces of the launch logic
// that decide index ranges, LDS layouts, tile subsets and copy slices.  Kept apart so that a host-compiled test
// (tests/host/test_host_plan.cpp) can drive them under AddressSanitizer / UBSan without a device (SURVEY.md
// section 5: sanitizers on the CPU build only); the .hip files use exactly these functions.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "forms.hpp"

namespace aggmg {

constexpr int kCrTailRows = 4096;  // scalar rows (blocks * m) the single-workgroup tail takes
constexpr int kCrMaxLevels = 40;
constexpr int kCrMaxStageLevels = 12;
constexpr int kCrMaxSteps = 8;

// ---- coarsest solve (src/solvers.jl:39): one launch of the cyclic reduction -----------------------------------
// levels [l0, l0 + q) of the reduction in steps of up to three thread-local levels (cr_kernels.hpp): step split,
// LDS layout, strides of the per-chunk stack and of the stored inner right-hand sides
struct CrStagePlan {
  int l0 = 0, q = 0;
  int64_t n_in = 0, n_out = 0;  // blocks before / after
  int nsteps = 0;
  int step_a[kCrMaxSteps + 1] = {0};
  int lds_off[kCrMaxSteps + 1] = {0}, lds_xoff[kCrMaxSteps + 1] = {0};
  int lds_total = 0;            // doubles
  int stack_stride = 0;
  int64_t mid_off[kCrMaxSteps + 1] = {0};
  int64_t mid_total = 0;        // doubles
};

// step split and LDS layout of a stage of q levels with block size m
inline void cr_plan_steps(CrStagePlan* S, int m) {
  const int Q = m <= 4 ? 3 : 2;
  S->nsteps = 0;
  S->step_a[0] = 0;
  for (int a = 0; a < S->q;) {
    const int qs = std::min(Q, S->q - a);
    a += qs;
    S->step_a[++S->nsteps] = a;
  }
  int o = 0;
  for (int s = 1; s <= S->nsteps; ++s) {
    const int cnt = ((1 << (S->q - S->step_a[s])) + 1) * m;
    S->lds_off[s] = o;
    o += 2 * cnt;
  }
  for (int s = 1; s <= S->nsteps; ++s) {
    const int cnt = ((1 << (S->q - S->step_a[s])) + 1) * m;
    S->lds_xoff[s] = o;
    o += cnt;
  }
  S->lds_total = o;
  S->stack_stride = 0;
  for (int s = 1; s < S->nsteps; ++s) S->stack_stride += ((1 << (S->q - S->step_a[s])) + 1) * m;
  // sub-chunk b of step s (a block index of the step's output level: at most (n_in >> a1) + 1 of them) keeps
  // 2^(qs-1) - 1 blocks; every region 16-byte aligned
  S->mid_total = 0;
  for (int s = 0; s < S->nsteps; ++s) {
    const int qs = S->step_a[s + 1] - S->step_a[s];
    S->mid_off[s] = S->mid_total;
    const int64_t cnt = ((S->n_in >> S->step_a[s + 1]) + 2) * (((int64_t)1 << (qs - 1)) - 1) * m;
    S->mid_total += (cnt + 1) & ~(int64_t)1;
  }
}

// LDS of a stage of q levels: two right-hand-side vectors and a solution per block of every step's output level, the
// first step's (2^(q - Q) + 1 blocks) dominating.  A stage must fit the LDS of a compute unit (gfx950: 160 KB, one
// workgroup per CU then): chunks of 2^12 blocks do up to block size 4 (55 KB); block sizes 5 - 8 would ask for
// 164 ... 262 KB -- a launch failure, on systems of 2^20 blocks and more -- and take chunks of 2^11.
constexpr size_t kCrLdsBudgetBytes = 160 * 1024;
inline size_t cr_stage_lds_bytes(int q, int m) {
  CrStagePlan S;
  S.q = q;
  cr_plan_steps(&S, m);
  return (size_t)S.lds_total * sizeof(double);
}
inline int cr_max_stage_levels(int m) {
  int q = kCrMaxStageLevels;
  while (q > 1 && cr_stage_lds_bytes(q, m) > kCrLdsBudgetBytes) --q;
  return q;
}

// Which launches a solve takes: chunk stages (one workgroup per 2^q-block chunk) until what is left fits the
// single-workgroup tail.  level_n[l] = blocks of reduction level l (level_n.size() = nl reducing levels; beyond
// them one block).  fill_max / min_workgroups: large chunks as long as a few hundred workgroups remain.
// -> false when the system cannot be planned (too many levels left for the tail).
struct CrSolvePlan {
  std::vector<CrStagePlan> stages;
  CrStagePlan tail;
};
inline bool cr_plan_solve(const std::vector<int64_t>& level_n, int m, int tail_rows, int max_q, int fill_max,
                          int min_workgroups, CrSolvePlan* out) {
  const int nl = (int)level_n.size();
  auto ln = [&](int l) -> int64_t { return l < nl ? level_n[l] : 1; };
  out->stages.clear();
  max_q = std::min(max_q, cr_max_stage_levels(m));
  int l0 = 0;
  while (l0 < nl && ln(l0) * m > tail_rows) {
    int need = 0;
    while (l0 + need < nl && ln(l0 + need) * m > tail_rows) ++need;
    int fill = 0;
    while (fill < fill_max && (ln(l0) >> (fill + 1)) >= min_workgroups) ++fill;
    CrStagePlan S;
    S.l0 = l0;
    S.q = std::min({max_q, std::max(need, fill), nl - l0});
    if (S.q < 1) break;
    S.n_in = ln(l0);
    S.n_out = ln(l0 + S.q);
    cr_plan_steps(&S, m);
    out->stages.push_back(S);
    l0 += S.q;
  }
  if (nl - l0 > kCrMaxStageLevels || ln(l0) * m > tail_rows) return false;
  out->tail = CrStagePlan();
  out->tail.l0 = l0;
  out->tail.q = nl - l0;
  out->tail.n_in = ln(l0);
  out->tail.n_out = 1;
  cr_plan_steps(&out->tail, m);
  return true;
}

// What one right-hand side needs of a stage besides the shared factors, in doubles: `part` = each of the three boundary
// vectors partR | partL | xq (n_out blocks, rounded up to 32 doubles: they share an allocation and each starts on 256
// bytes), the per-chunk stack (n_out + 1 chunks) and mid.  The tail takes mid alone.
struct CrStageBuffers {
  int64_t part = 0, stack = 0, mid = 0;
};
inline CrStageBuffers cr_stage_buffers(const CrStagePlan& S, int m) {
  CrStageBuffers b;
  b.part = (S.n_out * m + 31) & ~(int64_t)31;
  b.stack = S.stack_stride > 0 ? (S.n_out + 1) * (int64_t)S.stack_stride : 0;
  b.mid = S.mid_total;
  return b;
}

// The same buffers for a group of columns in ONE allocation: per stage the regions [cols][part] (partR | partL | xq of a
// column side by side), [cols][stack], [cols][mid], then the tail's [cols][mid]; every per-column stride even, so that
// every column starts on the 16 bytes the kernels' paired loads assume.  Stage: CrStagePlan or a type derived from it.
inline int64_t cr_even(int64_t v) { return (v + 1) & ~(int64_t)1; }
struct CrMultiStage {
  int64_t part = 0, stack = 0, mid = 0;              // doubles per column
  int64_t part_off = 0, stack_off = 0, mid_off = 0;  // start of the region
};
template <class Stage>
inline int64_t cr_multi_layout(const std::vector<Stage>& stages, const CrStagePlan& tail_plan, int m, int64_t cols,
                               std::vector<CrMultiStage>* st, CrMultiStage* tail) {
  int64_t o = 0;
  auto region = [&](int64_t stride, int64_t* off) {
    *off = o;
    o += cols * stride;
  };
  st->assign(stages.size(), CrMultiStage());
  for (size_t s = 0; s < stages.size(); ++s) {
    const CrStageBuffers b = cr_stage_buffers(stages[s], m);
    CrMultiStage& W = (*st)[s];
    W.part = 3 * b.part;
    W.stack = cr_even(b.stack);
    W.mid = cr_even(b.mid);
    region(W.part, &W.part_off);
    region(W.stack, &W.stack_off);
    region(W.mid, &W.mid_off);
  }
  *tail = CrMultiStage();
  tail->mid = cr_even(cr_stage_buffers(tail_plan, m).mid);
  region(tail->mid, &tail->mid_off);
  return o;
}

// ---- coarsest solve: a stage's dictionary of factor records (AGGMG_OPT_COARSE_DICTIONARY, cr_kernels.hpp) ------------
// A chunk stage whose levels hold few distinct factor records keeps them in LDS: per level one table of the even rows'
// records (the fe pair: 2 m^2 doubles) and one of the odd rows' (the fo pair, the lu block and perm: 2 m^2 + m^2 doubles
// and m 32-bit words, padded to 16 bytes), all of a stage in ONE table that a launch copies with 16-byte loads, and per
// level and parity the class index (uint16) of every row.  A launch's LDS then holds, behind the stage's vectors
// (lds_total doubles): the table, and the class indices of the workgroup's chunk -- 2^(q-l-1) + 1 even and 2^(q-l-1) odd
// rows of local level l.  Block sizes 1 and 2 (forms.hpp: cr_dict_form).
//
// kCrDictMaxClasses, the largest cap on classes per level and parity and the option's default: what the launch's LDS limit
// (kCrLdsBudgetBytes, the limit a stage's vectors are planned against) leaves at the largest plan, q = 12 levels of blocks
// of 2: 160 KiB - 28272 bytes of vectors - 16416 bytes of class indices = 119152 bytes for 12 levels of cap x (64 + 112)
// bytes -> cap 56.  The cap only bounds the worst case: a stage's table is as large as its levels' class counts make it,
// and the stage takes the form when that table fits (cr_dict_plan) -- all or nothing per stage.
constexpr int kCrDictMaxClasses = 56;
constexpr int cr_dict_even_words(int m) { return 2 * m * m; }                             // doubles per even record
constexpr int cr_dict_odd_words(int m) { return (3 * m * m + (m + 1) / 2 + 1) & ~1; }     // doubles per odd record
constexpr int cr_dict_index_count(int q) { return ((2 << q) - 2 + q + 7) & ~7; }          // uint16 per chunk, all levels
struct CrDictPlan {
  bool take = false;
  int tab_e[kCrMaxStageLevels] = {0}, tab_o[kCrMaxStageLevels] = {0};  // doubles from the table's start, per local level
  int tab_words = 0;                                                    // the table, doubles (even)
  int idx_e[kCrMaxStageLevels] = {0}, idx_o[kCrMaxStageLevels] = {0};  // uint16 from the index region's start
  int idx_count = 0;                                                    // uint16 (a multiple of 8)
  int tab_off = 0, idx_off = 0;                                         // doubles from the start of the launch's LDS
  size_t lds_bytes = 0;                                                 // vectors + table + class indices
};
// the layout of a stage of q levels whose local level l has n_even_cls[l] / n_odd_cls[l] classes; take = false (and the
// layout left undefined) for another block size, a level without classes or with more than `cap`, or a launch beyond
// lds_limit bytes
inline CrDictPlan cr_dict_plan(int m, int q, int lds_total, const int* n_even_cls, const int* n_odd_cls, int cap,
                               size_t lds_limit = kCrLdsBudgetBytes) {
  CrDictPlan P;
  if (!cr_dict_form(m) || q < 1 || q > kCrMaxStageLevels || cap < 1) return P;
  for (int l = 0; l < q; ++l)
    if (n_even_cls[l] < 1 || n_even_cls[l] > cap || n_odd_cls[l] < 1 || n_odd_cls[l] > cap) return P;
  int o = 0;
  for (int l = 0; l < q; ++l) {
    P.tab_e[l] = o;
    o += n_even_cls[l] * cr_dict_even_words(m);
    P.tab_o[l] = o;
    o += n_odd_cls[l] * cr_dict_odd_words(m);
  }
  P.tab_words = o;   // (both record lengths are even: every offset stands on 16 bytes)
  int i = 0;
  for (int l = 0; l < q; ++l) {
    P.idx_e[l] = i;
    i += (1 << (q - l - 1)) + 1;
    P.idx_o[l] = i;
    i += 1 << (q - l - 1);
  }
  P.idx_count = (i + 7) & ~7;
  P.tab_off = (lds_total + 1) & ~1;
  P.idx_off = P.tab_off + P.tab_words;
  P.lds_bytes = (size_t)P.idx_off * sizeof(double) + (size_t)P.idx_count * sizeof(uint16_t);
  P.take = P.lds_bytes <= lds_limit;
  return P;
}
// class c's odd record from the dictionary's arrays fo [nc][2 m^2], lu [nc][m^2], perm [nc][m]
inline void cr_dict_pack_odd(int m, int nc, const double* fo, const double* lu, const int32_t* perm, double* rec) {
  const int mm = m * m, w = cr_dict_odd_words(m);
  for (int c = 0; c < nc; ++c) {
    double* r = rec + (size_t)c * w;
    std::memset(r, 0, (size_t)w * sizeof(double));
    std::memcpy(r, fo + (size_t)c * 2 * mm, (size_t)2 * mm * sizeof(double));
    std::memcpy(r + 2 * mm, lu + (size_t)c * mm, (size_t)mm * sizeof(double));
    std::memcpy(r + 3 * mm, perm + (size_t)c * m, (size_t)m * sizeof(int32_t));
  }
}

// ---- generic CSR kernels: row blocks -------------------------------------------------------------------------------
// csr_stream_kernel: runs of consecutive rows holding at most max_nnz entries and at most max_rows rows; a row longer
// than max_nnz stands alone (the kernel reduces it across the workgroup).  -> block boundaries, blocks + 1 entries
inline std::vector<int32_t> stream_row_blocks(const int32_t* rowptr, int64_t nrows, int max_nnz, int max_rows) {
  std::vector<int32_t> blk;
  blk.push_back(0);
  int64_t r = 0;
  while (r < nrows) {
    int64_t e = r + 1;  // a block always takes at least one row
    const int64_t b0 = rowptr[r];
    while (e < nrows && e - r < max_rows && rowptr[e + 1] - b0 <= max_nnz) ++e;
    if (rowptr[r + 1] - b0 > max_nnz) e = r + 1;
    blk.push_back((int32_t)e);
    r = e;
  }
  return blk;
}

// csr_band_kernel (entries within bw of the diagonal, up to `sweeps` point-Jacobi sweeps per launch): a block's rows plus
// (sweeps - 1) * bw halo rows on either side hold at most max_nnz entries, and its window of x -- the rows plus
// sweeps * bw on either side -- fits `window` doubles.  -> false when some row is too long for its halo to fit
inline bool band_row_blocks(const int32_t* rowptr, int64_t nrows, int bw, int sweeps, int max_nnz, int window, int max_rows,
                            std::vector<int32_t>* out) {
  const int64_t H = (int64_t)(sweeps - 1) * bw;
  out->clear();
  out->push_back(0);
  int64_t r = 0;
  while (r < nrows) {
    const int64_t lo = std::max<int64_t>(0, r - H);
    auto fits = [&](int64_t e) {
      const int64_t hi = std::min(nrows, e + H);
      return rowptr[hi] - rowptr[lo] <= max_nnz && (e - r) + 2 * (int64_t)sweeps * bw <= window;
    };
    int64_t e = r + 1;
    if (!fits(e)) return false;
    while (e < nrows && e - r < max_rows && fits(e + 1)) ++e;
    out->push_back((int32_t)e);
    r = e;
  }
  return true;
}

// ---- fused level launches: which tiles a launch runs ------------------------------------------------------------
// A level of ne elements in tiles of `owned` elements.  mode 0: all tiles; 1: the tiles holding [0, head) and
// [tail, ne) (element-partitioned runs produce the interface elements first); 2: the ones in between.
// Workgroup b runs tile b + (b >= split ? skip : 0).
struct TileSubset {
  int64_t ntiles = 0;  // workgroups of the launch
  int split = 0;
  int64_t skip = 0;
};
inline TileSubset fused_tile_subset(int64_t ne, int owned, int mode, int64_t head_in, int64_t tail_in) {
  TileSubset t;
  t.ntiles = (ne + owned - 1) / owned;
  if (mode == 0) return t;
  const int64_t head = std::min(std::max<int64_t>(head_in, 0), ne);
  const int64_t tail = std::min(std::max(tail_in, head), ne);
  const int64_t all = t.ntiles;
  const int64_t tA = std::min(all, (head + owned - 1) / owned);   // tiles [0, tA) hold [0, head)
  const int64_t tB = std::min(all - tA, all - tail / owned);      // the last tB tiles hold [tail, ne)
  if (mode == 1) {
    t.split = (int)tA;
    t.skip = all - tA - tB;
    t.ntiles = tA + tB;
  } else {
    t.skip = tA;
    t.ntiles = all - tA - tB;
  }
  return t;
}

// ---- fused level launches: the tile itself ------------------------------------------------------------------------
// The tile constants (elements a workgroup holds) come in as arguments; every plan reports "no tile" as a zero size.

// Single-level launch: a tile of te elements keeps `halo` elements each side and owns the rest, rounded down to a
// multiple of `align` (the agglomeration ratio when the launch restricts to uniform agglomerates, 1 otherwise).
// var_agg: the launch restricts to agglomerates of different sizes (at most agg_shift + 1 elements; < 0: not known).
// Where the tile can afford it the owned ranges are moved onto agglomerate boundaries (agg_shift taken: plain
// stores); otherwise agglomerates cut by a tile boundary are summed from two tiles into a zeroed vector (-1).
struct FusedTilePlan {
  int owned = 0, halo_left = 0;
  int agg_shift = -1;
};
inline FusedTilePlan fused_tile_plan(int te, int halo, int align, bool var_agg, int agg_shift) {
  FusedTilePlan p;
  const bool aligned = var_agg && agg_shift >= 0 && te - 2 * halo - agg_shift >= te / 2;
  const int shift = aligned ? agg_shift : 0;
  if (aligned) p.agg_shift = agg_shift;
  p.owned = std::max(0, ((te - 2 * halo - shift) / align) * align);
  p.halo_left = halo + shift;
  return p;
}

// K-column launch (multi_kernels.hpp): the same without agglomerates of different sizes
inline int multi_tile_owned(int te, int halo, int align) { return std::max(0, ((te - 2 * halo) / align) * align); }

// Two levels A (fine, ratio rho_ab to B) and B (ratio rho_bc to C) in one launch (pair_kernels.hpp); tea / teb: the
// elements of A / B a workgroup can hold.  own == 0: no tile for these ratios and sweeps.
struct PairTilePlan {
  int own = 0;           // descent: owned elements of B, a multiple of rho_bc; ascent: of A, a multiple of rho_ab
  int te_a = 0, te_b = 0;
  int hb = 0;            // ascent: halo of B behind A's nPost elements
  int64_t all = 0, tA = 0, tB = 0;   // split ascent: tiles of the level, of them the prefix / suffix touching ghosts
};
inline PairTilePlan pair_down_plan(int nPre, int rho_ab, int rho_bc, int tea, int teb) {
  PairTilePlan p;
  const int hh = nPre + 1;
  const int te_b = std::min(teb, (tea - 2 * hh) / rho_ab);
  const int own = ((te_b - 2 * hh) / rho_bc) * rho_bc;
  if (own <= 0) return p;
  p.own = own;
  p.te_b = own + 2 * hh;
  p.te_a = p.te_b * rho_ab + 2 * hh;
  return p;
}
inline PairTilePlan pair_up_plan(int nPost, int rho_ab, int tea, int teb) {
  PairTilePlan p;
  const int hb = (nPost + rho_ab - 1) / rho_ab;
  const int own = (std::min(tea - 2 * nPost, (teb - 2 * hb - 2 * nPost) * rho_ab) / rho_ab) * rho_ab;
  if (own <= 0) return p;
  p.hb = hb;
  p.own = own;
  p.te_a = own + 2 * nPost;
  p.te_b = own / rho_ab + 2 * hb + 2 * nPost;
  return p;
}
// The ascent in two parts (element-partitioned runs, C = the coarsest level of nec elements, A has ne): tile t
// prolongs from the elements floor(Eb0 / rho_bc) .. floor((Eb0 + te_b - 1) / rho_bc) of C (clipped to the level).
// Tiles are ordered, so the ones reading the first gh_lo / last gh_hi elements of C are a prefix and a suffix.
inline void pair_up_split(PairTilePlan* p, int nPost, int rho_ab, int rho_bc, int64_t ne, int64_t nec, int64_t gh_lo,
                          int64_t gh_hi) {
  const int64_t ne_b = ne / rho_ab;
  auto eb0 = [&](int64_t t) { return (t * p->own) / rho_ab - p->hb - nPost; };
  auto jmin = [&](int64_t t) { return std::max<int64_t>(eb0(t), 0) / rho_bc; };
  auto jmax = [&](int64_t t) { return std::min<int64_t>(eb0(t) + p->te_b - 1, ne_b - 1) / rho_bc; };
  p->all = (ne + p->own - 1) / p->own;
  p->tA = p->tB = 0;
  while (p->tA < p->all && jmin(p->tA) < gh_lo) ++p->tA;
  while (p->tB < p->all - p->tA && jmax(p->all - 1 - p->tB) >= nec - gh_hi) ++p->tB;
}

// The chain kernel (cgt.hip): a tile of te blocks keeps hl / hr blocks of halo and owns the rest, rounded down to a
// multiple of `align` (the ratio of an agglomerating restriction, 1 otherwise)
inline int chain_tile_owned(int te, int hl, int hr, int align) { return std::max(0, ((te - hl - hr) / align) * align); }

// ---- element-patch Schwarz sweeps (patch_kernels.hpp) ---------------------------------------------------------------
// A workgroup of `threads` threads holds ns slabs of threads / m elements.  A sweep reaches two elements to each side,
// so a launch of S sweeps keeps 2 S elements of halo on either side of the owned ones.  The most sweeps a launch
// takes: as many as its weights array holds and the halos leave half the tile to own (at least one sweep where one
// sweep leaves a tile at all; 0: no tile).  LDS: two iterate buffers and the residual, each padded by one element a side.
constexpr int kPatchMaxSweeps = 8;   // == kSweepWeights (kernels.hpp; asserted where both are seen)
struct PatchTilePlan {
  int te = 0;      // elements a workgroup holds
  int halo = 0;    // per side
  int owned = 0;   // 0: no tile
  size_t lds_bytes = 0;
};
constexpr int patch_slabs(int m) { return m <= 3 ? 4 : (m == 4 ? 3 : (m <= 6 ? 2 : 1)); }   // PatchSlabs<M>::NS
inline int patch_tile_elems(int m, int threads = 256) { return m >= 1 && m <= threads ? (threads / m) * patch_slabs(m) : 0; }
inline int patch_owned(int te, int sweeps) { return std::max(0, te - 4 * sweeps); }
inline PatchTilePlan patch_tile_plan(int m, int sweeps, int threads = 256) {
  PatchTilePlan p;
  p.te = patch_tile_elems(m, threads);
  if (p.te <= 0 || sweeps < 1 || sweeps > kPatchMaxSweeps) return p;
  p.halo = 2 * sweeps;
  p.owned = patch_owned(p.te, sweeps);
  p.lds_bytes = (size_t)3 * (p.te + 2) * m * sizeof(double);
  return p;
}
inline int patch_max_sweeps(int m, int threads = 256) {
  const int te = patch_tile_elems(m, threads);
  if (patch_tile_plan(m, 1, threads).owned <= 0) return 0;
  return std::max(1, std::min(kPatchMaxSweeps, te / 8));
}
inline int64_t patch_tiles(int64_t ne, int owned) { return owned > 0 ? (ne + owned - 1) / owned : 0; }
// a run of `sweeps` sweeps in launches of at most smax: launch c of patch_chunks takes patch_chunk_sweeps
inline int patch_chunks(int sweeps, int smax) { return sweeps <= 0 || smax <= 0 ? 0 : (sweeps + smax - 1) / smax; }
inline int patch_chunk_sweeps(int sweeps, int smax, int c) { return std::min(smax, sweeps - c * smax); }

// ---- multiplicative two-colour patch sweeps (patch_gs_kernel) ---------------------------------------------------------
// The same tile of elements.  A sweep is two half-sweeps, each a residual and the patch solves of one colour: together
// they reach 3 elements to one side and 2 to the other (which side depends on the element's parity and the direction),
// and the wide sides of consecutive sweeps alternate: S sweeps reach 2 S + 1 elements, the halo of a launch.  The most
// sweeps a launch takes: as many as its weights array holds and the halos leave half the tile to own (at least one
// where one sweep leaves a tile at all; 0: no tile).  LDS: the iterate, updated in place, and the residual, each
// padded by one element a side.  A longer run is chunked as the hybrid sweeps are: patch_chunks / patch_chunk_sweeps
// with patch_gs_max_sweeps.
inline int patch_gs_halo(int sweeps) { return 2 * sweeps + 1; }
inline int patch_gs_owned(int te, int sweeps) { return std::max(0, te - 2 * patch_gs_halo(sweeps)); }
inline PatchTilePlan patch_gs_tile_plan(int m, int sweeps, int threads = 256) {
  PatchTilePlan p;
  p.te = patch_tile_elems(m, threads);
  if (p.te <= 0 || sweeps < 1 || sweeps > kPatchMaxSweeps) return p;
  p.halo = patch_gs_halo(sweeps);
  p.owned = patch_gs_owned(p.te, sweeps);
  p.lds_bytes = (size_t)2 * (p.te + 2) * m * sizeof(double);
  return p;
}
inline int patch_gs_max_sweeps(int m, int threads = 256) {
  const int te = patch_tile_elems(m, threads);
  if (patch_gs_tile_plan(m, 1, threads).owned <= 0) return 0;
  int s = 1;
  while (s < kPatchMaxSweeps && 2 * patch_gs_owned(te, s + 1) >= te) ++s;
  return s;
}

// ---- the same sweeps on K columns at once (patch_gs_multi_kernel, patch_multi_kernels.hpp) -----------------------------
// One slab: a workgroup of `threads` threads holds threads / m elements, for the block sizes the K-column transfer kernel
// covers (multi_block_size, forms.hpp), and a column group kb of them.  Reach, halo and the most sweeps per launch follow the
// single-column rules above (neither depends on kb).  LDS: per column an iterate plane, updated in place, and a residual
// plane, each padded by one element a side -- 2 kb (te + 2) m doubles, 33 KiB at kb = 8: four workgroups per compute unit.
inline int patch_gs_multi_tile_elems(int m, int threads = 256) { return multi_block_size(m) ? threads / m : 0; }
inline PatchTilePlan patch_gs_multi_tile_plan(int m, int sweeps, int kb, int threads = 256) {
  PatchTilePlan p;
  p.te = patch_gs_multi_tile_elems(m, threads);
  if (p.te <= 0 || !is_col_group(kb) || sweeps < 1 || sweeps > kPatchMaxSweeps) return p;
  p.halo = patch_gs_halo(sweeps);
  p.owned = patch_gs_owned(p.te, sweeps);
  p.lds_bytes = (size_t)2 * kb * (p.te + 2) * m * sizeof(double);
  return p;
}
inline int patch_gs_multi_max_sweeps(int m, int threads = 256) {
  const int te = patch_gs_multi_tile_elems(m, threads);
  if (patch_gs_multi_tile_plan(m, 1, 1, threads).owned <= 0) return 0;
  int s = 1;
  while (s < kPatchMaxSweeps && 2 * patch_gs_owned(te, s + 1) >= te) ++s;
  return s;
}

// ---- the hybrid / additive sweeps on K columns at once (patch_sweep_multi_kernel, patch_schwarz_multi_kernels.hpp) --------
// The same slab and column groups.  Reach, halo (2 S a side) and the most sweeps per launch follow the single-column rules
// of patch_tile_plan / patch_max_sweeps on that one slab (neither depends on kb).  LDS: per column an iterate plane, updated
// in place, and a residual plane, each padded by one element a side -- 2 kb (te + 2) m doubles, as above.
// Columns one launch takes of a group of up to 8: a group of more runs as launches of this many.  4: a group of eight is two
// launches of KB = 4 -- the KB = 8 kernel needs 156 - 158 registers where KB = 4 needs 92, three waves per SIMD in place of
// five, and came out 3 - 7 % slower per V(3,3) cycle at 2^20 and 2^22 elements (profiles/r34_patch_schwarz_multi.md).  The
// choice changes no bit.
constexpr int kPatchSchwarzMultiCols = 4;
inline int patch_schwarz_multi_tile_elems(int m, int threads = 256) { return multi_block_size(m) ? threads / m : 0; }
inline PatchTilePlan patch_schwarz_multi_tile_plan(int m, int sweeps, int kb, int threads = 256) {
  PatchTilePlan p;
  p.te = patch_schwarz_multi_tile_elems(m, threads);
  if (p.te <= 0 || !is_col_group(kb) || sweeps < 1 || sweeps > kPatchMaxSweeps) return p;
  p.halo = 2 * sweeps;
  p.owned = patch_owned(p.te, sweeps);
  p.lds_bytes = (size_t)2 * kb * (p.te + 2) * m * sizeof(double);
  return p;
}
inline int patch_schwarz_multi_max_sweeps(int m, int threads = 256) {
  const int te = patch_schwarz_multi_tile_elems(m, threads);
  if (patch_schwarz_multi_tile_plan(m, 1, 1, threads).owned <= 0) return 0;
  return std::max(1, std::min(kPatchMaxSweeps, te / 8));
}

// ---- the chain kernel on K columns at once (cgt_multi_kernel, cgt_multi_kernels.hpp) -------------------------------------
// One slab: a workgroup of `threads` threads holds threads / m blocks, for the sizes of chain_dict_form (forms.hpp; lane groups
// of m) and a column group kb of them.  The halos are the single-column launch's (cgt_launch_tt): a block per sweep and side, one more a
// side for a residual, one more on the left for a chain restriction, on the right for an agglomerating one, whose ratio the
// owned blocks are a multiple of.  The most sweeps per launch follow the single-column rule.  LDS: kb iterate planes per
// ping-pong buffer, each padded by one block a side, and (dictionary variant) the tile's classes behind them.
enum ChainRestrict { kChainNoRestrict = 0, kChainToChain = 1, kChainToAgg = 2 };
struct ChainMultiPlan {
  int te = 0;                        // blocks a workgroup holds (0: block size not covered)
  int halo_left = 0, halo_right = 0;
  int owned = 0;                     // 0: no tile
  size_t lds_bytes = 0;
};
inline int chain_multi_tile_blocks(int m, int threads = 256) { return chain_dict_form(m) ? threads / m : 0; }
inline ChainMultiPlan chain_multi_tile_plan(int m, int nsweeps, int restrict_kind, int rho, int kb, bool dict = false,
                                            int threads = 256) {
  ChainMultiPlan p;
  p.te = chain_multi_tile_blocks(m, threads);
  if (p.te <= 0 || !is_col_group(kb) || nsweeps < 0 || nsweeps > kPatchMaxSweeps || rho < 1) return p;
  if (restrict_kind < kChainNoRestrict || restrict_kind > kChainToAgg) return p;
  p.halo_left = nsweeps + (restrict_kind != kChainNoRestrict ? 1 : 0) + (restrict_kind == kChainToChain ? 1 : 0);
  p.halo_right = nsweeps + (restrict_kind != kChainNoRestrict ? 1 : 0) + (restrict_kind == kChainToAgg ? 1 : 0);
  p.owned = chain_tile_owned(p.te, p.halo_left, p.halo_right, restrict_kind == kChainToAgg ? rho : 1);
  p.lds_bytes = (size_t)2 * kb * (p.te + 2) * m * sizeof(double) + (dict ? (size_t)(p.te + 2) * 2 : 0);
  return p;
}
// (cgt_max_sweeps of cgt.hip on the one-slab tile: 2 * smax + 3 blocks of halo always fit it)
inline int chain_multi_max_sweeps(int m, int threads = 256) {
  const int te = chain_multi_tile_blocks(m, threads);
  return te <= 0 ? 0 : std::max(1, std::min(kPatchMaxSweeps, te / 8));
}

// ---- does a launch have a tile? ----------------------------------------------------------------------------------
// One question for every tiled launch, answered by the planner its launcher runs: the callers that choose between a
// launch and its fallback (two levels or one per launch, fused or unfused sequence, K columns or column by column) ask
// here, so a launch that was chosen never finds "no tile".
enum TileLaunch { kTileFused = 0, kTileMulti = 1, kTilePairDown = 2, kTilePairUp = 3, kTilePatch = 4, kTilePatchGs = 5, kTilePatchGsMulti = 6, kTileChainMulti = 7, kTilePatchSchwarzMulti = 8 };
struct TileQuery {
  int launch = kTileFused;
  int te = 0, te_b = 0;   // elements a workgroup holds (pairs: of level A and of level B)
  int halo = 0;           // fused / K-column: elements kept each side; pairs, patch sweeps: the sweeps
  int align = 1;          // fused / K-column: see fused_tile_plan; pairs: rho_ab
  int rho_bc = 1;         // descent of a pair
  bool var_agg = false;   // fused: see fused_tile_plan
  int agg_shift = -1;
  int restrict_kind = 0;  // K-column chain launch: ChainRestrict (there te = the block size m, halo = the sweeps, align = rho)
  int kb = 1;             // K-column chain launch: the column group
};
inline bool launch_has_tile(const TileQuery& q) {
  if (q.te <= 0 || q.align < 1 || q.rho_bc < 1 || q.halo < 0) return false;
  switch (q.launch) {
    case kTileFused: return fused_tile_plan(q.te, q.halo, q.align, q.var_agg, q.agg_shift).owned > 0;
    case kTileMulti: return multi_tile_owned(q.te, q.halo, q.align) > 0;
    case kTilePairDown: return pair_down_plan(q.halo, q.align, q.rho_bc, q.te, q.te_b).own > 0;
    case kTilePairUp: return pair_up_plan(q.halo, q.align, q.te, q.te_b).own > 0;
    case kTilePatch: return q.halo >= 1 && q.halo <= kPatchMaxSweeps && patch_owned(q.te, q.halo) > 0;
    case kTilePatchGs: return q.halo >= 1 && q.halo <= kPatchMaxSweeps && patch_gs_owned(q.te, q.halo) > 0;
    case kTilePatchGsMulti: return q.halo >= 1 && q.halo <= kPatchMaxSweeps && patch_gs_owned(q.te, q.halo) > 0;   // te: patch_gs_multi_tile_elems
    case kTileChainMulti: return chain_multi_tile_plan(q.te, q.halo, q.restrict_kind, q.align, q.kb).owned > 0;   // te: the block size
    case kTilePatchSchwarzMulti: return q.halo >= 1 && q.halo <= kPatchMaxSweeps && patch_owned(q.te, q.halo) > 0;   // te: patch_schwarz_multi_tile_elems
  }
  return false;
}

// ---- checkpoint launches: room for their partial sums ---------------------------------------------------------------
// A checkpoint launch stores two doubles per tile and checkpoint; the buffer is sized before the launches are known one
// by one.  What is known: the level (ne elements in tiles of te), the largest halo any of them takes, and the restriction
// of the one between two cycles (align / var_agg / agg_shift as fused_tile_plan; the others restrict nothing: align 1).
// -> the largest tile count of any such launch with a halo of 1 .. halo_max (the owned size is not monotone in the halo
// where agglomerates of different sizes move the tiles), at least 1.  The launchers refuse a launch with more tiles.
inline int64_t fused_chk_reserve(int64_t ne, int te, int halo_max, int align, bool var_agg, int agg_shift) {
  int64_t most = 1;
  for (int halo = 1; halo <= halo_max; ++halo)
    for (int restricting = 0; restricting < 2; ++restricting) {
      const int owned = restricting ? fused_tile_plan(te, halo, align, var_agg, agg_shift).owned
                                    : fused_tile_plan(te, halo, 1, false, -1).owned;
      if (owned > 0) most = std::max(most, fused_tile_subset(ne, owned, 0, 0, 0).ntiles);
    }
  return most;
}
// the chain kernel's: hsum_max = the largest hl + hr of its checkpoint launches
inline int64_t chain_chk_reserve(int64_t ne, int te, int hsum_max, int align) {
  int64_t most = 1;
  for (int hs = 2; hs <= hsum_max; ++hs)
    for (int a : {align, 1}) {
      const int owned = chain_tile_owned(te, hs - hs / 2, hs / 2, a);
      if (owned > 0) most = std::max(most, (ne + owned - 1) / owned);
    }
  return most;
}

// ---- host-pointer entry (aggmg_vcycle): lane t's byte range of a copy split over `lanes` worker threads ----------
inline void stage_lane_range(size_t bytes, int lanes, int t, size_t* lo, size_t* hi) {
  const size_t per = ((bytes / (size_t)lanes) + 4095) & ~(size_t)4095;
  *lo = std::min(bytes, (size_t)t * per);
  *hi = t == lanes - 1 ? bytes : std::min(bytes, (size_t)(t + 1) * per);
}

// ---- element-partitioned coarsest solve: chunked or gathered? ---------------------------------------------------
// Decided from GLOBAL quantities only (every rank must take the same route: mismatched collective counts hang):
// the replicated operator's plan (q = log2 chunk, or <= 0: none; its block size and block count must be the
// level's) and an even division of the level into whole chunks per rank.
//  -> 0 gather-and-replicate, 1 chunked, -1 chunked applies but THIS rank's range breaks the pattern (refuse)
inline int dist_chunk_route(int q, int plan_m, int64_t plan_blocks, int m, int64_t ne, int world, int rank, int64_t own_lo,
                            int64_t own_hi) {
  if (!(q > 0 && plan_m == m && plan_blocks == ne) || world < 1 || ne % world != 0) return 0;
  const int64_t per_rank = ne / world, chunk = (int64_t)1 << q;
  if (per_rank % chunk != 0 || per_rank < chunk) return 0;
  if (own_hi - own_lo != per_rank || own_lo != (int64_t)rank * per_rank) return -1;
  return 1;
}

// ---- element-partitioned cycle: are the ghost layers wide enough? -------------------------------------------------
// The margin recurrences of distributed.halo_widths over given widths W[0 .. nl) (elements per side; nl - 1 smoothed
// levels, ratio[k] elements of level k per element of level k + 1).  Elements per side by which S sweeps shrink the
// valid part of a local domain: block Jacobi S; red-black block Gauss-Seidel and the hybrid element patches 2 S; each
// of the three one less from a zero iterate, whose first residual reads no neighbour; the multiplicative patches
// 2 S + 1 (patch_gs_halo; no saving claimed from a zero start).  No sweep, no reach.
enum DistSmoother { kDistBlockJac = 0, kDistBlockGs = 1, kDistPatchSchwarz = 2, kDistPatchGs = 3 };
inline int dist_sweep_reach(int kind, int sweeps, bool zero_start) {
  if (sweeps <= 0) return 0;
  switch (kind) {
    case kDistBlockJac: return zero_start ? sweeps - 1 : sweeps;
    case kDistBlockGs:
    case kDistPatchSchwarz: return zero_start ? 2 * sweeps - 1 : 2 * sweeps;
    default: return patch_gs_halo(sweeps);
  }
}
// Descending: the margin of the pre-smoothed iterate (elements beyond the owned boundary that hold the single-domain
// values) must leave one valid neighbour for the residual; the restricted right-hand side keeps (margin - 1) / ratio.
// Ascending: the coarsest solution is exact on all its ghosts; a prolonged level is valid where both the coarse values
// and its own pre-smoothed iterate are, less the reach of the post sweeps -- which must not eat into the owned elements.
inline bool dist_halo_ok(int nl, const int64_t* W, const int* ratio, const int* kind, int nPre, int nPost) {
  if (nl < 2 || nl > 64) return false;
  int64_t pu[64];
  int64_t rm = W[0];   // the fine right-hand side is valid on the whole local domain
  for (int k = 0; k < nl - 1; ++k) {
    if (ratio[k] < 1) return false;
    pu[k] = std::min(rm, W[k]) - dist_sweep_reach(kind[k], nPre, k > 0);   // (levels below the finest start from zero)
    if (pu[k] < 1) return false;
    rm = (pu[k] - 1) / ratio[k];
  }
  int64_t v = W[nl - 1];
  for (int k = nl - 2; k >= 0; --k) {
    v = std::min(pu[k], ratio[k] * v) - dist_sweep_reach(kind[k], nPost, false);
    if (v < 0) return false;
  }
  return true;
}

// ---- the class records of the element-thread kernels (elem_kernels.hpp, AGGMG_OPT_ELEMENT_RECORDS_LDS) ---------------
// One record per class of a level with blocks of 4 rows, 16-byte groups: every operator word the kernels read for an
// element, repacked on the host from the dictionary's arrays (DictDev) --
//   [0]  the packed inverse (bsym), 10 words                 [10] pcol = B^{-1} q_{e-1}
//   [14] q_e (qrow)            [18] q_{e-1} (qmir)           [22] the upper triangle of D_e (dup), 10 words
//   [32] the four corr words   [34] lx0 ly0 .. lx3 ly3       (rows of L; a unit first column is stored as the 1.0 it
//                                                            stands for)
constexpr int kElemRecWords = 42;
constexpr int kElemRecBsym = 0, kElemRecPcol = 10, kElemRecQrow = 14, kElemRecQmir = 18, kElemRecDup = 22, kElemRecCorr = 32,
              kElemRecLf = 34;
static_assert(kElemRecWords % 2 == 0 && kElemRecPcol % 2 == 0 && kElemRecQrow % 2 == 0 && kElemRecQmir % 2 == 0 &&
                  kElemRecDup % 2 == 0 && kElemRecCorr % 2 == 0 && kElemRecLf % 2 == 0,
              "the groups of a record are read 16 bytes at a time");
// Most classes of a level these kernels take (a level with more keeps the kernels above).  A launch's LDS follows the
// level's class count: elem_lds_bytes<4>() = 16512 bytes of iterate buffers and 336 per class.  The registers allow 6
// workgroups per CU where they are fewest (80 VGPRs in the launch that forms the residual: 6 waves per SIMD; 87 in the
// replaying ascent: 5), and 6 workgroups share 163840 bytes of LDS: 27306 each, so (27306 - 16512) / 336 = 32 classes is
// the largest table that costs no workgroup -- 6 x (16512 + 32 x 336) = 163584 (profiles/r32_elem_records_lds.md).
#ifndef AGGMG_ELEM_REC_MAX_CLASSES
#define AGGMG_ELEM_REC_MAX_CLASSES 32
#endif
constexpr int kElemRecMaxClasses = AGGMG_ELEM_REC_MAX_CLASSES;
// rec [nclasses][kElemRecWords] from bsym [nclasses][10], qrow / qmir [nclasses][4], dup [nclasses][10] and corr
// [nclasses][4] (both null on a level without the symmetric residual form: zeros), lf [nclasses][4] (lf_unit: the second
// entries of the rows of L) or [nclasses][4][2] (the rows).  pcol is the kernels' chain (elem_sym_row_apply): row i of
// the symmetric inverse times q_{e-1}, fma(tri[.], qm[j], acc) with j ascending from 0.0 -- std::fma rounds once, as
// the device's fma does, so the words are the ones the kernels formed per element.
inline void elem_record_pack(int nclasses, const double* bsym, const double* qrow, const double* qmir, const double* dup,
                             const uint32_t* corr, const double* lf, bool lf_unit, double* rec) {
  constexpr int M = 4, T = 10;
  auto tri = [](int i, int j) { return i * M - (i * (i - 1)) / 2 + (j - i); };   // (i <= j) as elem_tri<4>
  for (int c = 0; c < nclasses; ++c) {
    double* r = rec + (size_t)c * kElemRecWords;
    for (int k = 0; k < kElemRecWords; ++k) r[k] = 0.0;
    for (int k = 0; k < T; ++k) r[kElemRecBsym + k] = bsym[c * T + k];
    for (int i = 0; i < M; ++i) {
      double acc = 0.0;
      for (int j = 0; j < M; ++j) acc = std::fma(bsym[c * T + (i < j ? tri(i, j) : tri(j, i))], qmir[c * M + j], acc);
      r[kElemRecPcol + i] = acc;
      r[kElemRecQrow + i] = qrow[c * M + i];
      r[kElemRecQmir + i] = qmir[c * M + i];
      r[kElemRecLf + 2 * i] = lf_unit ? 1.0 : lf[(c * M + i) * 2];
      r[kElemRecLf + 2 * i + 1] = lf_unit ? lf[c * M + i] : lf[(c * M + i) * 2 + 1];
    }
    if (dup && corr) {
      for (int k = 0; k < T; ++k) r[kElemRecDup + k] = dup[c * T + k];
      std::memcpy(r + kElemRecCorr, corr + c * M, M * sizeof(uint32_t));
    }
  }
}

}  // namespace aggmg
