// Element-thread form of the two-level dictionary launches (AGGMG_OPT_PAIR_ELEMENT_THREADS): one THREAD owns an element
// -- both of its rows, its b, u and g and the rows of P = B^{-1} Sub and Q = B^{-1} Sup -- where btd_pair_*_dict_kernel
// gives every row a thread.  In level a's phase a thread owns a level-a element, in level b's a level-b one; the
// element's index, clamp, class and validity are computed once and in 32 bits, and the 2 x 2 products are register FMAs
// instead of DPP broadcasts.  The class records of BOTH levels are copied into LDS at entry (PairElemDict::rec_*, the
// repacked records of setup_pair_dictionary, coalesced, all loads in flight together); a thread reads its words by
// class where it uses them -- the inverse and the sup rows before the sweeps, the residual's rows at the residual, the
// rows of L at the restriction / prolongation -- and holds none of them across phases (profiles/r27_pair_element_threads.md).
//
// Same tiles (pair_down_plan / pair_up_plan at kPairElemTEA / kPairElemTEB elements), same LDS iterate layout and the
// SAME BITS: every expression is the one btd_pair_*_dict_kernel<2, 2, 1, 256> is compiled to, pinned with __fma_rn /
// __dmul_rn / __dadd_rn so that no contraction depends on the code around it.
#pragma once
#include "elem_kernels.hpp"
#include "pair_kernels.hpp"

namespace aggmg {

// One class record, repacked at set-up (setup.hip, setup_pair_dictionary): the words pair_load_record / pair_load_residual_rows
// read for the two rows of an element, 16-byte groups --
//   [0] b00 b01   [2] b11 0     (packed symmetric inverse)
//   [4] rows 0, 1 of Sup_{e-1} (sback)   [8] of Sup_e   [12] of Sub_e   [16] of D_e
//   [20] lx0 ly0 lx1 ly1        (rows of L; a unit first column is stored as the 1.0 it stands for)
constexpr int kPairRecWords = 24;
constexpr int kPairRecBsym = 0, kPairRecSback = 4, kPairRecSup = 8, kPairRecSub = 12, kPairRecDblk = 16, kPairRecLf = 20;
// Most classes of a level the element-thread launches take (a level with more keeps the row-thread kernels).  The LDS of
// a launch follows the levels' class counts: 10304 bytes of buffers and 192 per class, so up to 53 classes on the two
// levels together leave the 8 workgroups per CU the registers allow (54 / 58 VGPRs) and two levels at the cap leave 7
// (profiles/r27_pair_element_threads.md)
#ifndef AGGMG_PAIR_ELEM_MAX_CLASSES
#define AGGMG_PAIR_ELEM_MAX_CLASSES 32
#endif
constexpr int kPairElemMaxClasses = AGGMG_PAIR_ELEM_MAX_CLASSES;
#ifndef AGGMG_PAIR_ELEM_NT
#define AGGMG_PAIR_ELEM_NT 256   // threads of a workgroup = level-a elements of a tile (measured: r27)
#endif
constexpr int kPairElemThreads = AGGMG_PAIR_ELEM_NT;
constexpr int kPairElemTEA = kPairElemThreads, kPairElemTEB = kPairElemThreads / 2;   // what the planners are given

struct PairElemDict {
  const uint16_t *cls_a, *cls_b;
  const double *rec_a, *rec_b;   // [nclasses][kPairRecWords]
  int nca, ncb;
};

// LDS of a launch: [ two level-a iterate buffers of (TEA + 2) elements, a zero element at either end | level-b vector
// of TEB elements | the two class tables ]; the level-b iterate buffers reuse the front region (pair_kernels.hpp)
constexpr size_t pair_elem_lds_bytes(int nca, int ncb) {
  return ((size_t)2 * (kPairElemTEA + 2) * 2 + (size_t)kPairElemTEB * 2 + (size_t)(nca + ncb) * kPairRecWords) * sizeof(double);
}

// both tables into LDS, 16 bytes per load, every load issued before the first store (a lane past a table reads its
// last word and stores nothing)
template <int NT>
__device__ __forceinline__ void pair_elem_stage(double* tabA, double* tabB, const PairElemDict& d, int x) {
  constexpr int K = (kPairElemMaxClasses * (kPairRecWords / 2) + NT - 1) / NT;
  const int na = d.nca * (kPairRecWords / 2), nb = d.ncb * (kPairRecWords / 2);
  elem_v2d va[K], vb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int t = x + k * NT;
    va[k] = reinterpret_cast<const elem_v2d*>(d.rec_a)[t < na ? t : na - 1];
    vb[k] = reinterpret_cast<const elem_v2d*>(d.rec_b)[t < nb ? t : nb - 1];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int t = x + k * NT;
    if (t < na) reinterpret_cast<elem_v2d*>(tabA)[t] = va[k];
    if (t < nb) reinterpret_cast<elem_v2d*>(tabB)[t] = vb[k];
  }
}

__device__ __forceinline__ void pair_elem_st2(double* p, double x, double y) {
  elem_v2d v;
  v.x = x;
  v.y = y;
#if AGGMG_NT & 2
  __builtin_nontemporal_store(v, reinterpret_cast<elem_v2d*>(p));
#else
  *reinterpret_cast<elem_v2d*>(p) = v;
#endif
}

// the element's g = B^{-1} b and its rows of P = B^{-1} Sub, Q = B^{-1} Sup from the class record in LDS:
// pair_rows_apply's chains, 0.0 first, k ascending
//   P[i][j] = sum_k Binv[i][k] Sup_{e-1}[j][k]      Q[i][j] = sum_k Binv[i][k] Sup_e[k][j]
__device__ __forceinline__ void pair_elem_rows(const double* rec, const double (&bb)[2], double (&g)[2], double (&P)[2][2],
                                               double (&Q)[2][2]) {
  double t0, t1, t2, pad, sm[2][2], sp[2][2];
  elem_ld2(rec + kPairRecBsym, t0, t1);
  elem_ld2(rec + kPairRecBsym + 2, t2, pad);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    elem_ld2(rec + kPairRecSback + 2 * i, sm[i][0], sm[i][1]);
    elem_ld2(rec + kPairRecSup + 2 * i, sp[i][0], sp[i][1]);
  }
  const double bi[2][2] = {{t0, t1}, {t1, t2}};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    g[i] = __fma_rn(bi[i][1], bb[1], __fma_rn(bi[i][0], bb[0], 0.0));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      P[i][j] = __fma_rn(bi[i][1], sm[j][1], __fma_rn(bi[i][0], sm[j][0], 0.0));
      Q[i][j] = __fma_rn(bi[i][1], sp[1][j], __fma_rn(bi[i][0], sp[0][j], 0.0));
    }
  }
}

// nsweeps block-Jacobi sweeps of a tile in LDS (pair_sweeps: ping-pong, one barrier per sweep), element x of the
// buffers, its two rows in uu; act: the thread has an element of the buffers at all (level b: x < TEB)
__device__ __forceinline__ void pair_elem_sweeps(int nsweeps, const SweepWeights& alpha, int x, bool act, bool valid,
                                                 const double (&g)[2], const double (&P)[2][2], const double (&Q)[2][2],
                                                 double (&uu)[2], double*& cur, double*& nxt) {
  for (int sw = 0; sw < nsweeps; ++sw) {
    if (act) {
      double um[2], up[2];
      elem_ld2(cur + (x - 1) * 2, um[0], um[1]);
      elem_ld2(cur + (x + 1) * 2, up[0], up[1]);
      const double w = alpha.w[(unsigned)sw];
      double un[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        double acc = __fma_rn(-P[i][0], um[0], g[i]);
        acc = __fma_rn(-P[i][1], um[1], acc);
        acc = __fma_rn(-Q[i][0], up[0], acc);
        acc = __fma_rn(-Q[i][1], up[1], acc);
        un[i] = __fma_rn(w, __dadd_rn(acc, -uu[i]), uu[i]);
        if (!valid) un[i] = 0.0;
        uu[i] = un[i];
      }
      elem_v2d v;
      v.x = un[0];
      v.y = un[1];
      *reinterpret_cast<elem_v2d*>(nxt + x * 2) = v;
    }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
}

// explicit residual r = b - A u of the element's two rows from the record's rows of Sub, D, Sup, ascending column order
// (pair_residual_row's chain, 0.0 first); ux: the element's own iterate
__device__ __forceinline__ void pair_elem_residual(const double* rec, const double* cur, int x, const double (&bb)[2],
                                                   const double (&ux)[2], double (&rr)[2]) {
  double um[2], up[2];
  elem_ld2(cur + (x - 1) * 2, um[0], um[1]);
  elem_ld2(cur + (x + 1) * 2, up[0], up[1]);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    double sb[2], db[2], sp[2];
    elem_ld2(rec + kPairRecSub + 2 * i, sb[0], sb[1]);
    elem_ld2(rec + kPairRecDblk + 2 * i, db[0], db[1]);
    elem_ld2(rec + kPairRecSup + 2 * i, sp[0], sp[1]);
    double t = __fma_rn(sb[0], um[0], 0.0);
    t = __fma_rn(sb[1], um[1], t);
    t = __fma_rn(db[0], ux[0], t);
    t = __fma_rn(db[1], ux[1], t);
    t = __fma_rn(sp[0], up[0], t);
    t = __fma_rn(sp[1], up[1], t);
    rr[i] = __dadd_rn(bb[i], -t);
  }
}

// the element's products lx * r and ly * r into the two (free) iterate buffers, zeros where the element restricts nothing
__device__ __forceinline__ void pair_elem_products(const double* rec, bool in, int x, const double (&rr)[2], double* bx, double* by) {
  double lx[2], ly[2];
  elem_ld2(rec + kPairRecLf, lx[0], ly[0]);
  elem_ld2(rec + kPairRecLf + 2, lx[1], ly[1]);
  elem_v2d vx, vy;
  vx.x = in ? __dmul_rn(lx[0], rr[0]) : 0.0;
  vx.y = in ? __dmul_rn(lx[1], rr[1]) : 0.0;
  vy.x = in ? __dmul_rn(ly[0], rr[0]) : 0.0;
  vy.y = in ? __dmul_rn(ly[1], rr[1]) : 0.0;
  *reinterpret_cast<elem_v2d*>(bx + x * 2) = vx;
  *reinterpret_cast<elem_v2d*>(by + x * 2) = vy;
}

// the window of a tile inside its level: element e0 at x = 0, te elements; x in [lo, hi] lies inside the level (never
// empty: the launcher's tiles all start inside their levels)
struct PairElemWindow {
  int lo, hi;
};
__device__ __forceinline__ PairElemWindow pair_elem_window(int64_t e0, int64_t ne, int te) {
  const int64_t rem = ne - 1 - e0;
  PairElemWindow w;
  w.lo = e0 < 0 ? (int)-e0 : 0;
  w.hi = rem < te - 1 ? (int)rem : te - 1;
  return w;
}

// descent: the schedule of btd_pair_down_dict_kernel
template <int NT>
__global__ __launch_bounds__(NT) void btd_pair_down_elem_kernel(PairArgs a, SweepWeights wa, SweepWeights wb, PairElemDict d) {
  constexpr int TEA = NT, TEB = NT / 2;
  extern __shared__ double lds[];
  double* buf0 = lds + 2;
  double* buf1 = lds + (TEA + 2) * 2 + 2;
  double* rhsB = lds + 2 * (TEA + 2) * 2;   // [TEB][2]
  double* tabA = rhsB + TEB * 2;
  double* tabB = tabA + d.nca * kPairRecWords;

  const int x = threadIdx.x;
  const int h = a.nsweeps + 1;
  const int64_t Eb0 = (int64_t)blockIdx.x * a.own - h;
  const int rhoA = a.ab.rho;
  const int64_t Ea0 = Eb0 * rhoA - h;
  const PairElemWindow wA = pair_elem_window(Ea0, a.A.ne, a.te_a), wB = pair_elem_window(Eb0, a.B.ne, a.te_b);
  const bool validA = x >= wA.lo && x <= wA.hi;
  const bool actB = x < TEB;
  const bool validB = x >= wB.lo && x <= wB.hi;
  const unsigned xcA = (unsigned)(x < wA.lo ? wA.lo : x > wA.hi ? wA.hi : x);
  const unsigned xcB = (unsigned)(x < wB.lo ? wB.lo : x > wB.hi ? wB.hi : x);

  // ---------------- the loads: the classes and level a's right-hand side, then the tables ---------------------------
  const int ca = (int)(d.cls_a + Ea0)[xcA];
  const int cb = (int)(d.cls_b + Eb0)[xcB];
  double bb[2];
  elem_ld2(a.rhs_a + Ea0 * 2 + xcA * 2, bb[0], bb[1]);
  pair_elem_stage<NT>(tabA, tabB, d, x);
  if (!validA) bb[0] = bb[1] = 0.0;

  // ---------------- level a: nsweeps sweeps from zero, residual, restriction into LDS ----------------------------
  {
    if (x < 2) {
      buf0[-2 + x] = 0.0;
      buf0[TEA * 2 + x] = 0.0;
      buf1[-2 + x] = 0.0;
      buf1[TEA * 2 + x] = 0.0;
    }
    buf0[x * 2] = 0.0;
    buf0[x * 2 + 1] = 0.0;
    __syncthreads();   // (the tables too)
    const double* rec = tabA + ca * kPairRecWords;
    double g[2], P[2][2], Q[2][2];
    double uu[2] = {0.0, 0.0};            // u = zeros below the finest level (src/solvers.jl:29-31)
    pair_elem_rows(rec, bb, g, P, Q);
    double* cur = buf0;
    double* nxt = buf1;
    pair_elem_sweeps(a.nsweeps, wa, x, true, validA, g, P, Q, uu, cur, nxt);
    // iterate of the children of the owned level-b elements
    const int xs0 = h + h * rhoA, xs1 = h + (h + a.own) * rhoA;
    if (validA && x >= xs0 && x < xs1) pair_elem_st2(a.u_a + Ea0 * 2 + (unsigned)(x * 2), uu[0], uu[1]);
    const bool in = validA && x >= h && x < a.te_a - h;
    double rr[2] = {0.0, 0.0};
    if (in) pair_elem_residual(rec, cur, x, bb, uu, rr);   // (a valid element's uu is its words of cur)
    __syncthreads();   // every residual has read the iterate: both buffers are free for the products
    pair_elem_products(rec, in, x, rr, nxt, cur);
    __syncthreads();
    // rhs_b = L' r for EVERY element of the level-b tile (ascending fine row, as the column dot of L')
    for (int t = x; t < a.te_b * 2; t += NT) {
      const int Jl = t >> 1, c = t & 1;
      double acc = 0.0;
      if (Jl >= wB.lo && Jl <= wB.hi) {
        const double* pr = (c ? cur : nxt) + (h + Jl * rhoA) * 2;
        for (int k = 0; k < rhoA * 2; ++k) acc = __dadd_rn(acc, pr[k]);
        if (Jl >= h && Jl < h + a.own) a.rhs_b[(Eb0 + Jl) * 2 + c] = acc;
      }
      rhsB[t] = acc;
    }
    __syncthreads();
  }

  // ---------------- level b: nsweeps sweeps from zero, residual, restriction to level b + 1 ----------------------
  {
    double* b0 = lds + 2;
    double* b1 = lds + (TEB + 2) * 2 + 2;
    if (x < 2) {
      b0[-2 + x] = 0.0;
      b0[TEB * 2 + x] = 0.0;
      b1[-2 + x] = 0.0;
      b1[TEB * 2 + x] = 0.0;
    }
    const double* rec = tabB + cb * kPairRecWords;
    double g[2], P[2][2], Q[2][2], bbB[2] = {0.0, 0.0};
    double uu[2] = {0.0, 0.0};
    if (actB) {
      if (validB) elem_ld2(rhsB + x * 2, bbB[0], bbB[1]);
      pair_elem_rows(rec, bbB, g, P, Q);
      b0[x * 2] = 0.0;
      b0[x * 2 + 1] = 0.0;
    }
    __syncthreads();
    double* cur = b0;
    double* nxt = b1;
    pair_elem_sweeps(a.nsweeps, wb, x, actB, validB, g, P, Q, uu, cur, nxt);
    const bool own = actB && validB && x >= h && x < h + a.own;
    double rr[2] = {0.0, 0.0};
    if (own) {
      pair_elem_st2(a.u_b + Eb0 * 2 + (unsigned)(x * 2), uu[0], uu[1]);
      pair_elem_residual(rec, cur, x, bbB, uu, rr);
    }
    __syncthreads();
    if (actB) pair_elem_products(rec, own, x, rr, nxt, cur);
    __syncthreads();
    const int rhoB = a.bc.rho;
    const int ncoarse = a.own / rhoB;
    const int64_t J0 = ((int64_t)blockIdx.x * a.own) / rhoB;
    for (int t = x; t < ncoarse * 2; t += NT) {
      const int Jl = t >> 1, c = t & 1;
      const int64_t J = J0 + Jl;
      if (J >= a.bc.nec) continue;
      const double* pr = (c ? cur : nxt) + (h + Jl * rhoB) * 2;
      double acc = 0.0;
      for (int k = 0; k < rhoB * 2; ++k) acc = __dadd_rn(acc, pr[k]);
      a.rhs_c[J * 2 + c] = acc;
    }
  }
}

// ascent (every tile of the level: the partitioned cycle's tile selections keep the full-array kernels): the schedule
// of btd_pair_up_dict_kernel
template <int NT>
__global__ __launch_bounds__(NT) void btd_pair_up_elem_kernel(PairArgs a, SweepWeights wa, SweepWeights wb, PairElemDict d) {
  constexpr int TEA = NT, TEB = NT / 2;
  extern __shared__ double lds[];
  double* uB = lds + 2 * (TEA + 2) * 2;   // [TEB][2]: post-smoothed level-b iterate of the tile
  double* tabA = uB + TEB * 2;
  double* tabB = tabA + d.nca * kPairRecWords;

  const int x = threadIdx.x;
  const int ns = a.nsweeps;
  const int rhoA = a.ab.rho, rhoB = a.bc.rho;
  const int64_t tile = (int64_t)blockIdx.x;
  const int64_t Ea0 = tile * a.own - ns;
  const int64_t Eb0 = (tile * a.own) / rhoA - a.hb - ns;
  const PairElemWindow wA = pair_elem_window(Ea0, a.A.ne, a.te_a), wB = pair_elem_window(Eb0, a.B.ne, a.te_b);
  const bool validA = x >= wA.lo && x <= wA.hi;
  const bool actB = x < TEB;
  const bool validB = x >= wB.lo && x <= wB.hi;
  const unsigned xcA = (unsigned)(x < wA.lo ? wA.lo : x > wA.hi ? wA.hi : x);
  const unsigned xcB = (unsigned)(x < wB.lo ? wB.lo : x > wB.hi ? wB.hi : x);

  // ---------------- the loads of both levels, then the tables ------------------------------------------------------
  const int cb = (int)(d.cls_b + Eb0)[xcB];
  const int ca = (int)(d.cls_a + Ea0)[xcA];
  double bbB[2], ubv[2], ucx, ucy, bbA[2], ua[2];
  {
    const int64_t eb = Eb0 + xcB;
    // J = e / rho, a 32-bit division wherever the level's elements count in 31 bits
    const int64_t J = a.B.ne <= 0x7fffffff ? (int64_t)((unsigned)eb / (unsigned)rhoB) : eb / rhoB;
    elem_ld2(a.rhs_b_in + eb * 2, bbB[0], bbB[1]);
    elem_ld2(a.ub_in + eb * 2, ubv[0], ubv[1]);
    elem_ld2(a.uc + J * 2, ucx, ucy);
    elem_ld2(a.rhs_a + Ea0 * 2 + xcA * 2, bbA[0], bbA[1]);
    elem_ld2(a.ua_in + Ea0 * 2 + xcA * 2, ua[0], ua[1]);
  }
  pair_elem_stage<NT>(tabA, tabB, d, x);

  // ---------------- level b -------------------------------------------------------------------------------------
  {
    double* b0 = lds + 2;
    double* b1 = lds + (TEB + 2) * 2 + 2;
    if (x < 2) {
      b0[-2 + x] = 0.0;
      b0[TEB * 2 + x] = 0.0;
      b1[-2 + x] = 0.0;
      b1[TEB * 2 + x] = 0.0;
    }
    __syncthreads();   // the tables
    const double* rec = tabB + cb * kPairRecWords;
    double g[2], P[2][2], Q[2][2];
    double uu[2] = {0.0, 0.0};
    if (actB) {
      if (validB) {
        // u += L uc (ascending mode order): the second product rounded, the first fused into the sum
        double lx[2], ly[2];
        elem_ld2(rec + kPairRecLf, lx[0], ly[0]);
        elem_ld2(rec + kPairRecLf + 2, lx[1], ly[1]);
#pragma unroll
        for (int i = 0; i < 2; ++i) uu[i] = __dadd_rn(ubv[i], __fma_rn(lx[i], ucx, __dmul_rn(ly[i], ucy)));
      } else {
        bbB[0] = bbB[1] = 0.0;
      }
      pair_elem_rows(rec, bbB, g, P, Q);
      b0[x * 2] = uu[0];
      b0[x * 2 + 1] = uu[1];
    }
    __syncthreads();
    double* cur = b0;
    double* nxt = b1;
    pair_elem_sweeps(ns, wb, x, actB, validB, g, P, Q, uu, cur, nxt);
    if (actB) {
      uB[x * 2] = uu[0];
      uB[x * 2 + 1] = uu[1];
      if (a.ub_out && validB) {
        const int64_t ob0 = (tile * a.own) / rhoA, ob1 = ob0 + a.own / rhoA;   // the parents of the owned level-a range
        const int64_t e = Eb0 + x;
        if (e >= ob0 && e < ob1) pair_elem_st2(a.ub_out + e * 2, uu[0], uu[1]);
      }
    }
    __syncthreads();
  }

  // ---------------- level a -------------------------------------------------------------------------------------
  {
    double* buf0 = lds + 2;
    double* buf1 = lds + (TEA + 2) * 2 + 2;
    if (x < 2) {
      buf0[-2 + x] = 0.0;
      buf0[TEA * 2 + x] = 0.0;
      buf1[-2 + x] = 0.0;
      buf1[TEA * 2 + x] = 0.0;
    }
    const double* rec = tabA + ca * kPairRecWords;
    double g[2], P[2][2], Q[2][2];
    double uu[2] = {0.0, 0.0};
    if (validA) {
      // the parent's place in the level-b tile: (e / rho_a) - Eb0 with e = tile own + x - ns, own a multiple of rho_a and
      // hb rho_a >= ns -- a 32-bit division
      const int xb = (int)((unsigned)(x - ns + a.hb * rhoA) / (unsigned)rhoA) + ns;
      double u2x, u2y, lx[2], ly[2];
      elem_ld2(uB + xb * 2, u2x, u2y);
      elem_ld2(rec + kPairRecLf, lx[0], ly[0]);
      elem_ld2(rec + kPairRecLf + 2, lx[1], ly[1]);
#pragma unroll
      for (int i = 0; i < 2; ++i) uu[i] = __dadd_rn(ua[i], __fma_rn(lx[i], u2x, __dmul_rn(ly[i], u2y)));
    } else {
      bbA[0] = bbA[1] = 0.0;
    }
    pair_elem_rows(rec, bbA, g, P, Q);
    // (the level-b buffers and this level's share the front of the LDS: all reads of uB -- behind them -- are done by
    // value above, the buffers themselves were last read in level b's sweeps, a barrier ago)
    buf0[x * 2] = uu[0];
    buf0[x * 2 + 1] = uu[1];
    __syncthreads();
    double* cur = buf0;
    double* nxt = buf1;
    pair_elem_sweeps(ns, wa, x, true, validA, g, P, Q, uu, cur, nxt);
    if (validA && x >= ns && x < ns + a.own) pair_elem_st2(a.u_a + Ea0 * 2 + (unsigned)(x * 2), uu[0], uu[1]);
  }
}

}  // namespace aggmg
