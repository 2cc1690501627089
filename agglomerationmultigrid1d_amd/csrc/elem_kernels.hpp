// Element-thread form of the dictionary variant of the fused kernel (AGGMG_OPT_ELEMENT_THREADS): one THREAD owns an
// element -- all M rows of it, its b, u, g, pcol, B^{-1}[:, r_sup] and q in registers -- where btd_fused_kernel<...,
// DICT = true> gives every row a thread.  The row-thread layout repeats the element's index, class, validity and address
// arithmetic in each of its M lanes, builds every row of the packed triangle with per-entry selects and forms every
// B^{-1} v and q . u+ out of DPP broadcasts and quad sums: at M = 4 about nine tenths of the VALU instructions on a
// cycle's path are not fp64 arithmetic, and the instruction count alone accounts for the launch's time
// (profiles/r26_element_threads.md).  Here the per-element work is done once and the 4 x 4 products are register FMAs.
//
// Same schedule (loads up front, block-Jacobi sweeps ping-pong in LDS with one barrier each, explicit residual from the
// lossless symmetric form with its escapes, two-mode restriction through LDS in ascending fine row) and the SAME BITS:
// every expression is the one btd_fused_kernel<4, true, 2, true, 256, false, false, SR, true> is compiled to, pinned
// with __fma_rn / __dmul_rn / __dadd_rn so that no contraction depends on the code around it.
#pragma once
#include <type_traits>

#include "host_plan.hpp"
#include "kernels.hpp"

namespace aggmg {

// the element's class record words, two doubles per load
typedef double elem_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void elem_ld2(const double* p, double& x, double& y) {
  const elem_v2d v = *reinterpret_cast<const elem_v2d*>(p);
  x = v.x;
  y = v.y;
}
// index of entry (i, j), i <= j, in the packed upper triangle of an M x M block (row-owned runs)
template <int M>
__host__ __device__ constexpr int elem_tri(int i, int j) {
  return i * M - (i * (i - 1)) / 2 + (j - i);
}
// row i of the symmetric block held as its packed upper triangle, times v: btd_group_apply's chain, 0.0 first
template <int M>
__device__ __forceinline__ double elem_sym_row_apply(const double (&tri)[M * (M + 1) / 2], int i, const double (&v)[M]) {
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) acc = __fma_rn(tri[i < j ? elem_tri<M>(i, j) : elem_tri<M>(j, i)], v[j], acc);
  return acc;
}
// q . u+ as group_dot<4> leaves it in the lanes of an element: lane i holds fma(a_i, b_i, rnd(a_{i^2} b_{i^2})) +
// fma(a_{i^1}, b_{i^1}, rnd(a_{i^3} b_{i^3})) -- one value in rows 0, 1 (lo), another, differently rounded, in rows 2, 3 (hi)
__device__ __forceinline__ void elem_group_dot4(const double (&a)[4], const double (&b)[4], double& lo, double& hi) {
  const double p0 = __dmul_rn(a[0], b[0]), p1 = __dmul_rn(a[1], b[1]);
  const double p2 = __dmul_rn(a[2], b[2]), p3 = __dmul_rn(a[3], b[3]);
  lo = __dadd_rn(__fma_rn(a[0], b[0], p2), __fma_rn(a[1], b[1], p3));
  hi = __dadd_rn(__fma_rn(a[2], b[2], p0), __fma_rn(a[3], b[3], p1));
}

constexpr int kElemThreads = 256;   // threads of a workgroup = elements of a tile (owned + halos), one slab
// LDS of a launch: two iterate buffers, component-major -- buf[j][x], x in [-1, TE] with a zero element at either end --
// so the reads of a sweep (four of u+, one of u-[c_sub]) and its four writes are consecutive 8-byte words across a wave
template <int M>
constexpr size_t elem_lds_bytes() {
  return (size_t)2 * M * (kElemThreads + 2) * sizeof(double);
}

// SR: the explicit residual reads the lossless symmetric form (BtdLevel::dup / corr by class); otherwise the full rows of
// the dictionary (dblk / scol by class).  What the launcher guarantees (launch_btd_t): a dictionary launch (cls, packed
// inverse, qmir), block-Jacobi, nsweeps >= 1, two-mode transfers of equal agglomerates, no stored residual, no (L'D)
// restriction, no checkpoint; a residual is always restricted (lf_out).
template <int M, bool SR>
__global__ __launch_bounds__(kElemThreads) void btd_elem_dict_kernel(FusedArgs a, SweepWeights wts) {
  static_assert(M == 4, "the element-thread kernel's block size");
  constexpr int TE = kElemThreads;
  constexpr int S = TE + 2;            // words of one component in a buffer
  constexpr int T = M * (M + 1) / 2;
  extern __shared__ double lds[];
  double* cur = lds + 1;               // (j, x) at cur[j * S + x]
  double* nxt = lds + M * S + 1;

  const int x = threadIdx.x;
  const int64_t ne = a.lv.ne;
  const int64_t e0 = fused_tile(a) * a.owned - a.halo_left;   // element at x = 0
  const int own0 = a.halo_left, own1 = a.halo_left + a.owned;
  // x in [xlo, xhi] lies inside the level; a lane outside reads the nearest element that does and is masked.  (The
  // launcher's tiles all own an element of the level; a tile past it would leave here, before any barrier.)
  const int64_t rem = ne - 1 - e0;
  if (rem < 0) return;
  const int xlo = e0 < 0 ? (int)-e0 : 0, xhi = rem < TE - 1 ? (int)rem : TE - 1;
  const bool valid = x >= xlo && x <= xhi;
  const bool own = valid && x >= own0 && x < own1;
  const unsigned xc = (unsigned)(x < xlo ? xlo : x > xhi ? xhi : x);

  if (x < 4 * M) {   // the zero elements at the ends of both buffers
    const int j = x & (M - 1), w = x / M;
    (w & 2 ? nxt : cur)[j * S + (w & 1 ? TE : -1)] = 0.0;
  }

  // ---- loads: first what depends on nothing the tile has loaded -- cls, b, u_in, the coarse pair -- straight-line ----
  const bool pro = a.lf_in != nullptr;
  const int64_t ce = (int64_t)(a.lv.cls + e0)[xc];
  double bb[M], uu[M];
  {
    const double* const bp = a.b + e0 * M + xc * M;
    // (no first iterate: the load goes to b's line and is dropped -- no branch in the load group)
    const double* const up = (a.u_in ? a.u_in : a.b) + e0 * M + xc * M;
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(bp + j, bb[j], bb[j + 1]);
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(up + j, uu[j], uu[j + 1]);
    if (!a.u_in) {
#pragma unroll
      for (int j = 0; j < M; ++j) uu[j] = 0.0;
    }
  }
  double ucx = 0.0, ucy = 0.0;
  if (pro) {
    // J = e / rho_in, a 32-bit division wherever the level's elements count in 31 bits
    const int64_t J = ne <= 0x7fffffff ? (int64_t)((unsigned)(e0 + xc) / (unsigned)a.rho_in) : (e0 + xc) / a.rho_in;
    elem_ld2(a.uc + J * 2, ucx, ucy);
  }
  // ... then the record of the element's class, from cache: the packed inverse whole, q_{e-1}, q_e, the rows of L
  double tri[T], qm[M], q[M];
#pragma unroll
  for (int k = 0; k < T; k += 2) elem_ld2(a.lv.bsym + ce * T + k, tri[k], tri[k + 1]);
#pragma unroll
  for (int j = 0; j < M; j += 2) elem_ld2(a.lv.qmir + ce * M + j, qm[j], qm[j + 1]);
#pragma unroll
  for (int j = 0; j < M; j += 2) elem_ld2(a.lv.qrow + ce * M + j, q[j], q[j + 1]);
  if (pro) {
    double lx[M], ly[M];
    if (a.lf1_in) {
#pragma unroll
      for (int j = 0; j < M; j += 2) elem_ld2(a.lf1_in + ce * M + j, ly[j], ly[j + 1]);
#pragma unroll
      for (int j = 0; j < M; ++j) lx[j] = 1.0;
    } else {
#pragma unroll
      for (int j = 0; j < M; ++j) elem_ld2(a.lf_in + (ce * M + j) * 2, lx[j], ly[j]);
    }
    // u += L uc: the second product rounded, the first fused into the sum
#pragma unroll
    for (int j = 0; j < M; ++j) uu[j] = __dadd_rn(uu[j], __fma_rn(lx[j], ucx, __dmul_rn(ly[j], ucy)));
  }
  if (!valid) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      uu[j] = 0.0;
      bb[j] = 0.0;
    }
  }
  // g = B^{-1} b, pcol = B^{-1} q_{e-1}, column r_sup of B^{-1} (symmetric: its row)
  double g[M], pc[M], br[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    g[i] = elem_sym_row_apply<M>(tri, i, bb);
    pc[i] = elem_sym_row_apply<M>(tri, i, qm);
    br[i] = 0.0;
    cur[i * S + x] = uu[i];
  }
  // (r_sup is the launch's: one branch, then moves -- not a select per entry and row)
  auto sym_col = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
#pragma unroll
    for (int i = 0; i < M; ++i) br[i] = tri[i < j ? elem_tri<M>(i, j) : elem_tri<M>(j, i)];
  };
  switch (a.lv.r_sup) {
    case 0: sym_col(std::integral_constant<int, 0>()); break;
    case 1: sym_col(std::integral_constant<int, 1>()); break;
    case 2: sym_col(std::integral_constant<int, 2>()); break;
    case 3: sym_col(std::integral_constant<int, 3>()); break;
  }
  __syncthreads();

  // ---- block-Jacobi sweeps, LDS ping-pong: u + w (g - pcol u-[c_sub] - B^{-1}[:, r_sup] (q . u+) - u) ----------------
  const int c_sub = a.lv.c_sub;
  for (int sw = 0; sw < a.nsweeps; ++sw) {
    const double um = cur[c_sub * S + x - 1];
    double up[M];
#pragma unroll
    for (int j = 0; j < M; ++j) up[j] = cur[j * S + x + 1];
    double dlo, dhi;
    elem_group_dot4(q, up, dlo, dhi);
    const double w = wts.w[(unsigned)sw];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double acc = __fma_rn(-pc[i], um, g[i]);
      acc = __fma_rn(-br[i], i < 2 ? dlo : dhi, acc);
      double un = __fma_rn(w, __dadd_rn(acc, -uu[i]), uu[i]);
      if (!valid) un = 0.0;
      uu[i] = un;
      nxt[i * S + x] = un;
    }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  }

  // ---- the iterate of the owned elements -------------------------------------------------------------------------
  if (a.u_out && own) {
    double* const op = a.u_out + e0 * M + (unsigned)(x * M);
#pragma unroll
    for (int j = 0; j < M; j += 2) {
      elem_v2d v;
      v.x = uu[j];
      v.y = uu[j + 1];
#if AGGMG_NT & 2
      __builtin_nontemporal_store(v, reinterpret_cast<elem_v2d*>(op + j));
#else
      *reinterpret_cast<elem_v2d*>(op + j) = v;
#endif
    }
  }
  if (!a.do_residual) return;

  // ---- explicit residual r = b - A u of the element's rows, ascending column order: the coupling entry times
  // u-[c_sub], the row of D_e, and (row r_sup) q . u+ in that row's rounding --------------------------------------
  double D[M][M], sc[M];
  if constexpr (SR) {
    // the upper triangle whole; a lower entry, and the coupling entry, is its mirror's bit pattern plus the int8
    // difference of the row's corr word; the escapes (the level's first element; a difference that does not fit) come
    // from the full rows of the record
    double du[T];
#pragma unroll
    for (int k = 0; k < T; k += 2) elem_ld2(a.lv.dup + ce * T + k, du[k], du[k + 1]);
    const uint4 w4 = *reinterpret_cast<const uint4*>(a.lv.corr + ce * M);
    const uint32_t w[M] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(a.lv.qmir + ce * M + j, sc[j], sc[j + 1]);
    bool esc = false;
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int j = 0; j < M; ++j) {
        if (j >= i) {
          D[i][j] = du[elem_tri<M>(i, j)];
        } else {
          const int d = (int)(int8_t)(w[i] >> (8 * j));
          D[i][j] = sym_residual_decode(du[elem_tri<M>(j, i)], d);
          esc |= d == kSymResidualEscape;
        }
      }
      const int dc = (int)(int8_t)(w[i] >> 24);
      sc[i] = sym_residual_decode(sc[i], dc);
      esc |= dc == kSymResidualEscape;
    }
    if (__builtin_expect(own && esc, 0)) {
#pragma unroll
      for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j)
          if ((int)(int8_t)(w[i] >> (8 * j)) == kSymResidualEscape) D[i][j] = a.lv.dblk[(ce * M + i) * M + j];
        if ((int)(int8_t)(w[i] >> 24) == kSymResidualEscape) sc[i] = a.lv.scol[ce * M + i];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int j = 0; j < M; j += 2) elem_ld2(a.lv.dblk + (ce * M + i) * M + j, D[i][j], D[i][j + 1]);
    }
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(a.lv.scol + ce * M + j, sc[j], sc[j + 1]);
  }
  // the rows of L' of the restriction, record words too
  double lx[M], ly[M];
  if (a.lf1_out) {   // unit first column: 1.0 * r is r, bit for bit what the stored 1.0 gives
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(a.lf1_out + ce * M + j, ly[j], ly[j + 1]);
#pragma unroll
    for (int j = 0; j < M; ++j) lx[j] = 1.0;
  } else {
#pragma unroll
    for (int j = 0; j < M; ++j) elem_ld2(a.lf_out + (ce * M + j) * 2, lx[j], ly[j]);
  }
  double rr[M];
  {
    const double um = cur[c_sub * S + x - 1];
    double up[M];
#pragma unroll
    for (int j = 0; j < M; ++j) up[j] = cur[j * S + x + 1];
    double dlo, dhi;
    elem_group_dot4(q, up, dlo, dhi);
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double t = __fma_rn(sc[i], um, 0.0);
#pragma unroll
      for (int j = 0; j < M; ++j) t = __fma_rn(D[i][j], uu[j], t);   // (a valid element's uu is its words of cur)
      if (i == a.lv.r_sup) t = __dadd_rn(t, i < 2 ? dlo : dhi);
      rr[i] = own ? __dadd_rn(bb[i], -t) : 0.0;
    }
  }

  // ---- restriction onto two coarse modes: every element leaves its rows' two products in the (now free) iterate
  // buffers; one thread per (J, mode) adds them, 0.0 first, in ascending fine row ---------------------------------------
  __syncthreads();
#pragma unroll
  for (int i = 0; i < M; ++i) {
    nxt[i * S + x] = own ? __dmul_rn(lx[i], rr[i]) : 0.0;
    cur[i * S + x] = own ? __dmul_rn(ly[i], rr[i]) : 0.0;
  }
  __syncthreads();
  const int rho = a.rho_out;
  const int ncoarse = a.owned / rho;   // owned coarse elements of this tile
  const int64_t J0 = fused_tile(a) * ncoarse;
  for (int t = x; t < ncoarse * 2; t += TE) {
    const int Jl = t >> 1, c = t & 1;
    const int64_t J = J0 + Jl;
    if (J >= a.nec_out) continue;
    const double* pr = (c ? cur : nxt) + a.halo_left + Jl * rho;
    double acc = 0.0;
    for (int k = 0; k < rho; ++k) {
#pragma unroll
      for (int j = 0; j < M; ++j) acc = __dadd_rn(acc, pr[j * S + k]);
    }
    a.rc_out[J * 2 + c] = acc;
  }
}

// The ascent that REPLAYS the pre-smoothing (AGGMG_OPT_REPLAY_PRESMOOTH): what the descent stores only for the ascent to
// read back -- the pre-smoothed iterate, a vector written and a vector read per cycle -- is rebuilt here from the
// descent's own inputs.  The launch reads u_in where the ascent reads the stored iterate (the cycle's first iterate;
// null: zeros, read not at all), runs the descent's npre sweeps, adds the prolongation, and goes on with the post sweeps:
// a.nsweeps = npre + npost sweeps with the weights wts.w[0 .. npre) ++ wts.w[npre .. nsweeps), a halo of nsweeps elements.
// The same arithmetic on the same inputs in the same order as btd_elem_dict_kernel's descent and ascent, so the SAME
// BITS.  The prolongation's terms fma(lx, ucx, rnd(ly ucy)) are formed with the loads -- four words held over the
// pre-sweeps -- and added where the last pre-sweep writes its result: u_pre + L uc is what the ascent forms from the
// stored u_pre, and no barrier is spent on it.  Lanes outside the level stay 0.0, as the sweeps leave them.
// What the launcher guarantees: btd_elem_dict_kernel's conditions for an ascent (lf_in, uc, no residual),
// 1 <= npre < a.nsweeps <= kSweepWeights, and u_in's range disjoint from u_out's (the launch reads u_in's halos while
// other workgroups store).
template <int M>
__global__ __launch_bounds__(kElemThreads) void btd_elem_replay_up_kernel(FusedArgs a, SweepWeights wts, int npre) {
  static_assert(M == 4, "the element-thread kernel's block size");
  constexpr int TE = kElemThreads;
  constexpr int S = TE + 2;            // words of one component in a buffer
  constexpr int T = M * (M + 1) / 2;
  extern __shared__ double lds[];
  double* cur = lds + 1;               // (j, x) at cur[j * S + x]
  double* nxt = lds + M * S + 1;

  const int x = threadIdx.x;
  const int64_t ne = a.lv.ne;
  const int64_t e0 = fused_tile(a) * a.owned - a.halo_left;   // element at x = 0
  const int own0 = a.halo_left, own1 = a.halo_left + a.owned;
  const int64_t rem = ne - 1 - e0;
  if (rem < 0) return;   // a tile wholly past the level: before any barrier
  const int xlo = e0 < 0 ? (int)-e0 : 0, xhi = rem < TE - 1 ? (int)rem : TE - 1;
  const bool valid = x >= xlo && x <= xhi;
  const bool own = valid && x >= own0 && x < own1;
  const unsigned xc = (unsigned)(x < xlo ? xlo : x > xhi ? xhi : x);

  if (x < 4 * M) {   // the zero elements at the ends of both buffers
    const int j = x & (M - 1), w = x / M;
    (w & 2 ? nxt : cur)[j * S + (w & 1 ? TE : -1)] = 0.0;
  }

  // ---- loads, straight-line: cls, b, u_in, the coarse pair; then the class record from cache -------------------------
  const int64_t ce = (int64_t)(a.lv.cls + e0)[xc];
  double bb[M], uu[M];
  {
    const double* const bp = a.b + e0 * M + xc * M;
    const double* const up = (a.u_in ? a.u_in : a.b) + e0 * M + xc * M;   // (no first iterate: b's line again, dropped)
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(bp + j, bb[j], bb[j + 1]);
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(up + j, uu[j], uu[j + 1]);
    if (!a.u_in) {
#pragma unroll
      for (int j = 0; j < M; ++j) uu[j] = 0.0;
    }
  }
  double ucx, ucy;
  {
    const int64_t J = ne <= 0x7fffffff ? (int64_t)((unsigned)(e0 + xc) / (unsigned)a.rho_in) : (e0 + xc) / a.rho_in;
    elem_ld2(a.uc + J * 2, ucx, ucy);
  }
  double tri[T], qm[M], q[M];
#pragma unroll
  for (int k = 0; k < T; k += 2) elem_ld2(a.lv.bsym + ce * T + k, tri[k], tri[k + 1]);
#pragma unroll
  for (int j = 0; j < M; j += 2) elem_ld2(a.lv.qmir + ce * M + j, qm[j], qm[j + 1]);
#pragma unroll
  for (int j = 0; j < M; j += 2) elem_ld2(a.lv.qrow + ce * M + j, q[j], q[j + 1]);
  // L uc of the element's rows: the second product rounded, the first fused into the sum
  double luc[M];
  {
    double lx[M], ly[M];
    if (a.lf1_in) {
#pragma unroll
      for (int j = 0; j < M; j += 2) elem_ld2(a.lf1_in + ce * M + j, ly[j], ly[j + 1]);
#pragma unroll
      for (int j = 0; j < M; ++j) lx[j] = 1.0;
    } else {
#pragma unroll
      for (int j = 0; j < M; ++j) elem_ld2(a.lf_in + (ce * M + j) * 2, lx[j], ly[j]);
    }
#pragma unroll
    for (int j = 0; j < M; ++j) luc[j] = __fma_rn(lx[j], ucx, __dmul_rn(ly[j], ucy));
  }
  if (!valid) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      uu[j] = 0.0;
      bb[j] = 0.0;
    }
  }
  // g = B^{-1} b, pcol = B^{-1} q_{e-1}, column r_sup of B^{-1} (symmetric: its row)
  double g[M], pc[M], br[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    g[i] = elem_sym_row_apply<M>(tri, i, bb);
    pc[i] = elem_sym_row_apply<M>(tri, i, qm);
    br[i] = 0.0;
    cur[i * S + x] = uu[i];
  }
  auto sym_col = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
#pragma unroll
    for (int i = 0; i < M; ++i) br[i] = tri[i < j ? elem_tri<M>(i, j) : elem_tri<M>(j, i)];
  };
  switch (a.lv.r_sup) {
    case 0: sym_col(std::integral_constant<int, 0>()); break;
    case 1: sym_col(std::integral_constant<int, 1>()); break;
    case 2: sym_col(std::integral_constant<int, 2>()); break;
    case 3: sym_col(std::integral_constant<int, 3>()); break;
  }
  __syncthreads();

  // ---- block-Jacobi sweeps, LDS ping-pong: u + w (g - pcol u-[c_sub] - B^{-1}[:, r_sup] (q . u+) - u); the last
  // pre-sweep leaves u + L uc ------------------------------------------------------------------------------------------
  // (the sweep is written once and placed three times -- the pre-sweeps but the last, the last one, the post-sweeps -- so
  // that the sweeps that add nothing carry no select for it: a conditional add per row in one common loop cost the launch
  // 7.12 instead of 5.51 vector instructions per element, profiles/r28_replay.md)
  const int c_sub = a.lv.c_sub;
  auto sweep = [&](int sw, auto add_luc) {
    const double um = cur[c_sub * S + x - 1];
    double up[M];
#pragma unroll
    for (int j = 0; j < M; ++j) up[j] = cur[j * S + x + 1];
    double dlo, dhi;
    elem_group_dot4(q, up, dlo, dhi);
    const double w = wts.w[(unsigned)sw];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double acc = __fma_rn(-pc[i], um, g[i]);
      acc = __fma_rn(-br[i], i < 2 ? dlo : dhi, acc);
      double un = __fma_rn(w, __dadd_rn(acc, -uu[i]), uu[i]);
      if constexpr (decltype(add_luc)::value) un = __dadd_rn(un, luc[i]);
      if (!valid) un = 0.0;
      uu[i] = un;
      nxt[i * S + x] = un;
    }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  };
  for (int sw = 0; sw < npre - 1; ++sw) sweep(sw, std::false_type());
  sweep(npre - 1, std::true_type());
  for (int sw = npre; sw < a.nsweeps; ++sw) sweep(sw, std::false_type());

  // ---- the iterate of the owned elements -------------------------------------------------------------------------
  if (own) {
    double* const op = a.u_out + e0 * M + (unsigned)(x * M);
#pragma unroll
    for (int j = 0; j < M; j += 2) {
      elem_v2d v;
      v.x = uu[j];
      v.y = uu[j + 1];
#if AGGMG_NT & 2
      __builtin_nontemporal_store(v, reinterpret_cast<elem_v2d*>(op + j));
#else
      *reinterpret_cast<elem_v2d*>(op + j) = v;
#endif
    }
  }
}

// ---- the class records in LDS (AGGMG_OPT_ELEMENT_RECORDS_LDS) ----------------------------------------------------------
// The kernels above fetch the element's class record through the vector memory path in two further round trips -- the
// packed inverse, q_{e-1}, q_e and the rows of L once cls has landed, the residual's words after the sweeps -- although a
// level has a handful of classes and nearly every lane of a wave asks for the same few hundred bytes.  The kernels below
// copy the level's table of records into LDS at entry, with loads issued ahead of cls, b and u_in, and read every record
// word from LDS where it is used (lanes of one class read one address, which LDS broadcasts).  After the entry phase they
// issue no global load but the escape path's.  pcol = B^{-1} q_{e-1}, the same for every element of a class, comes with
// the record: formed at set-up by elem_sym_row_apply's chain (host_plan.hpp, elem_record_pack), so the 16 FMAs per element
// and the q_{e-1} registers go.  Everything else is the expression of the kernels above: the SAME BITS.
//
// The record's layout (kElemRecWords and the offsets kElemRec*) and its host repack: host_plan.hpp, elem_record_pack.
// The escape words (dblk, scol) stay in global memory behind the unlikely branch.
struct ElemRecTab {
  const double* rec;   // [nclasses][kElemRecWords]
  int nclasses;        // 1 .. kElemRecMaxClasses
};
template <int M>
constexpr size_t elem_rec_lds_bytes(int nclasses) {
  return elem_lds_bytes<M>() + (size_t)nclasses * kElemRecWords * sizeof(double);
}

// the table's loads, 16 bytes each, strided over the workgroup, as many rounds as the table has words for (a lane past
// the table in its last round reads its last word) ...
constexpr int kElemRecStage = (kElemRecMaxClasses * (kElemRecWords / 2) + kElemThreads - 1) / kElemThreads;
__device__ __forceinline__ void elem_rec_fetch(const ElemRecTab& t, int x, elem_v2d (&v)[kElemRecStage]) {
  const int n = t.nclasses * (kElemRecWords / 2);
#pragma unroll
  for (int k = 0; k < kElemRecStage; ++k) {
    const int i = x + k * kElemThreads;
    // (a round wholly past the table is not issued: n is the launch's, the branch uniform)
    if (k == 0 || k * kElemThreads < n) v[k] = reinterpret_cast<const elem_v2d*>(t.rec)[i < n ? i : n - 1];
  }
}
// ... and their stores, issued once the loads behind them (cls, b, u_in) are under way
__device__ __forceinline__ void elem_rec_store(double* tab, const ElemRecTab& t, int x, const elem_v2d (&v)[kElemRecStage]) {
  const int n = t.nclasses * (kElemRecWords / 2);
#pragma unroll
  for (int k = 0; k < kElemRecStage; ++k) {
    const int i = x + k * kElemThreads;
    if (i < n) reinterpret_cast<elem_v2d*>(tab)[i] = v[k];
  }
}

// Keeps the uses of a loaded value behind this point.  (The compiler moves register arithmetic on a loaded value over
// the table's barrier, and the wait for the streaming loads with it: the barrier would then wait for HBM.)
template <class V>
__device__ __forceinline__ void elem_rec_pin(V& v) {
  asm volatile("" : "+v"(v));
}
template <int M>
__device__ __forceinline__ void elem_rec_pin_all(unsigned& ce, double (&bb)[M], double (&uu)[M], double& ucx, double& ucy) {
  elem_rec_pin(ce);
#pragma unroll
  for (int j = 0; j < M; ++j) elem_rec_pin(bb[j]);
#pragma unroll
  for (int j = 0; j < M; ++j) elem_rec_pin(uu[j]);
  elem_rec_pin(ucx);
  elem_rec_pin(ucy);
}

// what a sweep reads of the record: q_e, pcol and column r_sup of B^{-1} -- four words of the packed triangle
template <int M>
struct ElemRecStencil {
  double q[M], pc[M], br[M];
  __device__ __forceinline__ void load(const double* rec, int r_sup) {
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(rec + kElemRecQrow + j, q[j], q[j + 1]);
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(rec + kElemRecPcol + j, pc[j], pc[j + 1]);
#pragma unroll
    for (int i = 0; i < M; ++i) br[i] = rec[kElemRecBsym + (i < r_sup ? elem_tri<M>(i, r_sup) : elem_tri<M>(r_sup, i))];
  }
};
// g = B^{-1} b from the record's packed triangle
template <int M>
__device__ __forceinline__ void elem_rec_g(const double* rec, const double (&bb)[M], double (&g)[M]) {
  constexpr int T = M * (M + 1) / 2;
  double tri[T];
#pragma unroll
  for (int k = 0; k < T; k += 2) elem_ld2(rec + kElemRecBsym + k, tri[k], tri[k + 1]);
#pragma unroll
  for (int i = 0; i < M; ++i) g[i] = elem_sym_row_apply<M>(tri, i, bb);
}
// one block-Jacobi sweep cur -> nxt and its barrier: u + w (g - pcol u-[c_sub] - B^{-1}[:, r_sup] (q . u+) - u), plus the
// prolongation's terms where ADD says so (the replaying ascent's last pre-sweep)
template <int M, bool ADD>
__device__ __forceinline__ void elem_rec_sweep(const ElemRecStencil<M>& st, double*& cur, double*& nxt, int x, int c_sub,
                                               double w, bool valid, const double (&g)[M], double (&uu)[M],
                                               const double* luc) {
  constexpr int S = kElemThreads + 2;
  const double um = cur[c_sub * S + x - 1];
  double up[M];
#pragma unroll
  for (int j = 0; j < M; ++j) up[j] = cur[j * S + x + 1];
  double dlo, dhi;
  elem_group_dot4(st.q, up, dlo, dhi);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double acc = __fma_rn(-st.pc[i], um, g[i]);
    acc = __fma_rn(-st.br[i], i < 2 ? dlo : dhi, acc);
    double un = __fma_rn(w, __dadd_rn(acc, -uu[i]), uu[i]);
    if constexpr (ADD) un = __dadd_rn(un, luc[i]);
    if (!valid) un = 0.0;
    uu[i] = un;
    nxt[i * S + x] = un;
  }
  __syncthreads();
  double* t = cur;
  cur = nxt;
  nxt = t;
}
__device__ __forceinline__ void elem_rec_st_iterate(double* op, const double (&uu)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    elem_v2d v;
    v.x = uu[j];
    v.y = uu[j + 1];
#if AGGMG_NT & 2
    __builtin_nontemporal_store(v, reinterpret_cast<elem_v2d*>(op + j));
#else
    *reinterpret_cast<elem_v2d*>(op + j) = v;
#endif
  }
}

// btd_elem_dict_kernel with the class table in LDS.  RES: the launch forms and restricts the explicit residual, from the
// lossless symmetric form (btd_elem_dict_kernel<M, true>'s launches: the descent, the launch between two cycles);
// otherwise it ends with the iterate (the storing ascent).  What the launcher guarantees beyond btd_elem_dict_kernel's
// conditions: t.rec is the level's table, 1 <= t.nclasses <= kElemRecMaxClasses, every cls word is below t.nclasses, the
// launch's LDS is elem_rec_lds_bytes<M>(t.nclasses), RES == (a.do_residual != 0), and a residual launch has dup / corr.
template <int M, bool RES>
__global__ __launch_bounds__(kElemThreads) void btd_elem_rec_kernel(FusedArgs a, SweepWeights wts, ElemRecTab t) {
  static_assert(M == 4, "the element-thread kernel's block size");
  constexpr int TE = kElemThreads;
  constexpr int S = TE + 2;            // words of one component in a buffer
  constexpr int T = M * (M + 1) / 2;
  extern __shared__ double lds[];
  double* cur = lds + 1;               // (j, x) at cur[j * S + x]
  double* nxt = lds + M * S + 1;
  double* const tab = lds + 2 * M * S; // the class table, behind the two buffers (16-byte aligned: 2 M S is even)

  const int x = threadIdx.x;
  const int64_t ne = a.lv.ne;
  const int64_t e0 = fused_tile(a) * a.owned - a.halo_left;   // element at x = 0
  const int own0 = a.halo_left, own1 = a.halo_left + a.owned;
  const int64_t rem = ne - 1 - e0;
  if (rem < 0) return;   // a tile wholly past the level: before any barrier
  const int xlo = e0 < 0 ? (int)-e0 : 0, xhi = rem < TE - 1 ? (int)rem : TE - 1;
  const bool valid = x >= xlo && x <= xhi;
  const bool own = valid && x >= own0 && x < own1;
  const unsigned xc = (unsigned)(x < xlo ? xlo : x > xhi ? xhi : x);

  // ---- loads: the table first, then cls, b, u_in, the coarse pair -- the only global loads of the launch (but the
  // escapes'); the table is stored and its barrier passed while the others are in flight ---------------------------------
  elem_v2d tv[kElemRecStage];
  elem_rec_fetch(t, x, tv);
  const bool pro = a.lf_in != nullptr;
  unsigned ce = (a.lv.cls + e0)[xc];
  double bb[M], uu[M];
  {
    const double* const bp = a.b + e0 * M + xc * M;
    const double* const up = (a.u_in ? a.u_in : a.b) + e0 * M + xc * M;   // (no first iterate: b's line again, dropped)
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(bp + j, bb[j], bb[j + 1]);
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(up + j, uu[j], uu[j + 1]);
  }
  double ucx = 0.0, ucy = 0.0;
  if (pro) {
    const int64_t J = ne <= 0x7fffffff ? (int64_t)((unsigned)(e0 + xc) / (unsigned)a.rho_in) : (e0 + xc) / a.rho_in;
    elem_ld2(a.uc + J * 2, ucx, ucy);
  }
  elem_rec_store(tab, t, x, tv);
  if (x < 4 * M) {   // the zero elements at the ends of both buffers
    const int j = x & (M - 1), w = x / M;
    (w & 2 ? nxt : cur)[j * S + (w & 1 ? TE : -1)] = 0.0;
  }
  __syncthreads();
  elem_rec_pin_all<M>(ce, bb, uu, ucx, ucy);
  if (!a.u_in) {
#pragma unroll
    for (int j = 0; j < M; ++j) uu[j] = 0.0;
  }

  const double* const rec = tab + ce * kElemRecWords;
  if (pro) {   // u += L uc: the second product rounded, the first fused into the sum
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double lx, ly;
      elem_ld2(rec + kElemRecLf + 2 * j, lx, ly);
      uu[j] = __dadd_rn(uu[j], __fma_rn(lx, ucx, __dmul_rn(ly, ucy)));
    }
  }
  if (!valid) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      uu[j] = 0.0;
      bb[j] = 0.0;
    }
  }
  double g[M];
  elem_rec_g<M>(rec, bb, g);
#pragma unroll
  for (int i = 0; i < M; ++i) cur[i * S + x] = uu[i];
  const int c_sub = a.lv.c_sub, r_sup = a.lv.r_sup;
  ElemRecStencil<M> st;
  st.load(rec, r_sup);   // held over the sweeps: re-reading per sweep measured 0.030 ms per cycle slower (r32)
  __syncthreads();

  for (int sw = 0; sw < a.nsweeps; ++sw)
    elem_rec_sweep<M, false>(st, cur, nxt, x, c_sub, wts.w[(unsigned)sw], valid, g, uu, nullptr);

  if (a.u_out && own) elem_rec_st_iterate(a.u_out + e0 * M + (unsigned)(x * M), uu);
  if constexpr (RES) {
    // ---- explicit residual r = b - A u of the element's rows (btd_elem_dict_kernel<M, true>'s), the record's words
    // from LDS ---------------------------------------------------------------------------------------------------------
    double D[M][M], sc[M];
    {
      double du[T];
#pragma unroll
      for (int k = 0; k < T; k += 2) elem_ld2(rec + kElemRecDup + k, du[k], du[k + 1]);
      const uint4 w4 = *reinterpret_cast<const uint4*>(rec + kElemRecCorr);
      const uint32_t w[M] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int j = 0; j < M; j += 2) elem_ld2(rec + kElemRecQmir + j, sc[j], sc[j + 1]);
      bool esc = false;
#pragma unroll
      for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
          if (j >= i) {
            D[i][j] = du[elem_tri<M>(i, j)];
          } else {
            const int d = (int)(int8_t)(w[i] >> (8 * j));
            D[i][j] = sym_residual_decode(du[elem_tri<M>(j, i)], d);
            esc |= d == kSymResidualEscape;
          }
        }
        const int dc = (int)(int8_t)(w[i] >> 24);
        sc[i] = sym_residual_decode(sc[i], dc);
        esc |= dc == kSymResidualEscape;
      }
      if (__builtin_expect(own && esc, 0)) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
          for (int j = 0; j < i; ++j)
            if ((int)(int8_t)(w[i] >> (8 * j)) == kSymResidualEscape) D[i][j] = a.lv.dblk[((int64_t)ce * M + i) * M + j];
          if ((int)(int8_t)(w[i] >> 24) == kSymResidualEscape) sc[i] = a.lv.scol[(int64_t)ce * M + i];
        }
      }
    }
    double rr[M];
    {
      const double um = cur[c_sub * S + x - 1];
      double up[M];
#pragma unroll
      for (int j = 0; j < M; ++j) up[j] = cur[j * S + x + 1];
      double dlo, dhi;
      elem_group_dot4(st.q, up, dlo, dhi);
#pragma unroll
      for (int i = 0; i < M; ++i) {
        double s = __fma_rn(sc[i], um, 0.0);
#pragma unroll
        for (int j = 0; j < M; ++j) s = __fma_rn(D[i][j], uu[j], s);   // (a valid element's uu is its words of cur)
        if (i == r_sup) s = __dadd_rn(s, i < 2 ? dlo : dhi);
        rr[i] = own ? __dadd_rn(bb[i], -s) : 0.0;
      }
    }
    // ---- restriction onto two coarse modes, through the (now free) iterate buffers, ascending fine row ----------------
    __syncthreads();
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double lx, ly;
      elem_ld2(rec + kElemRecLf + 2 * i, lx, ly);
      nxt[i * S + x] = own ? __dmul_rn(lx, rr[i]) : 0.0;
      cur[i * S + x] = own ? __dmul_rn(ly, rr[i]) : 0.0;
    }
    __syncthreads();
    const int rho = a.rho_out;
    const int ncoarse = a.owned / rho;   // owned coarse elements of this tile
    const int64_t J0 = fused_tile(a) * ncoarse;
    for (int k2 = x; k2 < ncoarse * 2; k2 += TE) {
      const int Jl = k2 >> 1, c = k2 & 1;
      const int64_t J = J0 + Jl;
      if (J >= a.nec_out) continue;
      const double* pr = (c ? cur : nxt) + a.halo_left + Jl * rho;
      double acc = 0.0;
      for (int k = 0; k < rho; ++k) {
#pragma unroll
        for (int j = 0; j < M; ++j) acc = __dadd_rn(acc, pr[j * S + k]);
      }
      a.rc_out[J * 2 + c] = acc;
    }
  }
}

// btd_elem_replay_up_kernel with the class table in LDS: the same conditions, and btd_elem_rec_kernel's on the table.
template <int M>
__global__ __launch_bounds__(kElemThreads) void btd_elem_rec_replay_up_kernel(FusedArgs a, SweepWeights wts, int npre, ElemRecTab t) {
  static_assert(M == 4, "the element-thread kernel's block size");
  constexpr int TE = kElemThreads;
  constexpr int S = TE + 2;            // words of one component in a buffer
  extern __shared__ double lds[];
  double* cur = lds + 1;               // (j, x) at cur[j * S + x]
  double* nxt = lds + M * S + 1;
  double* const tab = lds + 2 * M * S;

  const int x = threadIdx.x;
  const int64_t ne = a.lv.ne;
  const int64_t e0 = fused_tile(a) * a.owned - a.halo_left;   // element at x = 0
  const int own0 = a.halo_left, own1 = a.halo_left + a.owned;
  const int64_t rem = ne - 1 - e0;
  if (rem < 0) return;   // a tile wholly past the level: before any barrier
  const int xlo = e0 < 0 ? (int)-e0 : 0, xhi = rem < TE - 1 ? (int)rem : TE - 1;
  const bool valid = x >= xlo && x <= xhi;
  const bool own = valid && x >= own0 && x < own1;
  const unsigned xc = (unsigned)(x < xlo ? xlo : x > xhi ? xhi : x);

  // ---- loads, straight-line: the table, then cls, b, u_in, the coarse pair ------------------------------------------------
  elem_v2d tv[kElemRecStage];
  elem_rec_fetch(t, x, tv);
  unsigned ce = (a.lv.cls + e0)[xc];
  double bb[M], uu[M];
  {
    const double* const bp = a.b + e0 * M + xc * M;
    const double* const up = (a.u_in ? a.u_in : a.b) + e0 * M + xc * M;   // (no first iterate: b's line again, dropped)
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(bp + j, bb[j], bb[j + 1]);
#pragma unroll
    for (int j = 0; j < M; j += 2) elem_ld2(up + j, uu[j], uu[j + 1]);
  }
  double ucx, ucy;
  {
    const int64_t J = ne <= 0x7fffffff ? (int64_t)((unsigned)(e0 + xc) / (unsigned)a.rho_in) : (e0 + xc) / a.rho_in;
    elem_ld2(a.uc + J * 2, ucx, ucy);
  }
  elem_rec_store(tab, t, x, tv);
  if (x < 4 * M) {   // the zero elements at the ends of both buffers
    const int j = x & (M - 1), w = x / M;
    (w & 2 ? nxt : cur)[j * S + (w & 1 ? TE : -1)] = 0.0;
  }
  __syncthreads();
  elem_rec_pin_all<M>(ce, bb, uu, ucx, ucy);
  if (!a.u_in) {
#pragma unroll
    for (int j = 0; j < M; ++j) uu[j] = 0.0;
  }

  const double* const rec = tab + ce * kElemRecWords;
  // L uc of the element's rows: the second product rounded, the first fused into the sum
  double luc[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double lx, ly;
    elem_ld2(rec + kElemRecLf + 2 * j, lx, ly);
    luc[j] = __fma_rn(lx, ucx, __dmul_rn(ly, ucy));
  }
  if (!valid) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      uu[j] = 0.0;
      bb[j] = 0.0;
    }
  }
  double g[M];
  elem_rec_g<M>(rec, bb, g);
#pragma unroll
  for (int i = 0; i < M; ++i) cur[i * S + x] = uu[i];
  const int c_sub = a.lv.c_sub, r_sup = a.lv.r_sup;
  ElemRecStencil<M> st;
  st.load(rec, r_sup);   // held over the sweeps: re-reading per sweep measured 0.030 ms per cycle slower (r32)
  __syncthreads();

  // (the sweep placed three times, as in btd_elem_replay_up_kernel: the sweeps that add nothing carry no select for it)
  for (int sw = 0; sw < npre - 1; ++sw)
    elem_rec_sweep<M, false>(st, cur, nxt, x, c_sub, wts.w[(unsigned)sw], valid, g, uu, nullptr);
  elem_rec_sweep<M, true>(st, cur, nxt, x, c_sub, wts.w[(unsigned)(npre - 1)], valid, g, uu, luc);
  for (int sw = npre; sw < a.nsweeps; ++sw)
    elem_rec_sweep<M, false>(st, cur, nxt, x, c_sub, wts.w[(unsigned)sw], valid, g, uu, nullptr);

  if (own) elem_rec_st_iterate(a.u_out + e0 * M + (unsigned)(x * M), uu);
}

}  // namespace aggmg
