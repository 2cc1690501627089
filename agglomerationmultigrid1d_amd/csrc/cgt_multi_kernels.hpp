// The fused point-Jacobi schedule of the chain kernel (cgt_fused_kernel<M, 1, 256, 0>, cgt_kernels.hpp) on K columns in one
// pass over the operator (the chain levels of aggmg_vcycle_multi_dev under AGGMG_OPT_CHAIN_MULTI):
//     [u += L uc]  ->  S sweeps  u += w_s * (b - A u) / diag(A)  ->  [r = b - A u  ->  rc = L' r]
// for kc <= KB columns at once.  One thread per row of a block, lane groups of M.  A thread loads its row's operator words
// -- dblk[row][0 .. M), supcol[row], subrow[row], the diagonal --, forms its caller-side index (affine, or from perm), its
// row of the prolongation and the coarse indices behind it (cperm included) ONCE, from the full arrays or by class (DICT:
// the tile's classes also sit in LDS for the restriction, as in cgt_fused_kernel), and then walks the columns: b and the
// row's current value of every column stay in registers, every column has an iterate plane per ping-pong buffer in LDS,
// padded by one zero block a side, and a sweep has one barrier for all columns.  The restriction stages every column's
// residual through the free planes and sums one (column, coarse DoF) per thread.  Column j of a vector lies at
// base + j * ld; columns >= kc are neither read nor written.
//
// Bitwise: a column's arithmetic is cgt_fused_kernel's, operation for operation -- the row product in row_Au's order
// (the cross-lane sum of sr * um[i] kept on lane 0, + d[0] ux[0], + sup up[0], then j = 1 .. M - 1), the update
// uu + w * ((b - A u) / dg) behind the same `valid` guard, the prolongation sums in the same order and the same form per
// block size (the batched one, which adds 0 * 0 for a skipped entry, at M >= 4; the skipping loop below), the restriction
// sums in the same order.  The tile is one slab, as the single-column default; tile shapes do not enter the bits: an owned
// block's sweeps see only values within the halo, and every coarse DoF is summed by one thread in a fixed order.  No
// atomics, no scratch.
#pragma once
#include "cgt_kernels.hpp"

namespace aggmg {

struct CgtMultiArgs {
  CgtArgs a;   // column 0 of u_in, b, u_out, uc, rc_out (r_out and the checkpoint fields are not used); owned / halo_left of
               // chain_multi_tile_plan (host_plan.hpp)
  int kc;      // columns of this launch (<= KB)
  int64_t ld_uin, ld_b, ld_uout, ld_uc, ld_rc;   // column strides (doubles)
};

template <int M, int KB, int NT, bool DICT>
__global__ __launch_bounds__(NT) void cgt_multi_kernel(CgtMultiArgs ma, SweepWeights wts) {
  static_assert(M == 1 || M == 2 || M == 4, "lane groups of 1, 2 or 4 rows");
  static_assert(NT % M == 0 && (KB == 1 || KB == 2 || KB == 4 || KB == 8), "column groups of 1, 2, 4 or 8");
  const CgtArgs& a = ma.a;
  const int kc = ma.kc;
  constexpr int TE = NT / M;          // blocks per tile (one slab, owned + halos)
  constexpr int PL = (TE + 2) * M;    // one column's padded plane: index x * M + j, x in [-1, TE]
  extern __shared__ double lds[];
  double* const buf0 = lds + M;       // plane k of a buffer: + k * PL
  double* const buf1 = lds + KB * PL + M;
  // DICT: class of block x of the tile at lcls[x], x in [-1, TE] (the launch reserves TE + 2 entries behind the planes)
  [[maybe_unused]] uint16_t* lcls = reinterpret_cast<uint16_t*>(lds + 2 * KB * PL) + 1;

  const int tid = threadIdx.x;
  const int x = tid / M;
  const int i = tid - x * M;
  const int64_t ne = a.lv.ne;
  const int64_t e0 = (int64_t)blockIdx.x * a.owned - a.halo_left;   // block at x = 0
  const int64_t e = e0 + x;
  const bool valid = e >= 0 && e < ne;
  const int64_t row = e * M + i;

  if (tid < M) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      buf0[k * PL - M + tid] = 0.0;
      buf0[k * PL + TE * M + tid] = 0.0;
      buf1[k * PL - M + tid] = 0.0;
      buf1[k * PL + TE * M + tid] = 0.0;
    }
  }

  // ---- load phase: the row's operator record, its indices, b and the starting value of every column ------------------
  [[maybe_unused]] int ce = 0;
  if constexpr (DICT) {
    ce = valid ? (int)a.cls[e] : 0;
    if (tid == 0) {
      lcls[-1] = 0;
      lcls[TE] = 0;
    }
    if (i == 0) lcls[x] = (uint16_t)ce;
  }
  // the operator's record: the block's own, or (DICT) its class's in the dictionary
  const int64_t oe = DICT ? (int64_t)ce : e;
  const int64_t orow = DICT ? (int64_t)(ce * M + i) : row;
  double d[M], sup = 0.0, sr = 0.0, dg = 1.0, bb[KB], uu[KB];
  int32_t pr = -1;
#pragma unroll
  for (int j = 0; j < M; ++j) d[j] = 0.0;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    bb[k] = 0.0;
    uu[k] = 0.0;
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < M; ++j) d[j] = AGGMG_LD(a.lv.dblk[orow * M + j]);
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (j == i) dg = d[j];
    sup = AGGMG_LD(a.lv.supcol[orow]);
    sr = AGGMG_LD(a.lv.subrow[orow]);   // entry i of the block's sub-diagonal row
    if (a.ext) {
      if (a.affine)
        pr = i == 0 ? (int32_t)e : (e == ne - 1 ? -1 : (int32_t)(ne + e * (M - 1) + (i - 1)));
      else
        pr = a.perm[row];
    }
    const int64_t rb = (a.ext & kExtB) ? (int64_t)pr : row;
    if (rb >= 0) {
#pragma unroll
      for (int k = 0; k < KB; ++k)
        if (k < kc) bb[k] = a.b[rb + k * ma.ld_b];
    }
    if (a.u_in) {
      const int64_t ru = (a.ext & kExtUin) ? (int64_t)pr : row;
      if (ru >= 0) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
          if (k < kc) uu[k] = a.u_in[ru + k * ma.ld_uin];
      }
    }
    if (a.tin.type == kTrChain) {
      const int mc = a.tin.mc;
      const double* lr = a.tin.l + orow * (mc + 1);
      // coarse entry c of the row: DoF c of coarse block e, the last one DoF 0 of block e + 1; -1: none
      auto coarse_index = [&](int c) -> int64_t {
        const int64_t cb = c < mc ? e * mc + c : (e + 1) * mc;
        if (cb >= a.tin.nec * mc) return -1;
        return a.tin.cperm ? (int64_t)a.tin.cperm[cb] : cb;
      };
      // the row's mc + 1 entries and coarse indices once, the products column by column.  BATCH: cgt_fused_kernel's
      // batched form (M >= 4; a skipped entry adds 0.0 * 0.0); otherwise its loop, which skips the entry
      auto held = [&](auto cmax_tag, auto batch_tag) {
        constexpr int CMAX = decltype(cmax_tag)::value;
        constexpr bool BATCH = decltype(batch_tag)::value;
        double lv[CMAX + 1];
        int64_t ci[CMAX + 1];
#pragma unroll
        for (int c = 0; c <= CMAX; ++c) {
          lv[c] = 0.0;
          ci[c] = -1;
          if (c <= mc) {
            ci[c] = coarse_index(c);
            if (ci[c] >= 0) lv[c] = lr[c];
          }
        }
#pragma unroll
        for (int k = 0; k < KB; ++k)
          if (k < kc) {
            const double* uc = a.uc + k * ma.ld_uc;
            double uv[CMAX + 1];
#pragma unroll
            for (int c = 0; c <= CMAX; ++c) uv[c] = ci[c] >= 0 ? uc[ci[c]] : 0.0;
            double add = 0.0;
#pragma unroll
            for (int c = 0; c <= CMAX; ++c)
              if (c <= mc && (BATCH || ci[c] >= 0)) add += lv[c] * uv[c];
            uu[k] += add;
          }
      };
      if (M >= 4 && mc <= 2) {
        held(std::integral_constant<int, 2>(), std::true_type());
      } else if (M >= 4 && mc <= kCgtMaxMcUnrolled) {
        held(std::integral_constant<int, kCgtMaxMcUnrolled>(), std::true_type());
      } else if (M < 4 && mc <= 2) {
        held(std::integral_constant<int, 2>(), std::false_type());
      } else {   // wider coarse blocks: the loop as it is, column by column
#pragma unroll
        for (int k = 0; k < KB; ++k)
          if (k < kc) {
            const double* uc = a.uc + k * ma.ld_uc;
            double add = 0.0;
            for (int c = 0; c <= mc; ++c) {
              const int64_t ci = coarse_index(c);
              if (ci >= 0) add += lr[c] * uc[ci];
            }
            uu[k] += add;
          }
      }
    } else if (a.tin.type == kTrAgg) {
      const int mc = a.tin.mc;
      const int64_t J = e / a.tin.rho;
      const bool prev = i == 0 && J >= 1 && e == J * a.tin.rho;   // the vertex row of a block that starts an agglomerate
      const bool own = J < a.tin.nec;
      const double* lpr = a.tin.lp + oe * mc;
      const double* lr = a.tin.l + orow * mc;
      auto held = [&](auto cmax_tag) {
        constexpr int CMAX = decltype(cmax_tag)::value;
        double lpv[CMAX], lv[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          lpv[c] = (prev && c < mc) ? lpr[c] : 0.0;
          lv[c] = (own && c < mc) ? lr[c] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < KB; ++k)
          if (k < kc) {
            const double* uc = a.uc + k * ma.ld_uc;
            double add = 0.0;
            if (prev) {
#pragma unroll
              for (int c = 0; c < CMAX; ++c)
                if (c < mc) add += lpv[c] * uc[(J - 1) * mc + c];
            }
            if (own) {
#pragma unroll
              for (int c = 0; c < CMAX; ++c)
                if (c < mc) add += lv[c] * uc[J * mc + c];
            }
            uu[k] += add;
          }
      };
      if (mc <= 2) {
        held(std::integral_constant<int, 2>());
      } else {   // wider coarse blocks: column by column
#pragma unroll
        for (int k = 0; k < KB; ++k)
          if (k < kc) {
            const double* uc = a.uc + k * ma.ld_uc;
            double add = 0.0;
            if (prev)
              for (int c = 0; c < mc; ++c) add += lpr[c] * uc[(J - 1) * mc + c];
            if (own)
              for (int c = 0; c < mc; ++c) add += lr[c] * uc[J * mc + c];
            uu[k] += add;
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < kc) buf0[k * PL + x * M + i] = uu[k];
  __syncthreads();

  // A u for this thread's row out of the column's LDS plane, in row_Au's order
  auto row_Au = [&](const double* cur) -> double {
    const double* um = cur + (x - 1) * M;
    const double* ux = cur + x * M;
    const double* up = cur + (x + 1) * M;
    double t = group_sum<M>(sr * um[i]);
    if (i != 0) t = 0.0;
    t += d[0] * ux[0];
    t += sup * up[0];
#pragma unroll
    for (int j = 1; j < M; ++j) t += d[j] * ux[j];
    return t;
  };

  // ---- sweeps: u <- u + w * ((b - A u) / diag), every column, one barrier per sweep ----------------------------------
  double* cur = buf0;
  double* nxt = buf1;
  for (int sw = 0; sw < a.nsweeps; ++sw) {
    const double wsw = wts.w[(unsigned)sw];
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < kc) {
        const double r = bb[k] - row_Au(cur + k * PL);
        const double y = r / dg;
        double un = uu[k] + wsw * y;
        if (!valid) un = 0.0;
        uu[k] = un;
        nxt[k * PL + x * M + i] = un;
      }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  }

  // ---- store the iterate of the owned blocks ----------------------------------------------------------------------
  const int xo0 = a.halo_left, xo1 = a.halo_left + a.owned;
  if (a.u_out && valid && x >= xo0 && x < xo1) {
    const int64_t ro = (a.ext & kExtUout) ? (int64_t)pr : row;
    if (ro >= 0) {
#pragma unroll
      for (int k = 0; k < KB; ++k)
        if (k < kc) AGGMG_ST(a.u_out[ro + k * ma.ld_uout], uu[k]);
    }
  }
  if (!a.do_residual) return;

  // ---- residual r = b - A u: owned blocks, plus the one block whose rows the restriction of an owned coarse block also
  // touches (chain: the block on the left, agg: the vertex on the right); staged through the free planes ----------------
  const int xr0 = xo0 - (a.tout.type == kTrChain ? 1 : 0);
  const int xr1 = xo1 + (a.tout.type == kTrAgg ? 1 : 0);
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < kc) {
      const double t = row_Au(cur + k * PL);   // every lane of a group takes part in the cross-lane sum
      double rr = 0.0;
      if (valid && x >= xr0 && x < xr1) rr = bb[k] - t;
      nxt[k * PL + x * M + i] = rr;
    }
  if (a.tout.type == kTrNone) return;
  __syncthreads();

  // ---- restriction rc = L' r: one thread per (column, owned coarse DoF) -------------------------------------------------
  const int mc = a.tout.mc;
  if (a.tout.type == kTrChain) {
    const double* L = a.tout.l;
    const int w = mc + 1;
    const int per = a.owned * mc;
    for (int t = tid; t < kc * per; t += NT) {
      const int k = t / per, tt = t - k * per;
      const int xl = tt / mc, c = tt - xl * mc;
      const int xb = xo0 + xl;
      const int64_t J = e0 + xb;  // coarse block = fine block
      if (J >= ne || J >= a.tout.nec) continue;
      const double* rs = nxt + k * PL;
      // the rows of L of block J and of block J - 1: the blocks' own, or (DICT) their classes' in the dictionary
      const int64_t rowb = DICT ? (int64_t)lcls[xb] * M : J * M;
      const int64_t rowl = DICT ? (int64_t)lcls[xb - 1] * M : rowb - M;
      // ascending fine row of the reference numbering: own vertex, the left element's rows, own interior
      double acc = L[rowb * w + c] * rs[xb * M];
      if (c == 0 && J > 0)
        for (int q = 0; q < M; ++q) acc += L[(rowl + q) * w + mc] * rs[(xb - 1) * M + q];
      for (int q = 1; q < M; ++q) acc += L[(rowb + q) * w + c] * rs[xb * M + q];
      const int64_t cb = J * mc + c;
      const int64_t ci = a.tout.cperm ? (int64_t)a.tout.cperm[cb] : cb;
      if (ci >= 0) a.rc_out[ci + k * ma.ld_rc] = acc;
    }
  } else {
    const int rho = a.tout.rho;
    const int ncoarse = a.owned / rho;
    const int64_t J0 = ((int64_t)blockIdx.x * a.owned) / rho;
    const int per = ncoarse * mc;
    for (int t = tid; t < kc * per; t += NT) {
      const int k = t / per, tt = t - k * per;
      const int Jl = tt / mc, c = tt - Jl * mc;
      const int64_t J = J0 + Jl;
      if (J >= a.tout.nec) continue;
      const double* rs = nxt + k * PL;
      const int xb = xo0 + Jl * rho;
      [[maybe_unused]] const int64_t rowb = (e0 + xb) * (int64_t)M;
      double acc = 0.0;
      if constexpr (DICT) {
        for (int q = 0; q < rho; ++q) {   // (the same rows in the same order, block by block through the classes)
          const int64_t rq = (int64_t)lcls[xb + q] * M;
          for (int j = 0; j < M; ++j) acc += a.tout.l[(rq + j) * mc + c] * rs[(xb + q) * M + j];
        }
      } else {
        for (int q = 0; q < rho * M; ++q) acc += a.tout.l[(rowb + q) * mc + c] * rs[xb * M + q];
      }
      // the vertex that closes the agglomerate on the right belongs to the next fine block
      const int64_t en = (J + 1) * rho;
      if (en < ne) acc += a.tout.lp[(DICT ? (int64_t)lcls[xb + rho] : en) * mc + c] * rs[(xb + rho) * M];
      a.rc_out[J * mc + c + k * ma.ld_rc] = acc;
    }
  }
}

}  // namespace aggmg
