// The multiplicative two-colour element-patch sweeps (patch_gs_body, patch_kernels.hpp) on K columns
// in one pass over the operator (aggmg_smooth_multi_dev, and the patch levels of aggmg_vcycle_multi_dev under
// AGGMG_OPT_PATCH_MULTI).  One launch runs patch_gs_body's schedule -- per sweep the half-sweeps
// colour = h ^ reverse, each the residual rows of the tile, a barrier, the one patch solve per row, a barrier -- for
// kc <= KB columns at once: a row's operator words (its 4M inverse-row words, its M entries of D_e, its couplings) come
// from HBM, or from the smoother's dictionary by class (DICT), once and stay in the thread's registers while it walks the
// columns; every column has an iterate plane, updated in place, and a residual plane in LDS, each padded by one zero
// element a side (the planes of btd_multi_kernel); b and the row's current value per column stay in registers.
//
// Bitwise: a column's arithmetic is patch_gs_body's, operation for operation -- the same helpers (btd_apply_cmp<M, false>,
// btd_apply_dense<M>) in the same translation unit, the same 2M-term dot in ascending j, the same uu + w * y behind the
// same valid / with_prev / with_next guards.  The slot of the inverse rows a half-sweep applies is chosen once per
// half-sweep and not once per column: the same words.  The tile is one slab (256 / M elements) where patch_gs_body keeps
// several, which changes nothing: an owned element's sweeps see only values within the halo.  Plain C++ per row -- no
// atomics, no cross-lane operations.  Columns >= kc are neither read nor written.
//
// Instantiated for the forms the K-column transfer kernel (multi_kernels.hpp) covers: compressed couplings with M = 2, 4,
// dense ones with M = 2; KB = 1, 2, 4, 8.
#pragma once
#include "patch_kernels.hpp"

namespace aggmg {

struct PatchGsMultiArgs {
  PatchGsArgs g;   // column 0 of u_in, b, u_out; owned / halo of patch_gs_multi_tile_plan (host_plan.hpp)
  int64_t ld_uin, ld_b, ld_uout;   // column stride (doubles)
  int kc;          // columns of this launch (<= KB)
};

template <int M, bool CMP, int KB, bool DICT>
__global__ __launch_bounds__(kThreads) void patch_gs_multi_kernel(PatchGsMultiArgs ma, SweepWeights wts,
                                                                  const uint16_t* __restrict__ cls) {
  static_assert(M == 2 || M == 4, "the K-column transfer kernel's block sizes");
  static_assert(CMP || M == 2, "dense couplings: M = 2");
  const PatchGsArgs& g = ma.g;
  const PatchArgs& a = g.p;
  const int kc = ma.kc;
  constexpr int TE = kThreads / M;    // elements per tile (one slab, owned + halos)
  constexpr int PL = (TE + 2) * M;    // one column's padded plane: index x * M + j, x in [-1, TE]
  extern __shared__ double lds[];
  double* cur = lds + M;              // plane k: cur + k * PL
  double* res = lds + KB * PL + M;

  const int tid = threadIdx.x;
  const int x = tid / M;
  const int i = tid - x * M;
  const int64_t ne = a.ne;
  const int64_t e0 = (int64_t)blockIdx.x * a.owned - a.halo;   // element at x = 0
  const int64_t e = e0 + x;
  const bool valid = e >= 0 && e < ne;
  const int64_t row = e * M + i;

  if (tid < M) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      cur[k * PL - M + tid] = 0.0;
      cur[k * PL + TE * M + tid] = 0.0;
      res[k * PL - M + tid] = 0.0;
      res[k * PL + TE * M + tid] = 0.0;
    }
  }

  // ---- the row's operator words, once for all columns (DICT: from the dictionary) ----------------------------------------
  double dk[M], lo[CMP ? 1 : M], hi[M], z[4 * M];
  const int par = (int)(e & 1);
  const bool with_prev = valid && e >= 1;        // the patches {e - 1, e} and {e, e + 1} exist
  const bool with_next = valid && e <= ne - 2;
  const int c = (DICT && valid) ? (int)cls[e] : 0;
#pragma unroll
  for (int j = 0; j < M; ++j) dk[j] = hi[j] = 0.0;
#pragma unroll
  for (int j = 0; j < (CMP ? 1 : M); ++j) lo[j] = 0.0;
#pragma unroll
  for (int j = 0; j < 4 * M; ++j) z[j] = 0.0;
  if (valid) {
    if constexpr (DICT) {
      const int crow = c * M + i;   // the row in its class's record (c < kDictMaxClasses: 32-bit offsets)
      const double* zr = a.zrows + crow * (4 * M);
#pragma unroll
      for (int j = 0; j < 4 * M; ++j) z[j] = zr[j];
#pragma unroll
      for (int j = 0; j < M; ++j) dk[j] = a.dblk[crow * M + j];
      if constexpr (CMP) {
        lo[0] = a.scol[crow];
        if (i == a.r_sup) {
#pragma unroll
          for (int j = 0; j < M; ++j) hi[j] = a.qrow[c * M + j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) lo[j] = a.sub[crow * M + j];
#pragma unroll
        for (int j = 0; j < M; ++j) hi[j] = a.sup[crow * M + j];
      }
    } else {
      const double* zr = a.zrows + row * (4 * M);
#pragma unroll
      for (int j = 0; j < 4 * M; ++j) z[j] = AGGMG_LD(zr[j]);
#pragma unroll
      for (int j = 0; j < M; ++j) dk[j] = AGGMG_LD(a.dblk[row * M + j]);
      if constexpr (CMP) {
        lo[0] = AGGMG_LD(a.scol[row]);
        if (i == a.r_sup) {
#pragma unroll
          for (int j = 0; j < M; ++j) hi[j] = a.qrow[e * M + j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) lo[j] = AGGMG_LD(a.sub[row * M + j]);
#pragma unroll
        for (int j = 0; j < M; ++j) hi[j] = AGGMG_LD(a.sup[row * M + j]);
      }
    }
  }

  // ---- the columns' vectors ---------------------------------------------------------------------------------------------
  double bb[KB], uu[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    bb[k] = 0.0;
    uu[k] = 0.0;
    if (valid && k < kc) {
      bb[k] = a.b[k * ma.ld_b + row];
      if (a.u_in) uu[k] = a.u_in[k * ma.ld_uin + row];
    }
    cur[k * PL + x * M + i] = uu[k];
  }
  __syncthreads();

  for (int sw = 0; sw < a.nsweeps; ++sw) {
    const double w = wts.w[sw];   // this sweep's factor, for both of its halves: wave-uniform, a scalar load
    for (int h = 0; h < 2; ++h) {
      const int colour = h ^ g.reverse;
      // residual rows of the tile (zero outside the level), all columns per barrier
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        if (k < kc) {
          const double *um = cur + k * PL + (x - 1) * M, *ux = cur + k * PL + x * M, *up = cur + k * PL + (x + 1) * M;
          double t;
          if constexpr (CMP)
            t = btd_apply_cmp<M, false>(lo[0], dk, hi, um, ux, up, a.c_sub, a.r_sup, i);
          else
            t = btd_apply_dense<M>(lo, dk, hi, um, ux, up);
          res[k * PL + x * M + i] = valid ? bb[k] - t : 0.0;
        }
      }
      __syncthreads();
      // the one patch of this colour covering the row: the element is its first one (slot 1) or its second (slot 0)
      const bool first = par == colour;
      const bool covered = first ? with_next : with_prev;
      double zs[2 * M];
#pragma unroll
      for (int j = 0; j < 2 * M; ++j) zs[j] = first ? z[2 * M + j] : z[j];
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        if (k < kc) {
          const double* r = res + k * PL + (first ? x : x - 1) * M;
          double y = 0.0;
#pragma unroll
          for (int j = 0; j < 2 * M; ++j) y += zs[j] * r[j];
          if (covered) {
            uu[k] = uu[k] + w * y;
            cur[k * PL + x * M + i] = uu[k];
          }
        }
      }
      __syncthreads();
    }
  }

  if (valid && x >= a.halo && x < a.halo + a.owned) {
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < kc) AGGMG_ST(a.u_out[k * ma.ld_uout + row], uu[k]);
  }
}

}  // namespace aggmg
