// The hybrid / additive element-patch Schwarz sweeps (patch_sweep_kernel / patch_sweep_dict_kernel, patch_kernels.hpp;
// DESIGN.md section 19) on K columns in one pass over the operator (aggmg_smooth_multi_dev, and the hybrid patch levels of
// aggmg_vcycle_multi_dev under AGGMG_OPT_PATCH_SCHWARZ_MULTI).  One launch runs patch_sweep_kernel's
// schedule -- per sweep the residual rows of the tile, a barrier, the two patch solves covering the row (patch e - 1
// first), the halving on inner elements (HYB), the weight, the update, a barrier -- for kc <= KB columns at once: a row's
// operator words (its 4M inverse-row words, its M entries of D_e, its couplings) come from HBM, or from the smoother's
// dictionary by class (DICT), once and stay in the thread's registers while it walks the columns; b and the row's
// current value per column stay in registers.
//
// LDS: per column an iterate plane and a residual plane, each padded by one zero element a side (patch_gs_multi_kernel's
// layout), 2 KB (TE + 2) M doubles.  patch_sweep_kernel keeps two iterate planes and swaps them; here the iterate is
// updated in place, which reads and writes the same values: a row's update reads the residual plane and its own
// register value only, and the barrier behind it stands before the next residual reads the plane.
//
// Bitwise: a column's arithmetic is patch_sweep_kernel's, operation for operation.  The residual goes through the same
// helpers (btd_apply_cmp<M, false>, btd_apply_dense<M>) in the same translation unit.  The patch solves and the update
// are written with the roundings patch_sweep_kernel is compiled to (contraction is on there), said explicitly: each dot
// product is 2M fused multiply-adds in ascending j, the first onto 0.0; the two are added as (0.0 + ya) + yb (0.0 + ya is
// ya bit for bit -- such a chain from +0.0 is never -0.0 -- and the compiler keeps it at M = 4 and drops it at M = 2), halved
// where HYB says so, and the weight and the iterate go into one more fused multiply-add, fma(w, v, u) -- the product
// w * v is never rounded on its own (patch_schwarz_solve below; DESIGN.md section 25 has the instruction counts this was
// read from).  The tile is one slab (256 / M elements) where patch_sweep_kernel keeps several, which changes nothing: an
// owned element's sweeps see only values within the halo.  Plain C++ per row -- no atomics, no cross-lane operations.
// Columns >= kc are neither read nor written.
//
// Instantiated for the forms the K-column transfer kernel (multi_kernels.hpp) covers: compressed couplings with M = 2, 4,
// dense ones with M = 2; KB = 1, 2, 4, 8; HYB and DICT both ways.
#pragma once
#include "patch_kernels.hpp"

namespace aggmg {

struct PatchSchwarzMultiArgs {
  PatchArgs p;     // column 0 of u_in, b, u_out; owned / halo of patch_schwarz_multi_tile_plan (host_plan.hpp)
  int64_t ld_uin, ld_b, ld_uout;   // column stride (doubles)
  int kc;          // columns of this launch (<= KB)
};

// (Z r)[row] over one patch: 2M terms in ascending j, as patch_sweep_kernel's `y = 0.0; y += z[j] * r[j]` is compiled --
// every term a fused multiply-add, the first one onto 0.0
template <int M>
__device__ __forceinline__ double patch_schwarz_solve(const double* z, const double* r) {
  double y = 0.0;
#pragma unroll
  for (int j = 0; j < 2 * M; ++j) y = __fma_rn(z[j], r[j], y);
  return y;
}

template <int M, bool CMP, int KB, bool HYB, bool DICT>
__global__ __launch_bounds__(kThreads) void patch_sweep_multi_kernel(PatchSchwarzMultiArgs ma, SweepWeights wts,
                                                                     const uint16_t* __restrict__ cls) {
  static_assert(M == 2 || M == 4, "the K-column transfer kernel's block sizes");
  static_assert(CMP || M == 2, "dense couplings: M = 2");
  const PatchArgs& a = ma.p;
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
  const bool inner = e > 0 && e < ne - 1;
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
    const double w = wts.w[sw];   // this sweep's factor: wave-uniform, a scalar load
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
    // the two patch solves covering the row, patch e - 1 first; the iterate plane in place (the residual plane is all a
    // row reads here)
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if (k < kc) {
        const double *ra = res + k * PL + (x - 1) * M, *rb = res + k * PL + x * M;
        const double ya = patch_schwarz_solve<M>(z, ra);
        const double yb = patch_schwarz_solve<M>(z + 2 * M, rb);
        double v = __dadd_rn(__dadd_rn(0.0, ya), yb);   // v = 0.0; v += ya; v += yb
        if (HYB && inner) v = __dmul_rn(v, 0.5);        // c_e = 2: the division, exactly
        const double un = valid ? __fma_rn(w, v, uu[k]) : 0.0;   // uu + w * v, contracted
        uu[k] = un;
        cur[k * PL + x * M + i] = un;
      }
    }
    __syncthreads();
  }

  if (valid && x >= a.halo && x < a.halo + a.owned) {
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < kc) AGGMG_ST(a.u_out[k * ma.ld_uout + row], uu[k]);
  }
}

}  // namespace aggmg
