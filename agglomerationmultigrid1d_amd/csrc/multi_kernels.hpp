// K right-hand sides in one pass over a level's operator (aggmg_vcycle_multi_dev; EXTENSION: the reference's
// multigrid_v_cycle / ldiv! take vectors, src/solvers.jl:19,63,84).  One launch runs btd_fused_kernel's schedule --
// descent: [x0 | zero] -> nsweeps block-Jacobi sweeps -> explicit residual -> restriction; ascent: prolong-add ->
// nsweeps sweeps -- for KB columns at once: every element's operator entries come from HBM once and stay in the
// thread's registers while it walks the columns; the KB iterates ping-pong in LDS, one plane per column.
//
// Bitwise: a column's arithmetic is btd_fused_kernel's -- the per-element helpers of kernels.hpp (btd_group_apply,
// btd_dsym_pq, btd_stencil_*, btd_damped, btd_apply_*, btd_prolong2) are called by both kernels, in the same order, in
// the same translation unit (aggmg_hip.hip, one set of compiler flags).  Tiles cut the level differently (one slab per
// thread here), which changes nothing: an owned element's sweeps see only the halo's values, every restricted coarse
// element lies inside one tile and sums its fine rows in ascending order.  The explicit residual reads the operator's
// full entry arrays where the single-column launch may read their lossless symmetric form: the same values.
//
// Coverage (multi_level_ok in aggmg_hip.hip decides; everything else runs column by column): block-Jacobi sweeps,
// compressed couplings with M = 2, 4 (lane groups) or dense ones with M = 2, symmetric-packed or not, two-mode
// transfers with one agglomeration ratio (TransferBtd::rho > 0, mc = 2), the explicit restriction.
#pragma once
#include "kernels.hpp"

namespace aggmg {

struct MultiArgs {
  FusedArgs a;  // column 0 of every vector (FusedArgs::u_in, b, u_out, uc, rc_out), tiling, level, transfer
  // column stride (doubles) of u_in, b, u_out, uc, rc_out
  int64_t ld_uin, ld_b, ld_uout, ld_uc, ld_rc;
  int kc;       // columns of this launch (<= KB; the rest of the KB are neither read nor written)
};

template <int M, bool CMP, bool SYM, int KB, int NT>
__global__ __launch_bounds__(NT) void btd_multi_kernel(MultiArgs ma, SweepWeights wts) {
  static_assert(M == 2 || M == 4, "lane-group path only");
  static_assert(CMP || M == 2, "dense couplings: M = 2");
  constexpr bool GRP = CMP;
  constexpr bool DSYM = !CMP && SYM;
  constexpr int TE = NT / M;            // elements per tile (one slab)
  constexpr int PL = (TE + 2) * M;      // one column's iterate plane, padded by one zero element on both sides
  const FusedArgs& a = ma.a;
  const int kc = ma.kc;
  extern __shared__ double lds[];
  double* buf0 = lds + M;               // plane k: buf0 + k * PL, index (x * M + j), x in [-1, TE]
  double* buf1 = lds + KB * PL + M;

  const int tid = threadIdx.x;
  const int x = tid / M;
  const int i = tid - x * M;
  const int64_t ne = a.lv.ne;
  const int64_t e0 = (int64_t)blockIdx.x * a.owned - a.halo_left;
  const int own0 = a.halo_left, own1 = a.halo_left + a.owned;
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

  // ---- the element's operator rows, once for all columns --------------------------------------
  const bool need_g = a.nsweeps > 0;
  const bool pre2 = a.do_residual && a.lf_out && a.mc_out == 2;
  double bi[M], Pr[M], Qr[M];
  double pc = 0.0, qv[1] = {0.0}, l2x = 0.0, l2y = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    bi[j] = 0.0;
    Pr[j] = 0.0;
    Qr[j] = 0.0;
  }
  if (valid) {
    if (need_g) {
      if (SYM) {
        constexpr int T = M * (M + 1) / 2;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const int lo_ = i < j ? i : j, hi_ = i < j ? j : i;
          bi[j] = a.lv.bsym[e * T + lo_ * M - (lo_ * (lo_ - 1)) / 2 + (hi_ - lo_)];
        }
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) bi[j] = AGGMG_LD(a.lv.binv[row * M + j]);
      }
    }
    if (pre2) {
      if (a.lf1_out) {
        l2x = 1.0;
        l2y = AGGMG_LD(a.lf1_out[row]);
      } else {
        const double2 t2 = *reinterpret_cast<const double2*>(a.lf_out + row * 2);
        l2x = t2.x;
        l2y = t2.y;
      }
    }
    if (CMP) {
      if (SYM)
        pc = (need_g && e > 0) ? a.lv.qrow[(e - 1) * M + i] : 0.0;  // q_{e-1}[i]; B^{-1} applied below
      else
        pc = need_g ? AGGMG_LD(a.lv.pcol[row]) : 0.0;
      qv[0] = AGGMG_LD(a.lv.qrow[e * M + i]);
    } else if (DSYM) {
#pragma unroll
      for (int j = 0; j < M; ++j) {
        Pr[j] = (need_g && e > 0) ? a.lv.sup[(row - M) * M + j] : 0.0;
        Qr[j] = need_g ? a.lv.sup[row * M + j] : 0.0;
      }
    } else {
#pragma unroll
      for (int j = 0; j < M; ++j) {
        Pr[j] = need_g ? AGGMG_LD(a.lv.P[row * M + j]) : 0.0;
        Qr[j] = need_g ? AGGMG_LD(a.lv.Q[row * M + j]) : 0.0;
      }
    }
  }
  double binv_r = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j)
    if (j == a.lv.r_sup) binv_r = bi[j];
  // prolongation rows (two coarse modes, one agglomeration ratio)
  double2 l2in = make_double2(0.0, 0.0);
  int64_t J = 0;
  if (valid && a.lf_in) {
    J = e / a.rho_in;
    if (a.lf1_in) {
      l2in.x = 1.0;
      l2in.y = AGGMG_LD(a.lf1_in[row]);
    } else {
      typedef double v2d __attribute__((ext_vector_type(2)));
      const v2d lv2 = AGGMG_LD(*reinterpret_cast<const v2d*>(a.lf_in + row * 2));
      l2in.x = lv2.x;
      l2in.y = lv2.y;
    }
  }

  // ---- the columns' vectors ------------------------------------------------------------------
  double bb[KB], uu[KB], g[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    uu[k] = 0.0;
    bb[k] = 0.0;
    if (valid && k < kc) {
      bb[k] = a.b[k * ma.ld_b + row];
      if (a.u_in) uu[k] = a.u_in[k * ma.ld_uin + row];
      if (a.lf_in) {
        const double2 u2 = *reinterpret_cast<const double2*>(a.uc + k * ma.ld_uc + J * 2);
        uu[k] += btd_prolong2(l2in, u2);
      }
    }
    buf0[k * PL + x * M + i] = uu[k];
  }
#pragma unroll
  for (int k = 0; k < KB; ++k) g[k] = btd_group_apply<M>(bi, bb[k]);
  if (DSYM) btd_dsym_pq<M>(bi, Pr, Qr);
  if (SYM && CMP) pc = btd_group_apply<M>(bi, pc);  // pcol = B^{-1} q_{e-1}
  __syncthreads();

  // ---- sweeps: all columns per barrier -------------------------------------------------------
  double* cur = buf0;
  double* nxt = buf1;
  for (int sw = 0; sw < a.nsweeps; ++sw) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const double* um = cur + k * PL + (x - 1) * M;
      const double* up = cur + k * PL + (x + 1) * M;
      double acc;
      if (CMP)
        acc = btd_stencil_cmp<M, GRP>(g[k], pc, qv, binv_r, um, up, a.lv.c_sub, i);
      else
        acc = btd_stencil_dense<M>(g[k], Pr, Qr, um, up);
      double un = btd_damped(uu[k], wts.w[sw], acc);
      if (!valid) un = 0.0;
      uu[k] = un;
      nxt[k * PL + x * M + i] = un;
    }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  }

  // ---- the owned elements' iterates ----------------------------------------------------------
  const bool own = valid && x >= own0 && x < own1;
  if (a.u_out && own) {
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < kc) AGGMG_ST(a.u_out[k * ma.ld_uout + row], uu[k]);
  }
  if (!a.do_residual) return;

  // ---- explicit residual r = b - A u of the owned elements, the row's entries read once -------
  double rr[KB];
  {
    double dk[M], sc = 0.0, sb[M], sp[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      dk[j] = 0.0;
      sb[j] = 0.0;
      sp[j] = 0.0;
    }
    if (own) {
      if (CMP) {
        sc = a.lv.scol[row];
#pragma unroll
        for (int j = 0; j < M; ++j) dk[j] = a.lv.dblk[row * M + j];
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) {
          sb[j] = a.lv.sub[row * M + j];
          dk[j] = a.lv.dblk[row * M + j];
          sp[j] = a.lv.sup[row * M + j];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const double* um = cur + k * PL + (x - 1) * M;
      const double* ux = cur + k * PL + x * M;
      const double* up = cur + k * PL + (x + 1) * M;
      double t;
      if (CMP)
        t = btd_apply_cmp<M, GRP>(sc, dk, qv, um, ux, up, a.lv.c_sub, a.lv.r_sup, i);
      else
        t = btd_apply_dense<M>(sb, dk, sp, um, ux, up);
      rr[k] = own ? bb[k] - t : 0.0;
    }
  }
  if (!pre2) return;

  // ---- restriction, two coarse modes: the row products through LDS, one thread per (column, J, mode) ----
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    nxt[k * PL + x * M + i] = own ? l2x * rr[k] : 0.0;
    cur[k * PL + x * M + i] = own ? l2y * rr[k] : 0.0;
  }
  __syncthreads();
  const int rho = a.rho_out;
  const int ncoarse = a.owned / rho;
  const int64_t J0 = ((int64_t)blockIdx.x * a.owned) / rho;
  const int64_t nec = ne / rho;
  for (int t = tid; t < kc * ncoarse * 2; t += NT) {
    const int k = t / (ncoarse * 2);
    const int r = t - k * ncoarse * 2;
    const int Jl = r >> 1, c = r & 1;
    const int64_t Jc = J0 + Jl;
    if (Jc >= nec) continue;
    const double* pr = (c ? cur : nxt) + k * PL + (a.halo_left + Jl * rho) * M;
    double acc = 0.0;
    for (int q = 0; q < rho * M; ++q) acc += pr[q];  // ascending fine row, as the column dot of L'
    a.rc_out[k * ma.ld_rc + Jc * 2 + c] = acc;
  }
}

}  // namespace aggmg
