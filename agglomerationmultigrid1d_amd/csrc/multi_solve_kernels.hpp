// What the outer solver loops do around the K-column cycle, on N x K column-major matrices (aggmg_pcg_multi_dev,
// aggmg_multigrid_multi_dev; EXTENSION: the reference's solvers take vectors, src/solvers.jl:116-139): the operator
// apply / residual, the column dots and norms, the conjugate-gradient updates.  Column j of every result is bit for bit
// what the single-vector kernel gives on column j:
//   btd_residual_multi_kernel   aggmg_residual_dev's launch (btd_fused_kernel, no sweeps, do_residual, r_out)
//   dot_cols_* / diff2_cols_*   dot_partial_kernel / diff2_partial_kernel + dot_final_kernel
//   pcg_xr_cols / pcg_p_cols    pcg_xr_kernel / pcg_p_kernel
// The residual row is btd_apply_cmp / btd_apply_dense of kernels.hpp -- the helpers btd_fused_kernel calls, in the same
// translation unit.  The vector kernels' multiply-adds are written as __fma_rn: the single-column kernels' `acc += x * y`
// forms are contracted to fma by the compiler (checked in the assembly), and whether it does so depends on the code around
// them, so the kernels that must agree say it.
#pragma once
#include "kernels.hpp"

namespace aggmg {

struct ResMultiArgs {
  BtdLevel lv;
  const double* x;   // column 0 of X
  const double* b;   // column 0 of B, or null: R = -A X (the bits of a zero B: 0.0 - (A x)_row)
  double* r;         // column 0 of R
  int64_t ld_x, ld_b, ld_r;
  int kc;            // columns of this launch (<= KB)
  int owned;         // owned elements per tile: NT / M - 2 (one element of halo on each side)
};

// R[:, k] = B[:, k] - A X[:, k], k < kc <= KB: one thread per DoF row, the row's operator entries loaded once into
// registers, the columns' u planes (one element of halo, zero pads beyond) in LDS.
template <int M, bool CMP, int KB, int NT>
__global__ __launch_bounds__(NT) void btd_residual_multi_kernel(ResMultiArgs a) {
  static_assert(M == 2 || M == 4, "lane-group path only");
  static_assert(CMP || M == 2, "dense couplings: M = 2");
  constexpr bool GRP = CMP;
  constexpr int TE = NT / M;            // elements per tile
  constexpr int PL = (TE + 2) * M;      // one column's plane, padded by one zero element on both sides
  extern __shared__ double lds[];
  double* buf = lds + M;                // plane k: buf + k * PL, index (x * M + j), x in [-1, TE]

  const int tid = threadIdx.x;
  const int x = tid / M;
  const int i = tid - x * M;
  const int kc = a.kc;
  const int64_t ne = a.lv.ne;
  const int64_t e = (int64_t)blockIdx.x * a.owned - 1 + x;
  const bool valid = e >= 0 && e < ne;
  const bool own = valid && x >= 1 && x < 1 + a.owned;
  const int64_t row = e * M + i;

  if (tid < M) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      buf[k * PL - M + tid] = 0.0;
      buf[k * PL + TE * M + tid] = 0.0;
    }
  }

  // ---- the row's entries, once for all columns ------------------------------------------------
  double dk[M], sb[M], sp[M];
  double sc = 0.0, qv[1] = {0.0};
#pragma unroll
  for (int j = 0; j < M; ++j) {
    dk[j] = 0.0;
    sb[j] = 0.0;
    sp[j] = 0.0;
  }
  if (own) {
    if (CMP) {
      qv[0] = AGGMG_LD(a.lv.qrow[e * M + i]);
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

  // ---- the columns' vectors -------------------------------------------------------------------
  double bb[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    double u = 0.0;
    bb[k] = 0.0;
    if (valid && k < kc) {
      u = a.x[k * a.ld_x + row];
      if (own && a.b) bb[k] = a.b[k * a.ld_b + row];
    }
    buf[k * PL + x * M + i] = u;
  }
  __syncthreads();

  // ---- r = b - A u of the owned rows, ascending column order ----------------------------------
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const double* um = buf + k * PL + (x - 1) * M;
    const double* ux = buf + k * PL + x * M;
    const double* up = buf + k * PL + (x + 1) * M;
    double t;
    if (CMP)
      t = btd_apply_cmp<M, GRP>(sc, dk, qv, um, ux, up, a.lv.c_sub, a.lv.r_sup, i);
    else
      t = btd_apply_dense<M>(sb, dk, sp, um, ux, up);
    if (own && k < kc) a.r[k * a.ld_r + row] = bb[k] - t;
  }
}

// ---- column-wise reductions: grid (kDotBlocks, K) + one workgroup per column; slice bounds, per-thread stride and LDS
// tree of dot_partial_kernel / diff2_partial_kernel / dot_final_kernel ------------------------------------------------
// partial[c * gridDim.x + b] = sum_{i in slice b} X[i, c] Y[i, c]
static __global__ __launch_bounds__(kThreads) void dot_cols_partial_kernel(int64_t n, const double* x, int64_t ldx, const double* y,
                                                                         int64_t ldy, double* __restrict__ partial) {
  __shared__ double sh[kThreads];
  x += (int64_t)blockIdx.y * ldx;
  y += (int64_t)blockIdx.y * ldy;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) acc = __fma_rn(x[i], y[i], acc);
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// partial[c * gridDim.x + b] = sum_{i in slice b} (X[i, c] - Y[i, ycol ? ycol[c] : c])^2
static __global__ __launch_bounds__(kThreads) void diff2_cols_partial_kernel(int64_t n, const double* x, int64_t ldx,
                                                                           const double* y, int64_t ldy,
                                                                           const int* __restrict__ ycol,
                                                                           double* __restrict__ partial) {
  __shared__ double sh[kThreads];
  x += (int64_t)blockIdx.y * ldx;
  y += (int64_t)(ycol ? ycol[blockIdx.y] : (int)blockIdx.y) * ldy;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const double d = x[i] - y[i];
    acc = __fma_rn(d, d, acc);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// out[c] = sum of column c's partials (workgroup c), optionally its square root
static __global__ __launch_bounds__(kThreads) void dot_cols_final_kernel(int nparts, const double* __restrict__ partial,
                                                                       double* __restrict__ out, int take_sqrt) {
  __shared__ double sh[kThreads];
  partial += (int64_t)blockIdx.x * nparts;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) acc += partial[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = take_sqrt ? sqrt(sh[0]) : sh[0];
}

// ---- conjugate-gradient updates over N x K, grid (ceil(n / kThreads), K): slot c of the work matrices (leading
// dimension ldw) belongs to column xcol[c] of X; its scalars are entry c of the device arrays ------------------------
// a_c = rz_c / (-(p.q)_c);  x += a p;  r += a q
static __global__ __launch_bounds__(kThreads) void pcg_xr_cols_kernel(int64_t n, double* __restrict__ x, int64_t ldx,
                                                                    const int* __restrict__ xcol, double* __restrict__ r,
                                                                    const double* __restrict__ p,
                                                                    const double* __restrict__ q, int64_t ldw,
                                                                    const double* __restrict__ rz,
                                                                    const double* __restrict__ pq) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int c = blockIdx.y;
  const double a = rz[c] / (-pq[c]);
  double* xc = x + (int64_t)xcol[c] * ldx;
  const int64_t w = (int64_t)c * ldw + i;
  xc[i] = __fma_rn(a, p[w], xc[i]);
  r[w] = __fma_rn(a, q[w], r[w]);
}

// p = z + (rz_new / rz_old) p
static __global__ __launch_bounds__(kThreads) void pcg_p_cols_kernel(int64_t n, double* __restrict__ p,
                                                                   const double* __restrict__ z, int64_t ldw,
                                                                   const double* __restrict__ rz_new,
                                                                   const double* __restrict__ rz_old) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int c = blockIdx.y;
  const int64_t w = (int64_t)c * ldw + i;
  p[w] = __fma_rn(rz_new[c] / rz_old[c], p[w], z[w]);
}

}  // namespace aggmg
