// The two streaming passes of the orthogonalisation of flexible GMRES (aggmg_fgmres_dev; EXTENSION: the reference has
// no Krylov loop), over a column-major basis V (vector i at V + i * ld, ld >= n) and one vector w:
//   multi_dot_partial_kernel<G>      G <= 8 dots V_i . w in ONE pass over w and the G vectors
//   multi_axpy_kernel<G, NORM>       w <- fma(c[G-1], V_{G-1}, ... fma(c[0], V_0, w)) in place, in one pass; NORM: the
//                                    same pass sums the squares of the values it stores
// and, further down, their forms over K independent bases in one launch (multi_dot_cols_partial_kernel,
// multi_axpy_cols_kernel, div_scalar_cols_kernel).
// Both keep the reduction shape of dot_partial_kernel (kernels.hpp): its grid (kDotBlocks), its contiguous slice of rows
// per workgroup, its per-thread order i = lo + tid, += kThreads, its LDS tree per accumulator, and then the one-workgroup
// final tree (dot_cols_final_kernel / dot_final_kernel).  So dot i is bit for bit aggmg_dot_dev(V_i, w), and the norm
// is bit for bit aggmg_norm2_dev of the vector the pass stored.  dot_partial_kernel's `acc += x[i] * y[i]` is one
// v_fma_f64 in its code object (the compiler contracts it); these kernels must not depend on what the compiler decides
// around other code, so they say __fma_rn.  No atomics: the same bits run to run.
#pragma once
#include "kernels.hpp"

namespace aggmg {

constexpr int kKrylovGroup = 8;   // vectors per pass: G + 1 streams per thread, G accumulators in registers

// partial[g * gridDim.x + b] = sum_{i in slice b} V_g[i] w[i],  g < G
template <int G>
static __global__ __launch_bounds__(kThreads) void multi_dot_partial_kernel(int64_t n, const double* __restrict__ V, int64_t ld,
                                                                          const double* __restrict__ w,
                                                                          double* __restrict__ partial) {
  __shared__ double sh[G][kThreads];
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  double acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const double wi = w[i];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __fma_rn(V[(int64_t)g * ld + i], wi, acc[g]);
  }
#pragma unroll
  for (int g = 0; g < G; ++g) sh[g][threadIdx.x] = acc[g];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int g = 0; g < G; ++g) sh[g][threadIdx.x] += sh[g][threadIdx.x + s];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < G) partial[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = sh[threadIdx.x][0];
}

// w[i] <- fma(scale c[G-1], V_{G-1}[i], ... fma(scale c[0], V_0[i], w[i])), ascending g; c on the device, scale = +-1
// (exact: the orthogonalisation subtracts the dots it has just formed).  NORM: partial[b] = sum_{i in slice b} of the
// squares of the stored values, in dot_partial_kernel's order.
template <int G, bool NORM>
static __global__ __launch_bounds__(kThreads) void multi_axpy_kernel(int64_t n, const double* __restrict__ V, int64_t ld,
                                                                   const double* __restrict__ coef, double scale,
                                                                   double* __restrict__ w, double* __restrict__ partial) {
  __shared__ double sh[NORM ? kThreads : 1];
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  double c[G];
#pragma unroll
  for (int g = 0; g < G; ++g) c[g] = scale * coef[g];
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    double x = w[i];
#pragma unroll
    for (int g = 0; g < G; ++g) x = __fma_rn(c[g], V[(int64_t)g * ld + i], x);
    w[i] = x;
    if (NORM) acc = __fma_rn(x, x, acc);
  }
  if (NORM) {
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
  }
}

// ---- the same passes over K independent bases at once (aggmg_fgmres_multi_dev): grid (kDotBlocks, Kact), blockIdx.y = the
// active slot c.  Basis vector g of slot c is V + g * bstride + c * cstride (basis index outer, slot inner), its vector
// w is W + c * ldw.  Within a slot every sum keeps the shape above -- slice, stride, __fma_rn, LDS tree per accumulator
// -- so dot (c, g) is bit for bit multi_dot_partial_kernel's on slot c alone, and so are the stored values and the norm.

// partial[(c * pcol + g) * gridDim.x + b] = sum_{i in slice b} V_g[i, c] W[i, c],  g < G; pcol: dots per slot of the
// whole pass (the caller offsets `partial` by the group's first vector), so that ONE dot_cols_final_kernel launch of
// Kact * pcol workgroups finishes every dot into out[c * pcol + g]
template <int G>
static __global__ __launch_bounds__(kThreads) void multi_dot_cols_partial_kernel(int64_t n, const double* __restrict__ V,
                                                                               int64_t bstride, int64_t cstride,
                                                                               const double* __restrict__ W, int64_t ldw,
                                                                               int64_t pcol, double* __restrict__ partial) {
  __shared__ double sh[G][kThreads];
  const int64_t c = blockIdx.y;
  V += c * cstride;
  W += c * ldw;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  double acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const double wi = W[i];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __fma_rn(V[(int64_t)g * bstride + i], wi, acc[g]);
  }
#pragma unroll
  for (int g = 0; g < G; ++g) sh[g][threadIdx.x] = acc[g];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int g = 0; g < G; ++g) sh[g][threadIdx.x] += sh[g][threadIdx.x + s];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < G) partial[(c * pcol + threadIdx.x) * gridDim.x + blockIdx.x] = sh[threadIdx.x][0];
}

// W[i, d] <- fma(scale coef[c][G-1], V_{G-1}[i, c], ... fma(scale coef[c][0], V_0[i, c], W[i, d])), ascending g, with
// coef[c][g] = coef[c * cld + g] on the device and d = wcol ? wcol[c] : c the destination column of slot c (the
// orthogonalisation updates its own slot; the end of a restart cycle updates column wcol[c] of X).  NORM:
// partial[c * gridDim.x + b] = the slice's sum of squares of the stored values: one dot_cols_final_kernel launch of Kact
// workgroups finishes the norms.
template <int G, bool NORM>
static __global__ __launch_bounds__(kThreads) void multi_axpy_cols_kernel(int64_t n, const double* __restrict__ V, int64_t bstride,
                                                                        int64_t cstride, const double* __restrict__ coef,
                                                                        int64_t cld, double scale, double* __restrict__ W,
                                                                        int64_t ldw, const int* __restrict__ wcol,
                                                                        double* __restrict__ partial) {
  __shared__ double sh[NORM ? kThreads : 1];
  const int64_t c = blockIdx.y;
  V += c * cstride;
  W += (wcol ? (int64_t)wcol[c] : c) * ldw;
  coef += c * cld;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  double cf[G];
#pragma unroll
  for (int g = 0; g < G; ++g) cf[g] = scale * coef[g];
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    double x = W[i];
#pragma unroll
    for (int g = 0; g < G; ++g) x = __fma_rn(cf[g], V[(int64_t)g * bstride + i], x);
    W[i] = x;
    if (NORM) acc = __fma_rn(x, x, acc);
  }
  if (NORM) {
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[c * gridDim.x + blockIdx.x] = sh[0];
  }
}

// V[i, c] = W[i, c] / s[c]: div_scalar_kernel on every slot, grid (ceil(n / kThreads), Kact)
static __global__ __launch_bounds__(kThreads) void div_scalar_cols_kernel(int64_t n, const double* __restrict__ W, int64_t ldw,
                                                                        const double* __restrict__ s, double* __restrict__ V,
                                                                        int64_t ldv) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t c = blockIdx.y;
  if (i < n) V[c * ldv + i] = W[c * ldw + i] / s[c];
}

}  // namespace aggmg
