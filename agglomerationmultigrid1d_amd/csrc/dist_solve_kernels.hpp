// Vector kernels of the Krylov loops on the element-partitioned path: conjugate gradients (distributed.pcg; EXTENSION: the
// reference stops at ldiv!, src/solvers.jl:84-92) and, in the second half of the file, flexible GMRES
// (distributed.fgmres).  A local vector holds a rank's owned rows plus its ghost rows; the
// owned rows are a few [lo, hi) index ranges (one for DG / agglomerated layouts, vertices + element-interior nodes for
// CG chain layouts).  The global scalars of the recurrence are rank-ordered sums of what these kernels reduce over the
// owned rows, so every reduction has a fixed shape -- slice bounds, per-thread stride, LDS tree, then dot_final_kernel
// over the partial sums in their stored order -- and no atomics: the same bits from run to run.
//   owned_dot_partial_kernel   partial[g * G + b] = sum over slice b of range g of x_i y_i
//   owned_xr_kernel            x += a p, r += a q on the whole local vector; partial[b] = sum of the new r_i^2 over the
//                              owned rows of slice b
//   owned_p_kernel             p = z + beta p on the whole local vector
// Pure vector bandwidth: two consecutive doubles per thread and step as one 16-byte access.  A pair starts where the
// ADDRESS is 16-byte aligned (`par`: ((address of element 0) / 8) & 1 -- the pair starts are the i with i + par even), a
// slice's odd first / last element goes to thread 0.  VEC = false (the vectors of a call do not share that alignment)
// walks the same pairs with 8-byte accesses: same assignment of elements to threads, same order of additions, same bits.
// The multiply-adds are __fma_rn (multi_solve_kernels.hpp: whether `a * b + c` contracts depends on the code around it).
#pragma once
#include "kernels.hpp"

namespace aggmg {

constexpr int kOwnedBlocks = 1024;    // slices per range (dot) / of the local vector (update): fixed, as kDotBlocks
constexpr int kOwnedMaxRanges = 4;

struct OwnedRanges {
  int64_t lo[kOwnedMaxRanges], hi[kOwnedMaxRanges];
  int n;
};

template <bool VEC>
__device__ __forceinline__ void owned_ld2(const double* p, double& v0, double& v1) {
  if (VEC) {
    const double2 t = *reinterpret_cast<const double2*>(p);
    v0 = t.x;
    v1 = t.y;
  } else {
    v0 = p[0];
    v1 = p[1];
  }
}
template <bool VEC>
__device__ __forceinline__ void owned_st2(double* p, double v0, double v1) {
  if (VEC) {
    *reinterpret_cast<double2*>(p) = make_double2(v0, v1);
  } else {
    p[0] = v0;
    p[1] = v1;
  }
}

// slice b of [lo, hi) cut into gridDim.x slices of even length: -> [s0, s1); `first`: the first pair start in it (or s1),
// np: whole pairs from there
__device__ __forceinline__ void owned_slice(int64_t lo, int64_t hi, int par, int64_t& s0, int64_t& s1, int64_t& first,
                                            int64_t& np) {
  int64_t per = (hi - lo + gridDim.x - 1) / gridDim.x;
  per += per & 1;
  s0 = lo + (int64_t)blockIdx.x * per;
  if (s0 > hi) s0 = hi;
  s1 = s0 + per < hi ? s0 + per : hi;
  first = s0 + ((s0 + par) & 1);
  if (first > s1) first = s1;
  np = (s1 - first) >> 1;
}

// the block's sum -> partial[slot] (LDS tree of dot_partial_kernel)
__device__ __forceinline__ void owned_block_sum(double acc, double* __restrict__ partial, int64_t slot) {
  __shared__ double sh[kThreads];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[slot] = sh[0];
}

// grid (kOwnedBlocks, ranges)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void owned_dot_partial_kernel(OwnedRanges R, int par, const double* __restrict__ x,
                                                                     const double* __restrict__ y,
                                                                     double* __restrict__ partial) {
  const int g = blockIdx.y;
  int64_t s0, s1, first, np;
  owned_slice(R.lo[g], R.hi[g], par, s0, s1, first, np);
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < np; k += kThreads) {
    const int64_t i = first + 2 * k;
    double x0, x1, y0, y1;
    owned_ld2<VEC>(x + i, x0, x1);
    owned_ld2<VEC>(y + i, y0, y1);
    acc = __fma_rn(x0, y0, acc);
    acc = __fma_rn(x1, y1, acc);
  }
  if (threadIdx.x == 0) {
    if (first > s0) acc = __fma_rn(x[s0], y[s0], acc);
    if (first + 2 * np < s1) acc = __fma_rn(x[s1 - 1], y[s1 - 1], acc);
  }
  owned_block_sum(acc, partial, (int64_t)g * gridDim.x + blockIdx.x);
}

__device__ __forceinline__ bool owned_has(const OwnedRanges& R, int64_t i) {
  bool in = false;
#pragma unroll
  for (int g = 0; g < kOwnedMaxRanges; ++g) in = in || (g < R.n && i >= R.lo[g] && i < R.hi[g]);
  return in;
}

// one row of the fused update; returns acc + r_new^2 on an owned row
__device__ __forceinline__ double owned_xr_row(double a, double pv, double qv, double& xv, double& rv, bool own, double acc) {
  xv = __fma_rn(a, pv, xv);
  rv = __fma_rn(a, qv, rv);
  return own ? __fma_rn(rv, rv, acc) : acc;
}

// grid (kOwnedBlocks): PCG step with q = -A p (the residual kernel's sign), a = rz / (-(p.q)) formed by the caller from
// the rank-summed scalars
template <bool VEC>
__global__ __launch_bounds__(kThreads) void owned_xr_kernel(int64_t n, int par, double* __restrict__ x, double* __restrict__ r,
                                                            const double* __restrict__ p, const double* __restrict__ q,
                                                            double a, OwnedRanges R, double* __restrict__ partial) {
  int64_t s0, s1, first, np;
  owned_slice(0, n, par, s0, s1, first, np);
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < np; k += kThreads) {
    const int64_t i = first + 2 * k;
    double x0, x1, r0, r1, p0, p1, q0, q1;
    owned_ld2<VEC>(x + i, x0, x1);
    owned_ld2<VEC>(r + i, r0, r1);
    owned_ld2<VEC>(p + i, p0, p1);
    owned_ld2<VEC>(q + i, q0, q1);
    acc = owned_xr_row(a, p0, q0, x0, r0, owned_has(R, i), acc);
    acc = owned_xr_row(a, p1, q1, x1, r1, owned_has(R, i + 1), acc);
    owned_st2<VEC>(x + i, x0, x1);
    owned_st2<VEC>(r + i, r0, r1);
  }
  if (threadIdx.x == 0) {
    if (first > s0) acc = owned_xr_row(a, p[s0], q[s0], x[s0], r[s0], owned_has(R, s0), acc);
    if (first + 2 * np < s1) acc = owned_xr_row(a, p[s1 - 1], q[s1 - 1], x[s1 - 1], r[s1 - 1], owned_has(R, s1 - 1), acc);
  }
  owned_block_sum(acc, partial, blockIdx.x);
}

// grid (kOwnedBlocks): p = z + beta p
template <bool VEC>
__global__ __launch_bounds__(kThreads) void owned_p_kernel(int64_t n, int par, double* __restrict__ p,
                                                           const double* __restrict__ z, double beta) {
  int64_t s0, s1, first, np;
  owned_slice(0, n, par, s0, s1, first, np);
  for (int64_t k = threadIdx.x; k < np; k += kThreads) {
    const int64_t i = first + 2 * k;
    double p0, p1, z0, z1;
    owned_ld2<VEC>(p + i, p0, p1);
    owned_ld2<VEC>(z + i, z0, z1);
    owned_st2<VEC>(p + i, __fma_rn(beta, p0, z0), __fma_rn(beta, p1, z1));
  }
  if (threadIdx.x == 0) {
    if (first > s0) p[s0] = __fma_rn(beta, p[s0], z[s0]);
    if (first + 2 * np < s1) p[s1 - 1] = __fma_rn(beta, p[s1 - 1], z[s1 - 1]);
  }
}

// ---- flexible GMRES on the element-partitioned path (distributed.fgmres): the two passes of the orthogonalisation over a
// basis V (vector g at V + g * ld) and the local vector w, in groups of at most kOwnedGroup vectors per pass over w --
// G accumulators and G + 1 streams per thread, as kKrylovGroup in krylov_kernels.hpp -- and the scaling v = w / s.
//   owned_multi_dot_partial_kernel<G>   partial[i * pstride + g * gridDim.x + b] = sum over slice b of range g of w_r V_i[r]
//   owned_multi_final_kernel            out[i] = the tree of dot_final_kernel over vector i's partial sums, stored order
//   owned_multi_axpy_kernel<G>          w <- fma(c[G-1], V_{G-1}, ... fma(c[0], V_0, w)) on the whole local vector; NORM:
//                                       partial[b] = sum of the squares of the stored values over the owned rows of slice b
//   owned_div_kernel                    v = w / s on the whole local vector
// The pair grid is w's (`par` from w's address), so w is always read and written 16 bytes at a time; VEC says whether the
// basis vectors (the target of the division) share that alignment.  Per accumulator the order of the multiply-adds is
// owned_dot_partial_kernel's with x = w, y = V_i, and the LDS tree is owned_block_sum's: dot i has the bits of
// aggmg_owned_dot_dev(w, V_i).
constexpr int kOwnedGroup = 8;

struct OwnedCoefs {
  double c[kOwnedGroup];
};

// grid (kOwnedBlocks, ranges)
template <int G, bool VEC>
__global__ __launch_bounds__(kThreads) void owned_multi_dot_partial_kernel(OwnedRanges R, int par, const double* __restrict__ w,
                                                                           const double* __restrict__ V, int64_t ld,
                                                                           double* __restrict__ partial, int64_t pstride) {
  __shared__ double sh[G][kThreads];
  const int rg = blockIdx.y;
  int64_t s0, s1, first, np;
  owned_slice(R.lo[rg], R.hi[rg], par, s0, s1, first, np);
  double acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.0;
  for (int64_t k = threadIdx.x; k < np; k += kThreads) {
    const int64_t i = first + 2 * k;
    double w0, w1;
    owned_ld2<true>(w + i, w0, w1);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double v0, v1;
      owned_ld2<VEC>(V + (int64_t)g * ld + i, v0, v1);
      acc[g] = __fma_rn(w0, v0, acc[g]);
      acc[g] = __fma_rn(w1, v1, acc[g]);
    }
  }
  if (threadIdx.x == 0) {
    if (first > s0) {
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __fma_rn(w[s0], V[(int64_t)g * ld + s0], acc[g]);
    }
    if (first + 2 * np < s1) {
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __fma_rn(w[s1 - 1], V[(int64_t)g * ld + s1 - 1], acc[g]);
    }
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
  if ((int)threadIdx.x < G) partial[(int64_t)threadIdx.x * pstride + (int64_t)rg * gridDim.x + blockIdx.x] = sh[threadIdx.x][0];
}

// grid (dots): workgroup i sums partial[i * pstride + 0 .. nparts - 1] as dot_final_kernel sums its partials
__global__ __launch_bounds__(kThreads) void owned_multi_final_kernel(int nparts, const double* __restrict__ partial,
                                                                     int64_t pstride, double* __restrict__ out) {
  __shared__ double sh[kThreads];
  partial += (int64_t)blockIdx.x * pstride;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) acc += partial[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// one row of the update: the chain over the group's vectors, ascending
template <int G>
__device__ __forceinline__ double owned_axpy_row(const OwnedCoefs& c, const double* __restrict__ V, int64_t ld, int64_t i,
                                                 double x) {
#pragma unroll
  for (int g = 0; g < G; ++g) x = __fma_rn(c.c[g], V[(int64_t)g * ld + i], x);
  return x;
}

// grid (kOwnedBlocks)
template <int G, bool VEC, bool NORM>
__global__ __launch_bounds__(kThreads) void owned_multi_axpy_kernel(int64_t n, int par, double* __restrict__ w,
                                                                    const double* __restrict__ V, int64_t ld, OwnedCoefs c,
                                                                    OwnedRanges R, double* __restrict__ partial) {
  int64_t s0, s1, first, np;
  owned_slice(0, n, par, s0, s1, first, np);
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < np; k += kThreads) {
    const int64_t i = first + 2 * k;
    double x0, x1;
    owned_ld2<true>(w + i, x0, x1);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double v0, v1;
      owned_ld2<VEC>(V + (int64_t)g * ld + i, v0, v1);
      x0 = __fma_rn(c.c[g], v0, x0);
      x1 = __fma_rn(c.c[g], v1, x1);
    }
    owned_st2<true>(w + i, x0, x1);
    if (NORM) {
      if (owned_has(R, i)) acc = __fma_rn(x0, x0, acc);
      if (owned_has(R, i + 1)) acc = __fma_rn(x1, x1, acc);
    }
  }
  if (threadIdx.x == 0) {
    if (first > s0) {
      const double x = owned_axpy_row<G>(c, V, ld, s0, w[s0]);
      w[s0] = x;
      if (NORM && owned_has(R, s0)) acc = __fma_rn(x, x, acc);
    }
    if (first + 2 * np < s1) {
      const double x = owned_axpy_row<G>(c, V, ld, s1 - 1, w[s1 - 1]);
      w[s1 - 1] = x;
      if (NORM && owned_has(R, s1 - 1)) acc = __fma_rn(x, x, acc);
    }
  }
  if (NORM) owned_block_sum(acc, partial, blockIdx.x);
}

// grid (kOwnedBlocks): v = w / s (a division, as div_scalar_kernel's); the pair grid is w's, VEC: v shares its alignment.
// v == w is allowed (every thread reads its pair before it stores it), hence no __restrict__.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void owned_div_kernel(int64_t n, int par, const double* w, double s, double* v) {
  int64_t s0, s1, first, np;
  owned_slice(0, n, par, s0, s1, first, np);
  for (int64_t k = threadIdx.x; k < np; k += kThreads) {
    const int64_t i = first + 2 * k;
    double w0, w1;
    owned_ld2<true>(w + i, w0, w1);
    owned_st2<VEC>(v + i, w0 / s, w1 / s);
  }
  if (threadIdx.x == 0) {
    if (first > s0) v[s0] = w[s0] / s;
    if (first + 2 * np < s1) v[s1 - 1] = w[s1 - 1] / s;
  }
}

}  // namespace aggmg
