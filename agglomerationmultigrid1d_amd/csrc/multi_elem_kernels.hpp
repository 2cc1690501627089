// K right-hand sides on a dictionary level, one THREAD per element (AGGMG_OPT_MULTI_ELEMENT_THREADS):
// btd_elem_rec_kernel's schedule (elem_kernels.hpp) for the kc columns of a group, where btd_multi_kernel (multi_kernels.hpp)
// gives every row a thread and streams the level's full operator arrays.  What an element's columns share is done once per
// workgroup -- the class table copied into LDS, the class word, the tile's index arithmetic -- and the workgroup then walks
// the columns in passes of KB: loads of b, u_in and the coarse pair at the column's stride, prolongation, g, the sweeps (KB
// iterate planes in LDS, one barrier per sweep for all of them), the store of the owned iterate and, in the descent, the
// explicit residual and its two-mode restriction.  After the first pass's entry phase the launch issues no global load
// but the columns' vectors (and the escape path's words).  The record words a pass needs -- the sweeps' stencil, the
// residual's decoded rows -- are read from LDS again in every pass and not held over the columns: held, the stencil alone
// costs the descent 12 VGPRs (117 against 105), and the decoded rows would cost 40 more.
//
// Bitwise: a column's arithmetic is btd_elem_rec_kernel's, expression by expression -- the same __device__ helpers
// (ElemRecStencil, elem_rec_g, elem_group_dot4, elem_sym_row_apply, sym_residual_decode) and the same pinned __fma_rn /
// __dmul_rn / __dadd_rn chains, so no contraction depends on the code around them.  The tile is planned by the same
// planner with the K-column halves' halos; an owned element's sweeps see only the halo's values, and every restricted
// coarse element lies inside one tile and sums its fine rows in ascending order: the same bits whatever the tiling.
#pragma once
#include "elem_kernels.hpp"
#include "multi_kernels.hpp"

namespace aggmg {

// two doubles of a column: a column starts wherever the caller's stride puts it, so the pair is 8-byte aligned only
typedef double elem_col_v2d __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ void elem_col_ld2(const double* p, double& x, double& y) {
  const elem_col_v2d v = *reinterpret_cast<const elem_col_v2d*>(p);
  x = v.x;
  y = v.y;
}
// elem_rec_st_iterate for a column
__device__ __forceinline__ void elem_col_st_iterate(double* op, const double (&uu)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    elem_col_v2d v;
    v.x = uu[j];
    v.y = uu[j + 1];
#if AGGMG_NT & 2
    __builtin_nontemporal_store(v, reinterpret_cast<elem_col_v2d*>(op + j));
#else
    *reinterpret_cast<elem_col_v2d*>(op + j) = v;
#endif
  }
}

// LDS of a launch: two iterate buffers of kb planes each (elem_lds_bytes: one plane pair), then the class table
template <int M>
constexpr size_t elem_rec_multi_lds_bytes(int kb, int nclasses) {
  return (size_t)kb * elem_lds_bytes<M>() + (size_t)nclasses * kElemRecWords * sizeof(double);
}

// elem_rec_sweep's update of one column's plane cur -> nxt, without its barrier and swap (the caller's, once for the KB
// planes of a pass): u + w (g - pcol u-[c_sub] - B^{-1}[:, r_sup] (q . u+) - u)
template <int M>
__device__ __forceinline__ void elem_rec_sweep_plane(const ElemRecStencil<M>& st, const double* cur, double* nxt, int x, int c_sub,
                                                     double w, bool valid, const double (&g)[M], double (&uu)[M]) {
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
    if (!valid) un = 0.0;
    uu[i] = un;
    nxt[i * S + x] = un;
  }
}

// RES: the launch forms and restricts the explicit residual of every column (the descent); otherwise it ends with the
// iterates (the storing ascent).  KB: columns of a pass, which share every barrier.  What the launcher guarantees
// (multi_elem_launch_ok, aggmg_hip.hip): btd_elem_rec_kernel's conditions on ma.a and t -- a dictionary launch of
// block-Jacobi sweeps, at least one, over all tiles of the level, two-mode transfers of equal agglomerates, t.rec the
// level's table with 1 <= t.nclasses <= kElemRecMaxClasses, RES == (ma.a.do_residual != 0) with dup / corr in the records
// -- 1 <= ma.kc, every column stride at least the vector's length, and elem_rec_multi_lds_bytes<M>(KB, t.nclasses) of LDS.
// Columns at or past ma.kc are neither read nor written.
template <int M, bool RES, int KB>
__global__ __launch_bounds__(kElemThreads) void btd_elem_rec_multi_kernel(MultiArgs ma, SweepWeights wts, ElemRecTab t) {
  static_assert(M == 4, "the element-thread kernel's block size");
  static_assert(KB == 1 || KB == 2, "columns of a pass: 4 would need more than the 64 KB of LDS a launch gets unasked");
  constexpr int TE = kElemThreads;
  constexpr int S = TE + 2;            // words of one component in a plane
  constexpr int PL = M * S;            // words of a plane
  constexpr int T = M * (M + 1) / 2;
  const FusedArgs& a = ma.a;
  extern __shared__ double lds[];
  double* cur = lds + 1;               // column c of a pass, (j, x) at cur[c * PL + j * S + x]
  double* nxt = lds + KB * PL + 1;
  double* const tab = lds + 2 * KB * PL;   // the class table, behind the buffers (16-byte aligned: 2 KB PL is even)

  const int x = threadIdx.x;
  const int kc = ma.kc;
  const int64_t ne = a.lv.ne;
  const int64_t e0 = fused_tile(a) * a.owned - a.halo_left;   // element at x = 0
  const int own0 = a.halo_left, own1 = a.halo_left + a.owned;
  const int64_t rem = ne - 1 - e0;
  if (rem < 0) return;   // a tile wholly past the level: before any barrier
  const int xlo = e0 < 0 ? (int)-e0 : 0, xhi = rem < TE - 1 ? (int)rem : TE - 1;
  const bool valid = x >= xlo && x <= xhi;
  const bool own = valid && x >= own0 && x < own1;
  const unsigned xc = (unsigned)(x < xlo ? xlo : x > xhi ? xhi : x);

  // ---- once per workgroup: the table's loads, the class word, where the element's rows and its coarse pair lie ---------
  elem_v2d tv[kElemRecStage];
  elem_rec_fetch(t, x, tv);
  const bool pro = a.lf_in != nullptr;
  unsigned ce = (a.lv.cls + e0)[xc];
  const int64_t row0 = e0 * M + xc * M;                        // the element's first row (a lane outside: its stand-in's)
  const int64_t orow0 = e0 * M + (int64_t)(unsigned)(x * M);   // ... of an owned element, for the stores
  int64_t J2 = 0;
  if (pro) J2 = 2 * (ne <= 0x7fffffff ? (int64_t)((unsigned)(e0 + xc) / (unsigned)a.rho_in) : (e0 + xc) / a.rho_in);

  // a pass's loads of b, u_in and the coarse pair, columns k0 .. k0 + KB (below kc), straight-line
  double bb[KB][M], uu[KB][M], ucx[KB], ucy[KB];
  auto load_cols = [&](int k0) {
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      ucx[c] = 0.0;
      ucy[c] = 0.0;
      if (c > 0 && k0 + c >= kc) {   // (uniform: the last pass of a group whose columns do not fill it)
#pragma unroll
        for (int j = 0; j < M; ++j) bb[c][j] = uu[c][j] = 0.0;
        continue;
      }
      const int64_t k = k0 + c;
      const double* const bp = a.b + k * ma.ld_b + row0;
      // (no first iterate: the load goes to b's line and is dropped -- no branch in the load group)
      const double* const up = a.u_in ? a.u_in + k * ma.ld_uin + row0 : bp;
#pragma unroll
      for (int j = 0; j < M; j += 2) elem_col_ld2(bp + j, bb[c][j], bb[c][j + 1]);
#pragma unroll
      for (int j = 0; j < M; j += 2) elem_col_ld2(up + j, uu[c][j], uu[c][j + 1]);
      if (pro) elem_col_ld2(a.uc + k * ma.ld_uc + J2, ucx[c], ucy[c]);
    }
  };
  load_cols(0);
  elem_rec_store(tab, t, x, tv);
  if (x < 4 * M * KB) {   // the zero elements at the ends of every plane of both buffers
    const int j = x & (M - 1), w = (x / M) & 3, c = x / (4 * M);
    (w & 2 ? nxt : cur)[c * PL + j * S + (w & 1 ? TE : -1)] = 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < KB; ++c) elem_rec_pin_all<M>(ce, bb[c], uu[c], ucx[c], ucy[c]);

  const double* const rec = tab + ce * kElemRecWords;
  const int c_sub = a.lv.c_sub, r_sup = a.lv.r_sup;

  for (int k0 = 0; k0 < kc; k0 += KB) {
    if (k0 > 0) load_cols(k0);
    ElemRecStencil<M> st;
    st.load(rec, r_sup);   // held over the sweeps of the pass
    // ---- per column: prolongation, g, the first iterate into its plane --------------------------------------------------
    double g[KB][M];
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if (!a.u_in) {
#pragma unroll
        for (int j = 0; j < M; ++j) uu[c][j] = 0.0;
      }
      if (pro) {   // u += L uc: the second product rounded, the first fused into the sum
#pragma unroll
        for (int j = 0; j < M; ++j) {
          double lx, ly;
          elem_ld2(rec + kElemRecLf + 2 * j, lx, ly);
          uu[c][j] = __dadd_rn(uu[c][j], __fma_rn(lx, ucx[c], __dmul_rn(ly, ucy[c])));
        }
      }
      if (!valid) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
          uu[c][j] = 0.0;
          bb[c][j] = 0.0;
        }
      }
      elem_rec_g<M>(rec, bb[c], g[c]);
#pragma unroll
      for (int i = 0; i < M; ++i) cur[c * PL + i * S + x] = uu[c][i];
    }
    __syncthreads();

    // ---- the sweeps: every plane of the pass, then one barrier ----------------------------------------------------------
    for (int sw = 0; sw < a.nsweeps; ++sw) {
      const double w = wts.w[(unsigned)sw];
#pragma unroll
      for (int c = 0; c < KB; ++c) elem_rec_sweep_plane<M>(st, cur + c * PL, nxt + c * PL, x, c_sub, w, valid, g[c], uu[c]);
      __syncthreads();
      double* const sp = cur;
      cur = nxt;
      nxt = sp;
    }

    if (a.u_out && own) {
#pragma unroll
      for (int c = 0; c < KB; ++c)
        if (k0 + c < kc) elem_col_st_iterate(a.u_out + (int64_t)(k0 + c) * ma.ld_uout + orow0, uu[c]);
    }
    if constexpr (RES) {
      // ---- explicit residual r = b - A u of the element's rows (btd_elem_rec_kernel's), the record's words from LDS ------
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
      double rr[KB][M];
#pragma unroll
      for (int c = 0; c < KB; ++c) {
        const double* const pl = cur + c * PL;
        const double um = pl[c_sub * S + x - 1];
        double up[M];
#pragma unroll
        for (int j = 0; j < M; ++j) up[j] = pl[j * S + x + 1];
        double dlo, dhi;
        elem_group_dot4(st.q, up, dlo, dhi);
#pragma unroll
        for (int i = 0; i < M; ++i) {
          double s = __fma_rn(sc[i], um, 0.0);
#pragma unroll
          for (int j = 0; j < M; ++j) s = __fma_rn(D[i][j], uu[c][j], s);   // (a valid element's uu is its words of the plane)
          if (i == r_sup) s = __dadd_rn(s, i < 2 ? dlo : dhi);
          rr[c][i] = own ? __dadd_rn(bb[c][i], -s) : 0.0;
        }
      }
      // ---- restriction onto two coarse modes, through the (now free) planes, ascending fine row --------------------------
      __syncthreads();
#pragma unroll
      for (int i = 0; i < M; ++i) {
        double lx, ly;
        elem_ld2(rec + kElemRecLf + 2 * i, lx, ly);
#pragma unroll
        for (int c = 0; c < KB; ++c) {
          nxt[c * PL + i * S + x] = own ? __dmul_rn(lx, rr[c][i]) : 0.0;
          cur[c * PL + i * S + x] = own ? __dmul_rn(ly, rr[c][i]) : 0.0;
        }
      }
      __syncthreads();
      const int rho = a.rho_out;
      const int ncoarse = a.owned / rho;   // owned coarse elements of this tile
      const int64_t J0 = fused_tile(a) * ncoarse;
#pragma unroll
      for (int c = 0; c < KB; ++c) {
        if (k0 + c >= kc) continue;
        double* const rcp = a.rc_out + (int64_t)(k0 + c) * ma.ld_rc;
        for (int k2 = x; k2 < ncoarse * 2; k2 += TE) {
          const int Jl = k2 >> 1, m = k2 & 1;
          const int64_t J = J0 + Jl;
          if (J >= a.nec_out) continue;
          const double* pr = (m ? cur : nxt) + c * PL + a.halo_left + Jl * rho;
          double acc = 0.0;
          for (int k = 0; k < rho; ++k) {
#pragma unroll
            for (int j = 0; j < M; ++j) acc = __dadd_rn(acc, pr[j * S + k]);
          }
          rcp[J * 2 + m] = acc;
        }
      }
      // (the next pass writes the planes these sums read)
      if (k0 + KB < kc) __syncthreads();
    }
  }
}

}  // namespace aggmg
