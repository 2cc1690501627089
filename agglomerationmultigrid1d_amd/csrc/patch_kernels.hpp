// Element-patch Schwarz smoother of a DG level (aggmg_patch_schwarz_setup): overlapping patches of
// two consecutive elements P_e = {e, e + 1}, e = 0 .. ne - 2, on an operator that is block tridiagonal in the element
// blocking.  One sweep with weight w:
//   r = b - A u                                       (ascending columns, the operator's own entries: btd_apply_cmp / _dense)
//   t_row = (Z_{e-1} r[P_{e-1}])[M + i] + (Z_e r[P_e])[i]   (patch e - 1 first, each dot product in ascending j)
//   u += w (t / c_e)   hybrid, c_e = patches covering element e (1 at both ends, 2 inside);   u += w t   additive
// -- the arithmetic of the generic route (block_sweep_kernel + block_combine_kernel) on the same lists, without index
// lists, without a CSR operator, and S sweeps per launch.
#pragma once
#include "kernels.hpp"

namespace aggmg {

// zrows [N][2][2M]: per row (e, i) the two inverse rows it applies -- row M + i of Z_{e-1}, then row i of Z_e; zeros where
// the patch does not exist (e = 0 / e = ne - 1).  patch_sweep_dict_kernel: the six operator arrays are the dictionary's.
struct PatchArgs {
  const double *dblk, *scol, *qrow, *sub, *sup;   // the element blocks of A (BtdLevel's arrays; compressed or dense couplings)
  const double* zrows;
  int64_t ne;
  int c_sub, r_sup;
  const double* u_in;   // nullptr: the iterate starts at zero
  const double* b;
  double* u_out;
  int nsweeps;
  int owned;            // owned elements per tile; the tile keeps `halo` = 2 * nsweeps more on either side
  int halo;
};

// slabs of 256 / M elements a workgroup holds: what the registers of a thread afford (per slab the row's 4M inverse-row
// words, its M entries of D_e, its couplings, b and u)
template <int M>
struct PatchSlabs {
  static constexpr int NS = M <= 3 ? 4 : (M == 4 ? 3 : (M <= 6 ? 2 : 1));
};

// 256 threads, one per DoF row of a slab, NS slabs: the tile's iterate (ping-pong) and its residual in LDS, each padded by
// one zero element on both sides; the row's operator entries, inverse rows, b and damping in registers, loaded once.
// Temporal blocking: a sweep reaches two elements to each side (the residual reads u[e +- 1], the patch solves r[e +- 1]),
// so after S sweeps the elements 2S and more away from the tile's ends hold what a sweep over the whole level gives.
template <int M, bool CMP, int NS, bool HYB>
__global__ __launch_bounds__(kThreads) void patch_sweep_kernel(PatchArgs a, SweepWeights wts) {
  constexpr int EPS = kThreads / M;   // elements per slab
  constexpr int TE = EPS * NS;        // elements per tile (owned + halos)
  constexpr int PL = (TE + 2) * M;    // a padded vector of the tile: index x * M + j, x in [-1, TE]
  extern __shared__ double lds[];
  double* cur = lds + M;
  double* nxt = cur + PL;
  double* res = nxt + PL;

  const int tid = threadIdx.x;
  const bool active = tid < EPS * M;
  const int le = tid / M;
  const int i = tid - le * M;
  const int64_t ne = a.ne;
  const int64_t e0 = (int64_t)blockIdx.x * a.owned - a.halo;   // element at x = 0

  if (tid < M) {
    cur[-M + tid] = 0.0;
    cur[TE * M + tid] = 0.0;
    nxt[-M + tid] = 0.0;
    nxt[TE * M + tid] = 0.0;
    res[-M + tid] = 0.0;
    res[TE * M + tid] = 0.0;
  }

  double dk[NS][M], lo[NS][CMP ? 1 : M], hi[NS][M], z[NS][4 * M], bb[NS], uu[NS];
  bool valid[NS], inner[NS];

  // ---- load phase: everything the tile needs from HBM, once ----------------------------------------------------------
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    const int64_t e = e0 + x;
    valid[s] = active && e >= 0 && e < ne;
    inner[s] = e > 0 && e < ne - 1;
    bb[s] = 0.0;
    uu[s] = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) dk[s][j] = hi[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < (CMP ? 1 : M); ++j) lo[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * M; ++j) z[s][j] = 0.0;
    if (valid[s]) {
      const int64_t row = e * M + i;
      const double* zr = a.zrows + row * (4 * M);
#pragma unroll
      for (int j = 0; j < 4 * M; ++j) z[s][j] = AGGMG_LD(zr[j]);
#pragma unroll
      for (int j = 0; j < M; ++j) dk[s][j] = AGGMG_LD(a.dblk[row * M + j]);
      if constexpr (CMP) {
        lo[s][0] = AGGMG_LD(a.scol[row]);
        if (i == a.r_sup) {
#pragma unroll
          for (int j = 0; j < M; ++j) hi[s][j] = a.qrow[e * M + j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) lo[s][j] = AGGMG_LD(a.sub[row * M + j]);
#pragma unroll
        for (int j = 0; j < M; ++j) hi[s][j] = AGGMG_LD(a.sup[row * M + j]);
      }
      bb[s] = a.b[row];
      if (a.u_in) uu[s] = a.u_in[row];
    }
    if (active) cur[x * M + i] = uu[s];
  }
  __syncthreads();

  for (int sw = 0; sw < a.nsweeps; ++sw) {
    const double w = wts.w[sw];   // this sweep's factor: wave-uniform, a scalar load
    // residual rows of the tile (zero outside the level)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!active) continue;
      const int x = s * EPS + le;
      const double *um = cur + (x - 1) * M, *ux = cur + x * M, *up = cur + (x + 1) * M;
      double t;
      if constexpr (CMP)
        t = btd_apply_cmp<M, false>(lo[s][0], dk[s], hi[s], um, ux, up, a.c_sub, a.r_sup, i);
      else
        t = btd_apply_dense<M>(lo[s], dk[s], hi[s], um, ux, up);
      res[x * M + i] = valid[s] ? bb[s] - t : 0.0;
    }
    __syncthreads();
    // the two patch solves covering the row, patch e - 1 first
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!active) continue;
      const int x = s * EPS + le;
      const double *ra = res + (x - 1) * M, *rb = res + x * M;
      double ya = 0.0, yb = 0.0;
#pragma unroll
      for (int j = 0; j < 2 * M; ++j) ya += z[s][j] * ra[j];
#pragma unroll
      for (int j = 0; j < 2 * M; ++j) yb += z[s][2 * M + j] * rb[j];
      double v = 0.0;
      v += ya;
      v += yb;
      if (HYB && inner[s]) v = v * 0.5;   // c_e = 2: the division, exactly
      v = w * v;
      const double un = valid[s] ? uu[s] + v : 0.0;
      uu[s] = un;
      nxt[x * M + i] = un;
    }
    __syncthreads();
    double* t2 = cur;
    cur = nxt;
    nxt = t2;
  }

#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    if (valid[s] && x >= a.halo && x < a.halo + a.owned) AGGMG_ST(a.u_out[(e0 + x) * M + i], uu[s]);
  }
}

// The same sweeps with the operator read through the smoother's dictionary (PatchDictDev; set-up: setup.hip,
// setup_patch_dictionary): a's six operator arrays are the dictionary's, [nclasses][...] in the layouts of the full ones,
// and cls[ne] holds the class of every element.  Tile, LDS layout, sweep loop, arithmetic and store phase are
// patch_sweep_kernel's, line by line; the load phase reads the classes of all slabs first and then the record words at
// c * stride + ... in place of e * stride + ..., with ordinary cached loads (the dictionary is re-read by every tile;
// b, u_in and the store keep the plain kernel's forms).  The loads return the bits the full arrays hold, so every result
// is patch_sweep_kernel's bit for bit.  (A kernel of its own text: with the body shared through an inlined function the
// compiler allocates the plain kernels' registers differently, and those are held identical to their earlier build.)
template <int M, bool CMP, int NS, bool HYB>
__global__ __launch_bounds__(kThreads) void patch_sweep_dict_kernel(PatchArgs a, SweepWeights wts,
                                                                    const uint16_t* __restrict__ cls) {
  constexpr int EPS = kThreads / M;   // elements per slab
  constexpr int TE = EPS * NS;        // elements per tile (owned + halos)
  constexpr int PL = (TE + 2) * M;    // a padded vector of the tile: index x * M + j, x in [-1, TE]
  extern __shared__ double lds[];
  double* cur = lds + M;
  double* nxt = cur + PL;
  double* res = nxt + PL;

  const int tid = threadIdx.x;
  const bool active = tid < EPS * M;
  const int le = tid / M;
  const int i = tid - le * M;
  const int64_t ne = a.ne;
  const int64_t e0 = (int64_t)blockIdx.x * a.owned - a.halo;   // element at x = 0

  if (tid < M) {
    cur[-M + tid] = 0.0;
    cur[TE * M + tid] = 0.0;
    nxt[-M + tid] = 0.0;
    nxt[TE * M + tid] = 0.0;
    res[-M + tid] = 0.0;
    res[TE * M + tid] = 0.0;
  }

  double dk[NS][M], lo[NS][CMP ? 1 : M], hi[NS][M], z[NS][4 * M], bb[NS], uu[NS];
  bool valid[NS], inner[NS];
  int c[NS];

  // ---- load phase: the classes first (the record loads depend on them), then the tile's vectors from HBM and its
  // operator words from the dictionary, once --------------------------------------------------------------------------
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int64_t e = e0 + s * EPS + le;
    valid[s] = active && e >= 0 && e < ne;
    c[s] = valid[s] ? (int)cls[e] : 0;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    const int64_t e = e0 + x;
    inner[s] = e > 0 && e < ne - 1;
    bb[s] = 0.0;
    uu[s] = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) dk[s][j] = hi[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < (CMP ? 1 : M); ++j) lo[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * M; ++j) z[s][j] = 0.0;
    if (valid[s]) {
      const int64_t row = e * M + i;
      const int crow = c[s] * M + i;   // the row in its class's record (c < kDictMaxClasses: 32-bit offsets)
      const double* zr = a.zrows + crow * (4 * M);
#pragma unroll
      for (int j = 0; j < 4 * M; ++j) z[s][j] = zr[j];
#pragma unroll
      for (int j = 0; j < M; ++j) dk[s][j] = a.dblk[crow * M + j];
      if constexpr (CMP) {
        lo[s][0] = a.scol[crow];
        if (i == a.r_sup) {
#pragma unroll
          for (int j = 0; j < M; ++j) hi[s][j] = a.qrow[c[s] * M + j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) lo[s][j] = a.sub[crow * M + j];
#pragma unroll
        for (int j = 0; j < M; ++j) hi[s][j] = a.sup[crow * M + j];
      }
      bb[s] = a.b[row];
      if (a.u_in) uu[s] = a.u_in[row];
    }
    if (active) cur[x * M + i] = uu[s];
  }
  __syncthreads();

  for (int sw = 0; sw < a.nsweeps; ++sw) {
    const double w = wts.w[sw];   // this sweep's factor: wave-uniform, a scalar load
    // residual rows of the tile (zero outside the level)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!active) continue;
      const int x = s * EPS + le;
      const double *um = cur + (x - 1) * M, *ux = cur + x * M, *up = cur + (x + 1) * M;
      double t;
      if constexpr (CMP)
        t = btd_apply_cmp<M, false>(lo[s][0], dk[s], hi[s], um, ux, up, a.c_sub, a.r_sup, i);
      else
        t = btd_apply_dense<M>(lo[s], dk[s], hi[s], um, ux, up);
      res[x * M + i] = valid[s] ? bb[s] - t : 0.0;
    }
    __syncthreads();
    // the two patch solves covering the row, patch e - 1 first
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!active) continue;
      const int x = s * EPS + le;
      const double *ra = res + (x - 1) * M, *rb = res + x * M;
      double ya = 0.0, yb = 0.0;
#pragma unroll
      for (int j = 0; j < 2 * M; ++j) ya += z[s][j] * ra[j];
#pragma unroll
      for (int j = 0; j < 2 * M; ++j) yb += z[s][2 * M + j] * rb[j];
      double v = 0.0;
      v += ya;
      v += yb;
      if (HYB && inner[s]) v = v * 0.5;   // c_e = 2: the division, exactly
      v = w * v;
      const double un = valid[s] ? uu[s] + v : 0.0;
      uu[s] = un;
      nxt[x * M + i] = un;
    }
    __syncthreads();
    double* t2 = cur;
    cur = nxt;
    nxt = t2;
  }

#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    if (valid[s] && x >= a.halo && x < a.halo + a.owned) AGGMG_ST(a.u_out[(e0 + x) * M + i], uu[s]);
  }
}

// ---- multiplicative two-colour sweeps (aggmg_patch_gs_setup) -------------------------------------
// The same patches, inverse rows and element blocks, applied one colour at a time: a forward sweep of weight w is the
// half-sweeps c = 0, 1 (a reverse one: c = 1, 0), each
//   r = b - A u                          (from the current u; ascending columns: btd_apply_cmp / _dense)
//   u[P_e] += w Z_e r[P_e]               for every patch e = c (mod 2), each dot product in ascending j
// The patches of a colour are disjoint, so a row applies one inverse row per half-sweep: slot 1 of its zrows (row i of
// Z_e, against r[e], r[e + 1]) where e = c (mod 2) and e <= ne - 2, slot 0 (row M + i of Z_{e-1}, against r[e - 1], r[e])
// where e != c (mod 2) and e >= 1; an element no patch of the colour covers keeps its value.
struct PatchGsArgs {
  PatchArgs p;   // owned / halo: the tile keeps halo = 2 * nsweeps + 1 elements on either side (patch_gs_tile_plan)
  int reverse;   // 0: colours 0, 1; 1: colours 1, 0 (post-smoothing) -- the same in every lane
};

// Tile, load phase and operator registers of patch_sweep_kernel (DICT: of patch_sweep_dict_kernel).  A row writes only
// its own entry of the iterate and reads only the residual while it does, so the iterate is updated in place: one iterate
// and one residual vector in LDS, each padded by one zero element a side.  Temporal blocking: a half-sweep reads
// u[e - 1 .. e + 2] (first element of its patch) or u[e - 2 .. e + 1] (second), so a sweep reaches 3 elements to one side
// and 2 to the other and S sweeps reach 2 S + 1: the elements 2 S + 1 and more away from the tile's ends hold what sweeps
// over the whole level give.  Plain C++ per row -- no atomics, no cross-lane operations -- so no result depends on where
// the tiles lie.
template <int M, bool CMP, int NS, bool DICT>
__device__ __forceinline__ void patch_gs_body(const PatchGsArgs& g, const SweepWeights& wts, const uint16_t* __restrict__ cls) {
  const PatchArgs& a = g.p;
  constexpr int EPS = kThreads / M;   // elements per slab
  constexpr int TE = EPS * NS;        // elements per tile (owned + halos)
  constexpr int PL = (TE + 2) * M;    // a padded vector of the tile: index x * M + j, x in [-1, TE]
  extern __shared__ double lds[];
  double* cur = lds + M;
  double* res = cur + PL;

  const int tid = threadIdx.x;
  const bool active = tid < EPS * M;
  const int le = tid / M;
  const int i = tid - le * M;
  const int64_t ne = a.ne;
  const int64_t e0 = (int64_t)blockIdx.x * a.owned - a.halo;   // element at x = 0

  if (tid < M) {
    cur[-M + tid] = 0.0;
    cur[TE * M + tid] = 0.0;
    res[-M + tid] = 0.0;
    res[TE * M + tid] = 0.0;
  }

  double dk[NS][M], lo[NS][CMP ? 1 : M], hi[NS][M], z[NS][4 * M], bb[NS], uu[NS];
  bool valid[NS], with_prev[NS], with_next[NS];   // the patches {e - 1, e} and {e, e + 1} exist
  int par[NS];                                    // e mod 2
  int c[NS];

  // ---- load phase: everything the tile needs from HBM (DICT: its operator words from the dictionary), once ----------------
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int64_t e = e0 + s * EPS + le;
    valid[s] = active && e >= 0 && e < ne;
    c[s] = (DICT && valid[s]) ? (int)cls[e] : 0;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    const int64_t e = e0 + x;
    par[s] = (int)(e & 1);
    with_prev[s] = valid[s] && e >= 1;
    with_next[s] = valid[s] && e <= ne - 2;
    bb[s] = 0.0;
    uu[s] = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) dk[s][j] = hi[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < (CMP ? 1 : M); ++j) lo[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * M; ++j) z[s][j] = 0.0;
    if (valid[s]) {
      const int64_t row = e * M + i;
      if constexpr (DICT) {
        const int crow = c[s] * M + i;   // the row in its class's record (c < kDictMaxClasses: 32-bit offsets)
        const double* zr = a.zrows + crow * (4 * M);
#pragma unroll
        for (int j = 0; j < 4 * M; ++j) z[s][j] = zr[j];
#pragma unroll
        for (int j = 0; j < M; ++j) dk[s][j] = a.dblk[crow * M + j];
        if constexpr (CMP) {
          lo[s][0] = a.scol[crow];
          if (i == a.r_sup) {
#pragma unroll
            for (int j = 0; j < M; ++j) hi[s][j] = a.qrow[c[s] * M + j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < M; ++j) lo[s][j] = a.sub[crow * M + j];
#pragma unroll
          for (int j = 0; j < M; ++j) hi[s][j] = a.sup[crow * M + j];
        }
      } else {
        const double* zr = a.zrows + row * (4 * M);
#pragma unroll
        for (int j = 0; j < 4 * M; ++j) z[s][j] = AGGMG_LD(zr[j]);
#pragma unroll
        for (int j = 0; j < M; ++j) dk[s][j] = AGGMG_LD(a.dblk[row * M + j]);
        if constexpr (CMP) {
          lo[s][0] = AGGMG_LD(a.scol[row]);
          if (i == a.r_sup) {
#pragma unroll
            for (int j = 0; j < M; ++j) hi[s][j] = a.qrow[e * M + j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < M; ++j) lo[s][j] = AGGMG_LD(a.sub[row * M + j]);
#pragma unroll
          for (int j = 0; j < M; ++j) hi[s][j] = AGGMG_LD(a.sup[row * M + j]);
        }
      }
      bb[s] = a.b[row];
      if (a.u_in) uu[s] = a.u_in[row];
    }
    if (active) cur[x * M + i] = uu[s];
  }
  __syncthreads();

  for (int sw = 0; sw < a.nsweeps; ++sw) {
    const double w = wts.w[sw];   // this sweep's factor, for both of its halves: wave-uniform, a scalar load
    for (int h = 0; h < 2; ++h) {
      const int colour = h ^ g.reverse;
      // residual rows of the tile (zero outside the level)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (!active) continue;
        const int x = s * EPS + le;
        const double *um = cur + (x - 1) * M, *ux = cur + x * M, *up = cur + (x + 1) * M;
        double t;
        if constexpr (CMP)
          t = btd_apply_cmp<M, false>(lo[s][0], dk[s], hi[s], um, ux, up, a.c_sub, a.r_sup, i);
        else
          t = btd_apply_dense<M>(lo[s], dk[s], hi[s], um, ux, up);
        res[x * M + i] = valid[s] ? bb[s] - t : 0.0;
      }
      __syncthreads();
      // the one patch of this colour covering the row: the element is its first one (slot 1) or its second (slot 0)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (!active) continue;
        const int x = s * EPS + le;
        const bool first = par[s] == colour;
        const double* r = res + (first ? x : x - 1) * M;
        double y = 0.0;
#pragma unroll
        for (int j = 0; j < 2 * M; ++j) y += (first ? z[s][2 * M + j] : z[s][j]) * r[j];
        if (first ? with_next[s] : with_prev[s]) {
          uu[s] = uu[s] + w * y;
          cur[x * M + i] = uu[s];
        }
      }
      __syncthreads();
    }
  }

#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    if (valid[s] && x >= a.halo && x < a.halo + a.owned) AGGMG_ST(a.u_out[(e0 + x) * M + i], uu[s]);
  }
}

template <int M, bool CMP, int NS>
__global__ __launch_bounds__(kThreads) void patch_gs_kernel(PatchGsArgs g, SweepWeights wts) {
  patch_gs_body<M, CMP, NS, false>(g, wts, nullptr);
}

// the operator read through the smoother's dictionary, as patch_sweep_dict_kernel reads it: the same bits, so every
// result is patch_gs_kernel's
template <int M, bool CMP, int NS>
__global__ __launch_bounds__(kThreads) void patch_gs_dict_kernel(PatchGsArgs g, SweepWeights wts,
                                                                 const uint16_t* __restrict__ cls) {
  patch_gs_body<M, CMP, NS, true>(g, wts, cls);
}

// ---- one-launch ascent of a multiplicative patch level (split ascent of the element-partitioned cycle) ----
// patch_gs_body with two additions.  The prolongation in the load phase: a row starts from u_in[row] + sum_c L[row][c]
// uc[J mc + c], J = e / rho (uniform agglomerates), with the arithmetic and the summation order of the zero-sweep fused
// launch that patch_up runs in front of the sweeps -- halo elements included, whose prolonged values the owned ones read --
// so the result is that two-launch sequence's bit for bit.  And the tile of a workgroup is selectable as fused_tile()'s
// is: workgroup w runs tile w + (w >= tile_split ? tile_skip : 0) -- the tiles at the two ends of the level, or the ones
// in between (fused_tile_subset) -- and writes only its own tile's owned rows of u_out; no scratch vector is shared
// between two launches.  The smoother's dictionary is read by class as patch_gs_dict_kernel reads it; the transfer rows
// come from the level's full lf / lf1 arrays.  A body of its own text: patch_gs_body's kernels keep their code.
struct PatchGsUpArgs {
  PatchGsArgs g;      // g.p.u_in: the pre-smoothed iterate (never null); reverse = 1
  const double* uc;   // the coarse level's result
  const double* lf;   // [N][mc] rows of L
  const double* lf1;  // [N] their second entries when mc == 2 and every first entry is exactly 1.0, else null
  int mc, rho;
  int tile_split;
  int64_t tile_skip;
};
__device__ __forceinline__ int64_t patch_up_tile(const PatchGsUpArgs& a) {
  return (int64_t)blockIdx.x + ((int)blockIdx.x >= a.tile_split ? a.tile_skip : 0);
}
// the second product rounded, the first fused into the sum: what btd_prolong2 is compiled to in the fused kernel
// (kernels.hpp says the same of its dictionary variant), said explicitly
__device__ __forceinline__ double patch_up_prolong2(double2 l2, double2 u2) { return __fma_rn(l2.x, u2.x, l2.y * u2.y); }

template <int M, bool CMP, int NS, bool DICT>
__device__ __forceinline__ void patch_gs_up_body(const PatchGsUpArgs& ga, const SweepWeights& wts, const uint16_t* __restrict__ cls) {
  const PatchGsArgs& g = ga.g;
  const PatchArgs& a = g.p;
  constexpr int EPS = kThreads / M;   // elements per slab
  constexpr int TE = EPS * NS;        // elements per tile (owned + halos)
  constexpr int PL = (TE + 2) * M;    // a padded vector of the tile: index x * M + j, x in [-1, TE]
  extern __shared__ double lds[];
  double* cur = lds + M;
  double* res = cur + PL;

  const int tid = threadIdx.x;
  const bool active = tid < EPS * M;
  const int le = tid / M;
  const int i = tid - le * M;
  const int64_t ne = a.ne;
  const int64_t e0 = patch_up_tile(ga) * a.owned - a.halo;   // element at x = 0

  if (tid < M) {
    cur[-M + tid] = 0.0;
    cur[TE * M + tid] = 0.0;
    res[-M + tid] = 0.0;
    res[TE * M + tid] = 0.0;
  }

  double dk[NS][M], lo[NS][CMP ? 1 : M], hi[NS][M], z[NS][4 * M], bb[NS], uu[NS];
  bool valid[NS], with_prev[NS], with_next[NS];   // the patches {e - 1, e} and {e, e + 1} exist
  int par[NS];                                    // e mod 2
  int c[NS];

  // ---- load phase: everything the tile needs from HBM (DICT: its operator words from the dictionary), once ----------------
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int64_t e = e0 + s * EPS + le;
    valid[s] = active && e >= 0 && e < ne;
    c[s] = (DICT && valid[s]) ? (int)cls[e] : 0;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    const int64_t e = e0 + x;
    par[s] = (int)(e & 1);
    with_prev[s] = valid[s] && e >= 1;
    with_next[s] = valid[s] && e <= ne - 2;
    bb[s] = 0.0;
    uu[s] = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) dk[s][j] = hi[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < (CMP ? 1 : M); ++j) lo[s][j] = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * M; ++j) z[s][j] = 0.0;
    if (valid[s]) {
      const int64_t row = e * M + i;
      if constexpr (DICT) {
        const int crow = c[s] * M + i;   // the row in its class's record (c < kDictMaxClasses: 32-bit offsets)
        const double* zr = a.zrows + crow * (4 * M);
#pragma unroll
        for (int j = 0; j < 4 * M; ++j) z[s][j] = zr[j];
#pragma unroll
        for (int j = 0; j < M; ++j) dk[s][j] = a.dblk[crow * M + j];
        if constexpr (CMP) {
          lo[s][0] = a.scol[crow];
          if (i == a.r_sup) {
#pragma unroll
            for (int j = 0; j < M; ++j) hi[s][j] = a.qrow[c[s] * M + j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < M; ++j) lo[s][j] = a.sub[crow * M + j];
#pragma unroll
          for (int j = 0; j < M; ++j) hi[s][j] = a.sup[crow * M + j];
        }
      } else {
        const double* zr = a.zrows + row * (4 * M);
#pragma unroll
        for (int j = 0; j < 4 * M; ++j) z[s][j] = AGGMG_LD(zr[j]);
#pragma unroll
        for (int j = 0; j < M; ++j) dk[s][j] = AGGMG_LD(a.dblk[row * M + j]);
        if constexpr (CMP) {
          lo[s][0] = AGGMG_LD(a.scol[row]);
          if (i == a.r_sup) {
#pragma unroll
            for (int j = 0; j < M; ++j) hi[s][j] = a.qrow[e * M + j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < M; ++j) lo[s][j] = AGGMG_LD(a.sub[row * M + j]);
#pragma unroll
          for (int j = 0; j < M; ++j) hi[s][j] = AGGMG_LD(a.sup[row * M + j]);
        }
      }
      bb[s] = a.b[row];
      uu[s] = a.u_in[row];
      {  // u += L uc : J = e / rho, ascending mode order -- the zero-sweep fused ascent's expressions (kernels.hpp)
        const int64_t J = e / ga.rho;
        double add = 0.0;
        if (ga.mc == 2) {  // one 16-byte load each for the L row and the coarse pair
          typedef double v2d __attribute__((ext_vector_type(2)));
          double2 l2;
          if (ga.lf1) {
            l2.x = 1.0;
            l2.y = AGGMG_LD(ga.lf1[row]);
          } else {
            const v2d lv2 = AGGMG_LD(*reinterpret_cast<const v2d*>(ga.lf + row * 2));
            l2.x = lv2.x;
            l2.y = lv2.y;
          }
          const double2 u2 = *reinterpret_cast<const double2*>(ga.uc + J * 2);
          add = patch_up_prolong2(l2, u2);
        } else {
          for (int c2 = 0; c2 < ga.mc; ++c2) add += ga.lf[row * ga.mc + c2] * ga.uc[J * ga.mc + c2];
        }
        uu[s] += add;
      }
    }
    if (active) cur[x * M + i] = uu[s];
  }
  __syncthreads();

  for (int sw = 0; sw < a.nsweeps; ++sw) {
    const double w = wts.w[sw];   // this sweep's factor, for both of its halves: wave-uniform, a scalar load
    for (int h = 0; h < 2; ++h) {
      const int colour = h ^ g.reverse;
      // residual rows of the tile (zero outside the level)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (!active) continue;
        const int x = s * EPS + le;
        const double *um = cur + (x - 1) * M, *ux = cur + x * M, *up = cur + (x + 1) * M;
        double t;
        if constexpr (CMP)
          t = btd_apply_cmp<M, false>(lo[s][0], dk[s], hi[s], um, ux, up, a.c_sub, a.r_sup, i);
        else
          t = btd_apply_dense<M>(lo[s], dk[s], hi[s], um, ux, up);
        res[x * M + i] = valid[s] ? bb[s] - t : 0.0;
      }
      __syncthreads();
      // the one patch of this colour covering the row: the element is its first one (slot 1) or its second (slot 0)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (!active) continue;
        const int x = s * EPS + le;
        const bool first = par[s] == colour;
        const double* r = res + (first ? x : x - 1) * M;
        double y = 0.0;
#pragma unroll
        for (int j = 0; j < 2 * M; ++j) y += (first ? z[s][2 * M + j] : z[s][j]) * r[j];
        if (first ? with_next[s] : with_prev[s]) {
          uu[s] = uu[s] + w * y;
          cur[x * M + i] = uu[s];
        }
      }
      __syncthreads();
    }
  }

#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int x = s * EPS + le;
    if (valid[s] && x >= a.halo && x < a.halo + a.owned) AGGMG_ST(a.u_out[(e0 + x) * M + i], uu[s]);
  }
}

template <int M, bool CMP, int NS>
__global__ __launch_bounds__(kThreads) void patch_gs_up_kernel(PatchGsUpArgs g, SweepWeights wts) {
  patch_gs_up_body<M, CMP, NS, false>(g, wts, nullptr);
}
template <int M, bool CMP, int NS>
__global__ __launch_bounds__(kThreads) void patch_gs_up_dict_kernel(PatchGsUpArgs g, SweepWeights wts,
                                                                    const uint16_t* __restrict__ cls) {
  patch_gs_up_body<M, CMP, NS, true>(g, wts, cls);
}

// ---- set-up ---------------------------------------------------------------------------------------------------------------
// the dense patch blocks A[P_p, P_p], [ne - 1][2m][2m] row-major, from the element blocks of A: one thread per entry
static __global__ __launch_bounds__(kThreads) void patch_assemble_kernel(int64_t total, int m, int cmp, int c_sub, int r_sup,
                                                                         const double* __restrict__ dblk,
                                                                         const double* __restrict__ scol,
                                                                         const double* __restrict__ qrow,
                                                                         const double* __restrict__ sub,
                                                                         const double* __restrict__ sup, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int m2 = 2 * m;
  const int64_t p = t / (m2 * m2);
  const int rc = (int)(t - p * (m2 * m2));
  const int ri = rc / m2, cj = rc - ri * m2;
  const int ei = ri / m, ii = ri - ei * m, ej = cj / m, jj = cj - ej * m;
  const int64_t row = (p + ei) * m + ii;   // the operator's row
  double v;
  if (ei == ej)
    v = dblk[row * m + jj];
  else if (ei == 0)   // Sup_p
    v = cmp ? (ii == r_sup ? qrow[p * m + jj] : 0.0) : sup[row * m + jj];
  else                // Sub_{p + 1}
    v = cmp ? (jj == c_sub ? scol[row] : 0.0) : sub[row * m + jj];
  out[t] = v;
}

// zrows from the patch inverses zinv [ne - 1][2m][2m]: one thread per word
static __global__ __launch_bounds__(kThreads) void patch_zrows_kernel(int64_t total, int m, int64_t ne,
                                                                      const double* __restrict__ zinv, double* __restrict__ zrows) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int m2 = 2 * m;
  const int64_t row = t / (2 * m2);
  const int sj = (int)(t - row * (2 * m2));
  const int slot = sj / m2, j = sj - slot * m2;
  const int64_t e = row / m;
  const int i = (int)(row - e * m);
  double v = 0.0;
  if (slot == 0) {
    if (e >= 1) v = zinv[((e - 1) * m2 + m + i) * m2 + j];
  } else {
    if (e + 1 < ne) v = zinv[(e * m2 + i) * m2 + j];
  }
  zrows[t] = v;
}

}  // namespace aggmg
