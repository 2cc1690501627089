// CG chain path of libaggmg_hip: continuous-Galerkin levels renumbered element by element run a
// temporally blocked fused point-Jacobi kernel (cgt_kernels.hpp) instead of the generic CSR kernels.
//
// The reference smooths CG levels with JacobiSmoother (cg_smoother(cgMesh, A, :jac),
// src/smoother.jl:88-102; src/mesh_heirarchy.jl:51,58) on matrices numbered "vertices first"
// (src/cg_mesh.jl:37-45,59-65).  aggmg_jacobi_setup_elements receives the element node lists the
// reference's own cg_smoother has at hand (cgMesh.mElements[k].mNodesInd -- the mBlockInds matrix of
// its Schwarz variants, src/smoother.jl:104-134), derives the element-contiguous order from them and
// re-packs the operator -- every stored entry is read from the uploaded matrix, nothing is assumed
// about the mesh beyond "consecutive elements share exactly one node".
#include "internal.hpp"
#include "cgt_multi_kernels.hpp"

// ---------------------------------------------------------------------------------------------
// tiles
// ---------------------------------------------------------------------------------------------
// slabs per thread (tile = NT / M * NS blocks): tuning knobs.  tools/exp_chain_tiles.sh on the config-5
// hierarchy at 2^24 elements: one slab everywhere 4.22 ms per V-cycle, two 4.31, four (M <= 2) 4.36-4.41 --
// occupancy beats the smaller halo share, as on the block-tridiagonal kernel
#ifndef AGGMG_CGT_NS1
#define AGGMG_CGT_NS1 1
#endif
#ifndef AGGMG_CGT_NS2
#define AGGMG_CGT_NS2 1
#endif
#ifndef AGGMG_CGT_NS4
#define AGGMG_CGT_NS4 1
#endif
// K: 0 point Jacobi, 1 element Schwarz, 2 red-black element Gauss-Seidel.  The Gauss-Seidel sweeps cost four blocks
// of halo each: two slabs per thread there (config-5 hierarchy at 2^24: 6.8 instead of 8.9 ms per V(3,3) cycle); the
// Schwarz sweeps (two blocks of halo) are faster with one (31 vs 34 us per sweep at 2^20 elements, p = 4)
#ifndef AGGMG_CGT_NS_GS
#define AGGMG_CGT_NS_GS 2
#endif
#ifndef AGGMG_CGT_NT
#define AGGMG_CGT_NT kThreads
#endif
template <int M, int K = 0>
struct CgtTile {
  static constexpr int NT = AGGMG_CGT_NT;   // threads per workgroup (tuning knob: tools/exp_tiles_r04.sh)
  static constexpr int NS0 = (M == 1) ? AGGMG_CGT_NS1 : (M == 2) ? AGGMG_CGT_NS2 : (M <= 4) ? AGGMG_CGT_NS4 : 3;
  static constexpr int NS = (K == 2) ? (NS0 < AGGMG_CGT_NS_GS ? AGGMG_CGT_NS_GS : NS0) : NS0;
  static constexpr int EPS = NT / M;
  static constexpr int TE = EPS * NS;
};

template <int SW>
static int cgt_tile_blocks_t(int m) {
  int te = 0;   // (no form of chain_form, forms.hpp: no tile)
  with_block_size<chain_form>(m, [&](auto n) { te = CgtTile<decltype(n)::value, SW>::TE; });
  return te;
}
int cgt_tile_blocks(int m) { return cgt_tile_blocks_t<0>(m); }

// sweeps fused into one launch: every sweep costs one block of halo per side (element Schwarz sweeps: two,
// red-black element Gauss-Seidel: four)
static int cgt_halo_per_sweep(int sw) { return sw == 3 ? 4 : (sw ? 2 : 1); }
static int cgt_max_sweeps(int m, int sw = 0) {
  const int te = sw == 3 ? cgt_tile_blocks_t<2>(m) : cgt_tile_blocks_t<0>(m);
  return std::max(1, std::min(8, te / (8 * cgt_halo_per_sweep(sw))));
}

int cgt_max_fused_sweeps(const CgtDev& g) { return cgt_max_sweeps(g.m, g.sw); }

// ---------------------------------------------------------------------------------------------
// K columns per launch (AGGMG_OPT_CHAIN_MULTI; cgt_multi_kernels.hpp)
// ---------------------------------------------------------------------------------------------
// the most columns a launch of block size M takes (a variant that spilled would get a lower ceiling here; the cycle's
// group stays what it is and goes in several launches)
template <int M>
constexpr int cgt_multi_kb_ceiling() { return 8; }

template <int M>
static int cgt_multi_launch_t(aggmg_ctx* ctx, CgtMultiArgs m, const SweepWeights& wts) {
  constexpr int NT = 256;
  CgtArgs& a = m.a;
  if (a.do_residual && a.tout.type == kTrNone) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column chain launch with a residual and no restriction");
  const int kind = !a.do_residual ? kChainNoRestrict : (a.tout.type == kTrChain ? kChainToChain : kChainToAgg);
  const int rho = kind == kChainToAgg ? a.tout.rho : 1;
  const int kc_all = m.kc;
  for (int c0 = 0; c0 < kc_all; c0 += cgt_multi_kb_ceiling<M>()) {
    const int kc = std::min(kc_all - c0, cgt_multi_kb_ceiling<M>());
    const ChainMultiPlan p = chain_multi_tile_plan(M, a.nsweeps, kind, rho, col_group(kc), a.cls != nullptr, NT);   // host_plan.hpp, the planner multi_chain_level_ok asks
    if (p.owned <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column chain tile too small for the requested halo");
    CgtMultiArgs q = m;
    q.kc = kc;
    q.a.owned = p.owned;
    q.a.halo_left = p.halo_left;
    if (q.a.u_in) q.a.u_in += c0 * m.ld_uin;
    q.a.b += c0 * m.ld_b;
    if (q.a.u_out) q.a.u_out += c0 * m.ld_uout;
    if (q.a.uc) q.a.uc += c0 * m.ld_uc;
    if (q.a.rc_out) q.a.rc_out += c0 * m.ld_rc;
    const int64_t ntiles = (a.lv.ne + p.owned - 1) / p.owned;
    if (ntiles == 0) return AGGMG_OK;
    if (ntiles >= ((int64_t)1 << 31)) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "grid too large");
    with_col_group(kc, [&](auto g) {
      constexpr int KB = decltype(g)::value;
      if (a.cls)
        hipLaunchKernelGGL((cgt_multi_kernel<M, KB, NT, true>), dim3((unsigned)ntiles), dim3(NT), p.lds_bytes, ctx->stream, q, wts);
      else
        hipLaunchKernelGGL((cgt_multi_kernel<M, KB, NT, false>), dim3((unsigned)ntiles), dim3(NT), p.lds_bytes, ctx->stream, q, wts);
    });
    HIPCHK(hipGetLastError());
    ++ctx->chain_multi_launches;
  }
  return AGGMG_OK;
}

static int cgt_multi_launch(aggmg_ctx* ctx, const CgtDev& g, const CgtMultiArgs& m, const SweepWeights& wts) {
  if (g.sw != 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column chain launch on element-block sweeps");
  int rc = AGGMG_OK;
  if (!with_block_size<chain_dict_form>(g.m, [&](auto n) { rc = cgt_multi_launch_t<decltype(n)::value>(ctx, m, wts); }))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: chain block size not instantiated for the K-column kernel");
  return rc;
}

template <int M, int K>
static int cgt_launch_tt(aggmg_ctx* ctx, CgtArgs a, const SweepWeights& wts, int sw, CgtChk* chk_io);

template <int M>
static int cgt_launch_t(aggmg_ctx* ctx, CgtArgs a, const SweepWeights& wts, int sw, CgtChk* chk_io) {
  if (a.nsweeps == 0) sw = 0;
  if (sw == 3) return cgt_launch_tt<M, 2>(ctx, a, wts, sw, chk_io);
  return sw ? cgt_launch_tt<M, 1>(ctx, a, wts, sw, chk_io) : cgt_launch_tt<M, 0>(ctx, a, wts, sw, chk_io);
}

template <int M, int K>
static int cgt_launch_tt(aggmg_ctx* ctx, CgtArgs a, const SweepWeights& wts, int sw, CgtChk* chk_io) {
  using T = CgtTile<M, K>;
  // halo: one block per sweep and side (element Schwarz: the update of a block reads the residual of its two
  // neighbours, i.e. the iterate two blocks away); the residual needs one more valid neighbour on both sides,
  // the restriction one more block of residual on the left (chain) or on the right (agglomerating)
  // (red-black element Gauss-Seidel: two such half-sweeps per sweep)
  int hl = a.nsweeps * cgt_halo_per_sweep(sw), hr = hl;
  if (sw == 3 && a.gs == 0) a.gs = 1;
  if (a.do_residual) {
    hl += 1 + (a.tout.type == kTrChain ? 1 : 0);
    hr += 1 + (a.tout.type == kTrAgg ? 1 : 0);
  } else if (a.chk_part) {   // a checkpoint after the last sweep forms residual rows of the final iterate
    hl += 1;
    hr += 1;
  }
  if (a.chk_part && K != 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: checkpoint launch with element-block sweeps");
  const int align = a.tout.type == kTrAgg ? a.tout.rho : 1;
  const int owned = chain_tile_owned(T::TE, hl, hr, align);   // host_plan.hpp
  if (owned <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "chain tile too small for the requested halo");
  a.owned = owned;
  a.halo_left = hl;
  a.tile_split = 0;
  a.tile_skip = 0;
  const int64_t ntiles = (a.lv.ne + owned - 1) / owned;
  if (chk_io) chk_io->ntiles = ntiles;
  if (ntiles == 0) return AGGMG_OK;
  // every tile stores its sums at chk_part[(checkpoint * ntiles + tile) * 2]: never past what was reserved
  if (a.chk_part && (!chk_io || ntiles > chk_io->cap))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: checkpoint launch of more tiles than its partial sums have room for");
  if (ntiles >= ((int64_t)1 << 31)) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "grid too large");
  a.chk_tiles = ntiles;
  if (a.chk_stride < 1) a.chk_stride = 1 << 30;
  size_t lds = (size_t)(sw ? 3 : 2) * (T::TE + 2) * M * sizeof(double) + (a.chk_part ? (size_t)2 * (T::NT / 64) * sizeof(double) : 0);
  // the operator dictionary (cgt_dictionary put its arrays in place of the full ones): point-Jacobi launches without
  // checkpoints on a block size of chain_dict_form; the tile's classes go to LDS behind the iterate buffers
  if (a.cls) {
    if constexpr (K == 0 && chain_dict_form(M)) {
      if (a.chk_part) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: dictionary launch of a checkpoint variant");
      lds += (size_t)(T::TE + 2) * sizeof(uint16_t);
      hipLaunchKernelGGL((cgt_fused_kernel<M, T::NS, T::NT, 0, false, true>), dim3((unsigned)ntiles), dim3(T::NT), lds, ctx->stream, a, wts);
      HIPCHK(hipGetLastError());
      return AGGMG_OK;
    }
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: dictionary launch of a chain variant that does not index by class");
  }
  if constexpr (K == 0) {
    if (a.chk_part) {
      hipLaunchKernelGGL((cgt_fused_kernel<M, T::NS, T::NT, 0, true>), dim3((unsigned)ntiles), dim3(T::NT), lds, ctx->stream, a, wts);
      HIPCHK(hipGetLastError());
      return AGGMG_OK;
    }
  }
  if constexpr (K == 2) {
    hipLaunchKernelGGL((cgt_fused_kernel<M, T::NS, T::NT, 3>), dim3((unsigned)ntiles), dim3(T::NT), lds, ctx->stream, a, wts);
  } else if constexpr (K == 1) {
    if (sw == 1)
      hipLaunchKernelGGL((cgt_fused_kernel<M, T::NS, T::NT, 1>), dim3((unsigned)ntiles), dim3(T::NT), lds, ctx->stream, a, wts);
    else
      hipLaunchKernelGGL((cgt_fused_kernel<M, T::NS, T::NT, 2>), dim3((unsigned)ntiles), dim3(T::NT), lds, ctx->stream, a, wts);
  } else {
    hipLaunchKernelGGL((cgt_fused_kernel<M, T::NS, T::NT, 0>), dim3((unsigned)ntiles), dim3(T::NT), lds, ctx->stream, a, wts);
  }
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int cgt_launch(aggmg_ctx* ctx, const CgtDev& g, const CgtArgs& a, const SweepWeights& wts, CgtChk* chk_io = nullptr) {
  int rc = AGGMG_OK;
  if (!with_block_size<chain_form>(g.m, [&](auto n) { rc = cgt_launch_t<decltype(n)::value>(ctx, a, wts, g.sw, chk_io); }))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "chain block size not instantiated");
  return rc;
}

static CgtArgs cgt_args(const CgtDev& g) {
  CgtArgs a;
  std::memset(&a, 0, sizeof(a));
  a.lv = CgtLevel{g.dblk, g.subrow, g.supcol, g.ne, g.zrows, g.zlast};
  a.perm = g.perm;
  a.affine = g.affine ? 1 : 0;
  return a;
}

// The level's operator dictionary in place of its full arrays: the point-Jacobi launches of a cycle -- no checkpoint -- on
// a level that has one.  tin / tout are the level's own transfer (or none).  The variant reads the same bits from the
// dictionary (cgt_fused_kernel<..., DICT = true>).
static void cgt_dictionary(CgtArgs& a, const CgtDev& g, const CgtDictDev* d) {
  if (!d || g.sw != 0 || a.chk_part) return;
  a.lv.dblk = d->dblk;
  a.lv.subrow = d->subrow;
  a.lv.supcol = d->supcol;
  a.cls = d->cls;
  for (CgtXfer* x : {&a.tin, &a.tout})
    if (x->type != kTrNone) {
      x->l = d->l;
      x->lp = d->lp;
    }
}

static CgtXfer cgt_xfer(const TransferCgt& t, bool coarse_native) {
  CgtXfer x;
  x.type = t.type;
  x.l = t.l;
  x.lp = t.lp;
  x.cperm = (t.type == kTrChain && !coarse_native) ? t.cperm : nullptr;
  x.mc = t.mc;
  x.rho = t.rho;
  x.nec = t.nec;
  return x;
}

// (set-up of the chain form and of its transfers: setup.hip, on the device)

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
// Chunk chain: src -(s1 sweeps)-> t0 -> t1 -> ... -> dst.  `first` decorates the first launch
// (prolongation), `last` the last one (residual / restriction); intermediates are block-ordered.
struct CgtChain {
  const double* src = nullptr;
  bool src_ext = false;
  const double* b = nullptr;
  bool b_ext = false;
  double* dst = nullptr;
  bool dst_ext = false;
  double *t0 = nullptr, *t1 = nullptr;  // block-ordered temporaries (needed when the sweeps do not fit one launch)
  int gs = 0;  // red-black element Gauss-Seidel: colour order of every sweep (1 forward, 2 reverse)
};

static int cgt_run(aggmg_ctx* ctx, const CgtDev& g, const CgtChain& c, Damping alpha, int nsweeps, const CgtArgs& first,
                   const CgtArgs& last, int kind, int level, CgtChk* chk = nullptr, const CgtDictDev* dict = nullptr) {
  // at most smax sweeps per launch (2 * smax + 3 blocks of halo always fit a tile)
  const int smax = cgt_max_sweeps(g.m, g.sw);
  const int nl = std::max(1, (nsweeps + smax - 1) / smax);
  if (chk && (nl != 1 || g.sw != 0)) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: checkpoints need the sweeps in one point-Jacobi launch");
  if (nl > 1 && (!c.t0 || (nl > 2 && !c.t1))) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: chain temporaries missing");
  const double* src = c.src;
  bool src_ext = c.src_ext;
  int left = nsweeps;
  for (int q = 0; q < nl; ++q) {
    CgtArgs a = cgt_args(g);
    a.gs = c.gs;
    a.nsweeps = std::min(left, smax);
    const SweepWeights wts = alpha.from(nsweeps - left).launch(a.nsweeps);   // this launch's slice of the run
    left -= a.nsweeps;
    a.u_in = src;
    a.b = c.b;
    a.ext = (src && src_ext ? kExtUin : 0) | (c.b_ext ? kExtB : 0);
    if (q == 0) {
      a.tin = first.tin;
      a.uc = first.uc;
    }
    double* dst;
    if (q == nl - 1) {
      dst = c.dst;
      if (c.dst_ext) a.ext |= kExtUout;
      a.do_residual = last.do_residual;
      a.r_out = last.r_out;
      if (last.r_out && (last.ext & kExtRout)) a.ext |= kExtRout;
      a.tout = last.tout;
      a.rc_out = last.rc_out;
    } else {
      dst = (q % 2 == 0) ? c.t0 : c.t1;  // launch q reads what launch q - 1 wrote
    }
    a.u_out = dst;
    if (chk) {
      a.chk_sweep = chk->sweep;
      a.chk_stride = chk->stride;
      a.chk_final = chk->final;
      a.chk_exact = chk->exact;
      a.chk_part = chk->part;
      a.ext |= kExtB;   // (the caller-side indices are formed: chk_exact goes through them)
      if (!c.b_ext) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: checkpoint launch on block-ordered vectors");
    }
    cgt_dictionary(a, g, dict);   // (every chunk: the intermediate launches read the operator too)
    {
      ProfScope ps(ctx, q == nl - 1 ? kind : AGGMG_KIND_SMOOTH, level);
      CHECK(cgt_launch(ctx, g, a, wts, chk));
    }
    src = dst;
    src_ext = false;
  }
  return AGGMG_OK;
}

int cgt_smooth_ext(aggmg_ctx* ctx, const CgtDev& g, const double* u_in, const double* b, Damping alpha, int nsweeps,
                   double* u_out, int level, CgtChk* chk) {
  if (nsweeps == 0) {
    if (u_in)
      HIPCHK(hipMemcpyAsync(u_out, u_in, g.N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    else
      HIPCHK(hipMemsetAsync(u_out, 0, g.N * sizeof(double), ctx->stream));
    return AGGMG_OK;
  }
  CgtChain c;
  c.src = u_in;
  c.src_ext = true;
  c.b = b;
  c.b_ext = true;
  c.dst = u_out;
  c.dst_ext = true;
  WorkLease t0, t1;   // (held across cgt_run: the chain keeps raw pointers)
  if (nsweeps > cgt_max_sweeps(g.m, g.sw)) {
    CHECK(scratch_lease(ctx, kScratchPing, g.ne * g.m, "cgt_smooth_ext", &t0));
    CHECK(scratch_lease(ctx, kScratchPong, g.ne * g.m, "cgt_smooth_ext", &t1));
    c.t0 = t0;
    c.t1 = t1;
  }
  CgtArgs none;
  std::memset(&none, 0, sizeof(none));
  return cgt_run(ctx, g, c, alpha, nsweeps, none, none, AGGMG_KIND_SMOOTH, level, chk);
}

int cgt_residual_ext(aggmg_ctx* ctx, const CgtDev& g, const double* u, const double* b, double* r_out) {
  CgtArgs a = cgt_args(g);
  a.u_in = u;
  a.b = b;
  a.ext = kExtUin | kExtB | kExtRout;
  a.do_residual = 1;
  a.r_out = r_out;
  return cgt_launch(ctx, g, a, SweepWeights{});   // (no sweeps)
}

// descending half on a fused chain level (src/solvers.jl:28-37): nPre sweeps, residual, restriction
int cgt_down(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* uin, const double* rhs, int nPre, double alpha) {
  Level& l = h->lv[k];
  Level& c = h->lv[k + 1];
  const CgtDev& g = *l.S->cgt;
  CgtChain ch;
  ch.src = uin;
  ch.src_ext = true;  // only level 0 has an initial guess, and it is the caller's vector
  ch.b = rhs;
  ch.b_ext = (k == 0) || !l.native_io;
  ch.dst = l.u[0];
  ch.t0 = l.u[1];
  ch.t1 = l.tmp;
  ch.gs = 1;  // pre-smoothing: even elements, then odd ones
  CgtArgs none, last;
  std::memset(&none, 0, sizeof(none));
  std::memset(&last, 0, sizeof(last));
  last.do_residual = 1;
  last.tout = cgt_xfer(*l.tc, c.native_io);
  last.rc_out = c.rhs;
  return cgt_run(ctx, g, ch, l.damp_pre(alpha), nPre, none, last, AGGMG_KIND_FUSED_DOWN, k, nullptr, l.cdict.get());
}

// ascending half (src/solvers.jl:41-47): prolongation-add, nPost sweeps
// src: the pre-smoothed iterate in block order (default: the level's u[0])
int cgt_up(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* rhs, int nPost, double alpha, double* dst, const double* src,
           CgtChk* chk) {
  const int n = (int)h->lv.size();
  Level& l = h->lv[k];
  Level& c = h->lv[k + 1];
  const CgtDev& g = *l.S->cgt;
  CgtChain ch;
  ch.src = src ? src : l.u[0];
  ch.src_ext = false;
  ch.b = rhs;
  ch.b_ext = (k == 0) || !l.native_io;
  ch.dst = dst;
  ch.dst_ext = (k == 0) || !l.native_io;
  // launch 0 consumes the source and writes tmp; launch 1 may then overwrite the source, and so on
  ch.t0 = l.tmp;
  ch.t1 = const_cast<double*>(ch.src);
  ch.gs = 2;  // post-smoothing in the reverse colour order: the cycle stays symmetric
  CgtArgs first, none;
  std::memset(&first, 0, sizeof(first));
  std::memset(&none, 0, sizeof(none));
  first.tin = cgt_xfer(*l.tc, c.native_io);
  first.uc = (k + 1 == n - 1) ? c.u[0] : c.u[1];
  return cgt_run(ctx, g, ch, l.damp_post(alpha), nPost, first, none, AGGMG_KIND_FUSED_UP, k, chk, l.cdict.get());
}

// Between two cycles of multigrid()'s loop (src/solvers.jl:124-126) the fine level post-smooths and then
// pre-smooths the same iterate with the same right-hand side: prolongation-add, nPost + nPre sweeps,
// residual and restriction in ONE launch -- the fine operator is read once per cycle instead of twice.
// cur -> alt, both in block order; b is the caller's vector.
int cgt_mid(aggmg_ctx* ctx, aggmg_hier* h, const double* cur, double* alt, const double* b, int nsweeps, double alpha,
            CgtChk* chk) {
  const int n = (int)h->lv.size();
  Level& l = h->lv[0];
  Level& c = h->lv[1];
  const CgtDev& g = *l.S->cgt;
  CgtChain ch;
  ch.src = cur;
  ch.src_ext = false;
  ch.b = b;
  ch.b_ext = true;
  ch.dst = alt;
  ch.dst_ext = false;
  ch.t0 = l.tmp;
  WorkLease t1;   // (held across cgt_run)
  if (nsweeps > 2 * cgt_max_sweeps(g.m, g.sw)) {
    CHECK(scratch_lease(ctx, kScratchPing, g.ne * g.m, "cgt_mid", &t1));
    ch.t1 = t1;
  }
  CgtArgs first, last;
  std::memset(&first, 0, sizeof(first));
  std::memset(&last, 0, sizeof(last));
  first.tin = cgt_xfer(*l.tc, c.native_io);
  first.uc = (1 == n - 1) ? c.u[0] : c.u[1];
  last.do_residual = 1;
  last.tout = cgt_xfer(*l.tc, c.native_io);
  last.rc_out = c.rhs;
  return cgt_run(ctx, g, ch, l.damp_mid(alpha), nsweeps, first, last, AGGMG_KIND_FUSED_MID, 0, chk, l.cdict.get());
}

// ---- K columns per launch: the halves of a chain level of the K-column cycle (the launcher: above, beside cgt_launch) ----
// what the two halves share: nsweeps sweeps from uin into uout with right-hand sides rhs, kc columns, the coarse result
// uc to prolong from or the restricted residuals rc to write (a null view: none)
static CgtMultiArgs cgt_multi_args(const CgtDev& g, int nsweeps, int kc, ColsIn uin, ColsIn rhs, ColsOut uout, ColsIn uc, ColsOut rc) {
  CgtMultiArgs m;
  std::memset(&m, 0, sizeof(m));
  m.a = cgt_args(g);
  m.a.nsweeps = nsweeps;
  m.a.u_in = uin.p;
  m.a.b = rhs.p;
  m.a.u_out = uout.p;
  m.a.uc = uc.p;
  m.a.rc_out = rc.p;
  multi_strides(m, kc, uin, rhs, uout, uc, rc);
  return m;
}

// descending half of kc columns on a fused chain level: nPre sweeps from uin (level 0 only: the caller's X0; null --
// zero), residual, restriction into the next level's right-hand sides; the pre-smoothed iterates go to the level's u in
// block order.  The ext flags are cgt_down's.
int cgt_multi_down(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn uin, ColsIn rhs, int nPre, double alpha, int kc) {
  Level& l = h->lv[k];
  const CgtDev& g = *l.S->cgt;
  CgtMultiArgs m = cgt_multi_args(g, nPre, kc, uin, rhs, multi_vec(h, k, &LevelCols::u), ColsIn(), multi_vec(h, k + 1, &LevelCols::rhs));
  m.a.ext = (uin.p ? kExtUin : 0) | ((k == 0 || !l.native_io) ? kExtB : 0);
  m.a.do_residual = 1;
  m.a.tout = cgt_xfer(*l.tc, h->lv[k + 1].native_io);
  cgt_dictionary(m.a, g, l.cdict.get());
  ProfScope ps(ctx, AGGMG_KIND_FUSED_DOWN, k);
  return cgt_multi_launch(ctx, g, m, l.damp_pre(alpha).launch(nPre));
}

// ascending half: prolongation-add of the coarse result onto the pre-smoothed iterates (the level's u, block order), nPost
// sweeps, into dst -- the caller's numbering at level 0 and on a level whose vectors are not kept in block order, as cgt_up
int cgt_multi_up(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn rhs, int nPost, double alpha, ColsOut dst, int kc) {
  Level& l = h->lv[k];
  const CgtDev& g = *l.S->cgt;
  CgtMultiArgs m = cgt_multi_args(g, nPost, kc, multi_vec(h, k, &LevelCols::u), rhs, dst, multi_coarse_result(h, k), ColsOut());
  m.a.ext = ((k == 0) || !l.native_io) ? (kExtB | kExtUout) : 0;
  m.a.tin = cgt_xfer(*l.tc, h->lv[k + 1].native_io);
  cgt_dictionary(m.a, g, l.cdict.get());
  ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, k);
  return cgt_multi_launch(ctx, g, m, l.damp_post(alpha).launch(nPost));
}

// ---- compulsory bytes: what the arrays of a launch hold, each read or written once -------------
static int64_t cgt_operator_bytes(const CgtDev& g, bool sweeps) {
  const int64_t D = sizeof(double), rows = g.ne * g.m;
  int64_t r = rows * g.m * D + g.ne * g.m * D + rows * D;    // dblk, subrow, supcol
  if (sweeps && g.sw) r += rows * (g.m + 1) * D + g.ne * (g.m + 1) * D;   // element inverses (Schwarz / element Gauss-Seidel)
  return r;
}
static int64_t cgt_xfer_bytes(const TransferCgt& t, const CgtDev& g) {
  const int64_t D = sizeof(double), rows = g.ne * g.m;
  return t.type == kTrChain ? rows * (t.mc + 1) * D : rows * t.mc * D + g.ne * t.mc * D;
}

int cgt_op_launch_bytes(const CgtDev& g, bool sweeps, int64_t* rd, int64_t* wr) {
  const int64_t D = sizeof(double);
  *rd = cgt_operator_bytes(g, sweeps) + 2 * g.N * D + (g.affine ? 0 : g.ne * g.m * 4);   // u and b in the caller's numbering
  *wr = g.N * D;
  return AGGMG_OK;
}

int cgt_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, bool down, bool up, bool has_x0, int64_t* rd, int64_t* wr) {
  const Level& l = h->lv[level];
  const Level& c = h->lv[level + 1];
  if (!l.S || !l.S->cgt || !l.tc) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_hier_launch_bytes: not a fused chain level");
  const CgtDev& g = *l.S->cgt;
  const int64_t D = sizeof(double), rows = g.ne * g.m;
  const bool ext = (level == 0) || !l.native_io;
  const int64_t vec = ext ? g.N : rows;
  int64_t r = cgt_operator_bytes(g, true) + vec * D, w = 0;            // operator, right-hand side
  if (up || has_x0) r += (up ? rows : g.N) * D;                        // iterate in (block order inside the hierarchy)
  if (ext && !g.affine) r += rows * 4;                                 // block order -> caller's numbering
  r += cgt_xfer_bytes(*l.tc, g);                                       // rows of L (either direction; once when both)
  const int64_t nc = l.tc->nec * l.tc->mc;
  const bool cp = l.tc->type == kTrChain && !c.native_io && l.tc->cperm;
  if (up) r += nc * D + (cp ? nc * 4 : 0);                             // coarse iterate
  if (down) w += nc * D;                                               // restricted residual
  if (down && !up && cp) r += nc * 4;
  w += (up && !down ? vec : rows) * D;                                 // iterate out
  *rd = r;
  *wr = w;
  return AGGMG_OK;
}

// the same for a launch of ncols columns (cgt_multi_down / cgt_multi_up): the operator and transfer arrays and the index
// arrays once, every vector once per column; at ncols = 1 the figures of cgt_launch_bytes
int cgt_multi_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, bool down, bool has_x0, int64_t ncols, int64_t* rd, int64_t* wr) {
  const Level& l = h->lv[level];
  const Level& c = h->lv[level + 1];
  if (!l.S || !l.S->cgt || !l.tc) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_hier_multi_launch_bytes: not a fused chain level");
  const CgtDev& g = *l.S->cgt;
  const int64_t D = sizeof(double), rows = g.ne * g.m;
  const bool up = !down;
  const bool ext = (level == 0) || !l.native_io;
  const int64_t vec = ext ? g.N : rows;
  const int64_t nc = l.tc->nec * l.tc->mc;
  const bool cp = l.tc->type == kTrChain && !c.native_io && l.tc->cperm;
  int64_t once = cgt_operator_bytes(g, true) + cgt_xfer_bytes(*l.tc, g);   // operator, rows of L
  if (ext && !g.affine) once += rows * 4;                                  // block order -> caller's numbering
  if (cp) once += nc * 4;                                                  // coarse block order -> caller's numbering
  int64_t r = vec * D, w = 0;                                              // per column: right-hand side
  if (up || has_x0) r += (up ? rows : g.N) * D;                            // iterate in
  if (up) r += nc * D;                                                     // coarse iterate
  if (down) w += nc * D;                                                   // restricted residual
  w += (up ? vec : rows) * D;                                              // iterate out
  *rd = once + ncols * r;
  *wr = ncols * w;
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int aggmg_jacobi_setup_elements(aggmg_ctx* ctx, aggmg_op* A, int64_t nodes_per_element, int64_t n_elements,
                                           const int64_t* element_nodes, int one_based, aggmg_smoother** out) {
  if (!ctx || !A || !out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_jacobi_setup_elements: NULL argument");
  const bool lists = element_nodes && n_elements > 0 && nodes_per_element >= 2;
  const bool detect = ctx->detect_chain;
  if (lists) ctx->detect_chain = false;   // the caller's lists decide, not the pattern
  const int st0 = aggmg_jacobi_setup(ctx, A, out);
  ctx->detect_chain = detect;
  CHECK(st0);
  if (!lists) return AGGMG_OK;
  std::unique_ptr<aggmg_smoother> sm(*out);
  *out = nullptr;
  CHECK(cgt_build(ctx, sm.get(), element_nodes, nodes_per_element, n_elements, one_based));
  *out = sm.release();
  return AGGMG_OK;
}
