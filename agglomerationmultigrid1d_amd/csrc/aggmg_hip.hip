// libaggmg_hip.so -- host side of the C ABI declared in include/aggmg_hip.h.
//
// What lives here: the context, operator / smoother / hierarchy handles, launch logic for the kernels
// in kernels.hpp, the on-device V-cycle driver, the outer solver loops and the HIP-event profiler.
// Set-up (upload, block LU, structured forms, cyclic-reduction factors) runs on the device: setup.hip;
// the CG chain path: cgt.hip; element-partitioned runs: dist.hip; sparse set-up products: spops.hip.
// No CPU compute fallback exists: every hot-path entry point launches HIP kernels or fails.
#include "internal.hpp"
#include "multi_kernels.hpp"
#include "multi_elem_kernels.hpp"
#include "multi_solve_kernels.hpp"
#include "pair_kernels.hpp"
#include "patch_kernels.hpp"
#include "patch_multi_kernels.hpp"
#include "patch_schwarz_multi_kernels.hpp"
#include "elem_kernels.hpp"
#include "pair_elem_kernels.hpp"
#include "krylov_kernels.hpp"
#include "host_gmres.hpp"
#include "host_gmres_cols.hpp"

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
extern "C" const char* aggmg_version(void) { return "aggmg_hip 0.1 gfx950 fp64"; }

extern "C" int aggmg_debug_device_memory(int64_t* live_allocations, int64_t* live_bytes) {
  if (live_allocations) *live_allocations = DevMemLive::allocations.load();
  if (live_bytes) *live_bytes = DevMemLive::bytes.load();
  return AGGMG_OK;
}

extern "C" int aggmg_create(int device_id, aggmg_ctx** out) {
  if (!out) return fail(nullptr, AGGMG_ERR_ARGUMENT, "aggmg_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, AGGMG_ERR_HIP,
                std::string("aggmg_create: no HIP device available (") + hipGetErrorString(e) + ")");
  if (device_id < 0 || device_id >= ndev)
    return fail(nullptr, AGGMG_ERR_ARGUMENT, "aggmg_create: device_id out of range");
  e = hipSetDevice(device_id);
  if (e != hipSuccess) return fail(nullptr, AGGMG_ERR_HIP, hipGetErrorString(e));
  aggmg_ctx* ctx = new aggmg_ctx();
  ctx->device = device_id;
  e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete ctx;
    return fail(nullptr, AGGMG_ERR_HIP, hipGetErrorString(e));
  }
  ctx->stream = ctx->own_stream;
  *out = ctx;
  return AGGMG_OK;
}

extern "C" int aggmg_destroy(aggmg_ctx* ctx) {
  if (!ctx) return AGGMG_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& pe : ctx->prof) {
    (void)hipEventDestroy(pe.a);
    (void)hipEventDestroy(pe.b);
  }
  for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
  for (auto& L : ctx->stage) {
    for (int k = 0; k < 2; ++k) {
      if (L.ev[k]) (void)hipEventDestroy(L.ev[k]);
      if (L.pin[k]) (void)hipHostFree(L.pin[k]);
    }
    if (L.stream) (void)hipStreamDestroy(L.stream);
  }
  for (auto& r : ctx->pinned) {
    if (r.owned) (void)hipHostFree(r.base);
    else (void)hipHostUnregister(r.base);
  }
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;   // frees the context's device work space
  return AGGMG_OK;
}

// ---- page-locked host memory kept across calls (the host-pointer entry's fast path) ------------------------------
static bool host_is_pinned(const aggmg_ctx* ctx, const void* p, size_t bytes) {
  const char* c = static_cast<const char*>(p);
  for (const auto& r : ctx->pinned)
    if (c >= r.base && c + bytes <= r.base + r.bytes) return true;
  return false;
}

extern "C" int aggmg_host_register(aggmg_ctx* ctx, void* ptr, int64_t nbytes) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!ptr || nbytes <= 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_host_register: NULL pointer or empty range");
  HIPCHK(hipSetDevice(ctx->device));
  if (host_is_pinned(ctx, ptr, (size_t)nbytes)) return AGGMG_OK;
  HIPCHK(hipHostRegister(ptr, (size_t)nbytes, hipHostRegisterDefault));
  ctx->pinned.push_back({static_cast<char*>(ptr), (size_t)nbytes, false});
  return AGGMG_OK;
}

extern "C" int aggmg_host_unregister(aggmg_ctx* ctx, void* ptr) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  for (size_t i = 0; i < ctx->pinned.size(); ++i)
    if (ctx->pinned[i].base == static_cast<char*>(ptr) && !ctx->pinned[i].owned) {
      HIPCHK(hipStreamSynchronize(ctx->stream));   // no copy of ours may still be reading it
      HIPCHK(hipHostUnregister(ptr));
      ctx->pinned.erase(ctx->pinned.begin() + (long)i);
      return AGGMG_OK;
    }
  return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_host_unregister: not a range registered with this context");
}

extern "C" int aggmg_host_alloc(aggmg_ctx* ctx, int64_t nbytes, void** out) {
  if (!ctx || !out) return AGGMG_ERR_ARGUMENT;
  if (nbytes < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_host_alloc: negative size");
  HIPCHK(hipSetDevice(ctx->device));
  void* p = nullptr;
  HIPCHK(hipHostMalloc(&p, (size_t)std::max<int64_t>(nbytes, 8), hipHostMallocDefault));
  ctx->pinned.push_back({static_cast<char*>(p), (size_t)std::max<int64_t>(nbytes, 8), true});
  *out = p;
  return AGGMG_OK;
}

extern "C" int aggmg_host_free(aggmg_ctx* ctx, void* ptr) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!ptr) return AGGMG_OK;
  for (size_t i = 0; i < ctx->pinned.size(); ++i)
    if (ctx->pinned[i].base == static_cast<char*>(ptr) && ctx->pinned[i].owned) {
      HIPCHK(hipStreamSynchronize(ctx->stream));
      HIPCHK(hipHostFree(ptr));
      ctx->pinned.erase(ctx->pinned.begin() + (long)i);
      return AGGMG_OK;
    }
  return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_host_free: not an allocation of this context");
}

extern "C" const char* aggmg_last_error(aggmg_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" int aggmg_set_stream(aggmg_ctx* ctx, void* hip_stream) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  ctx->stream = (hipStream_t)hip_stream;  // NULL is the device's default (null) stream
  return AGGMG_OK;
}

extern "C" int aggmg_reset_stream(aggmg_ctx* ctx) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  ctx->stream = ctx->own_stream;
  return AGGMG_OK;
}

extern "C" int aggmg_set_option(aggmg_ctx* ctx, int option, int value) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  switch (option) {
    case AGGMG_OPT_SYMMETRIC_PACKING:
      ctx->sym_packing = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_COARSE_CHUNK_LOG2:
      if (value < 1 || value > kCrMaxStageLevels)
        return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_set_option: AGGMG_OPT_COARSE_CHUNK_LOG2 takes 1 .. 12");
      ctx->cr_max_q = value;
      return AGGMG_OK;
    case AGGMG_OPT_DETECT_CHAIN:
      ctx->detect_chain = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_PAIR_LEVELS:
      ctx->pair_levels = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_MG_CHECKPOINT:
      ctx->mg_checkpoint = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_SYMMETRIC_RESIDUAL:
      ctx->sym_residual = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_OPERATOR_DICTIONARY:
      ctx->op_dict = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_ELEMENT_THREADS:
      ctx->elem_threads = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_PAIR_ELEMENT_THREADS:
      ctx->pair_elem_threads = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_REPLAY_PRESMOOTH:
      ctx->replay_presmooth = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_ELEMENT_RECORDS_LDS:
      if (value < 0 || value > kElemRecMaxClasses)
        return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_set_option: AGGMG_OPT_ELEMENT_RECORDS_LDS takes 0 .. " + std::to_string(kElemRecMaxClasses));
      ctx->elem_rec_cap = value;
      return AGGMG_OK;
    case AGGMG_OPT_COARSE_DICTIONARY:
      if (value < 0 || value > kCrDictMaxClasses)
        return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_set_option: AGGMG_OPT_COARSE_DICTIONARY takes 0 .. " + std::to_string(kCrDictMaxClasses));
      ctx->coarse_dict_cap = value;
      return AGGMG_OK;
    case AGGMG_OPT_PATCH_MULTI:
      ctx->patch_multi = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_CHAIN_MULTI:
      ctx->chain_multi = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_PATCH_SCHWARZ_MULTI:
      ctx->patch_schwarz_multi = value != 0;
      return AGGMG_OK;
    case AGGMG_OPT_MULTI_ELEMENT_THREADS:
      ctx->multi_elem_threads = value != 0;
      return AGGMG_OK;
  }
  return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_set_option: unknown option");
}

extern "C" int aggmg_synchronize(aggmg_ctx* ctx) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

extern "C" int aggmg_dev_alloc(aggmg_ctx* ctx, int64_t nbytes, void** out) {
  if (!ctx || !out || nbytes < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_dev_alloc: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMalloc(out, (size_t)std::max<int64_t>(nbytes, 8)));
  HIPCHK(hipMemsetAsync(*out, 0, (size_t)std::max<int64_t>(nbytes, 8), ctx->stream));   // zeroed: a fresh vector is a zero guess
  return AGGMG_OK;
}

extern "C" int aggmg_dev_free(aggmg_ctx* ctx, void* ptr) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (ptr) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipFree(ptr));
  }
  return AGGMG_OK;
}

extern "C" int aggmg_memcpy_h2d(aggmg_ctx* ctx, void* dst, const void* src, int64_t nbytes) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

extern "C" int aggmg_memcpy_d2h(aggmg_ctx* ctx, void* dst, const void* src, int64_t nbytes) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

extern "C" int aggmg_profile_enable(aggmg_ctx* ctx, int on) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  ctx->profiling = on < 0 ? 0 : (on > 2 ? 1 : on);
  return AGGMG_OK;
}

extern "C" int aggmg_profile_collect(aggmg_ctx* ctx, double* total_ms, int64_t* counts) {
  if (!ctx || !total_ms || !counts) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_profile_collect: NULL");
  for (int t = 0; t < AGGMG_PROFILE_NTAGS; ++t) {
    total_ms[t] = 0.0;
    counts[t] = 0;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (auto& pe : ctx->prof) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, pe.a, pe.b));
    total_ms[pe.tag] += ms;
    counts[pe.tag] += 1;
    ctx->ev_pool.push_back(pe.a);
    ctx->ev_pool.push_back(pe.b);
  }
  ctx->prof.clear();
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// operators
// ---------------------------------------------------------------------------------------------
extern "C" int aggmg_csc_upload(aggmg_ctx* ctx, int64_t m, int64_t n, const int64_t* colptr,
                                const int64_t* rowval, const double* nzval, int one_based, int kind,
                                aggmg_op** out) {
  if (!ctx || !out || !colptr) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: NULL argument");
  *out = nullptr;
  if (m < 0 || n < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: negative dimension");
  const int64_t base = one_based ? 1 : 0;
  const int64_t nnz = colptr[n] - base;
  const int64_t lim = (int64_t)1 << 31;
  if (m >= lim || n >= lim || nnz >= lim)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: dimension or nnz >= 2^31 (int32 device indices)");
  if (nnz < 0 || (nnz > 0 && (!rowval || !nzval)))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: inconsistent colptr / NULL arrays");
  if (kind != AGGMG_OP_STIFFNESS && kind != AGGMG_OP_TRANSFER)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: unknown kind");
  HIPCHK(hipSetDevice(ctx->device));
  // the arrays go to the device as they are; validation, the Int64 -> int32 conversion and everything
  // derived from them later (smoother blocks, structured forms, the row-gather CSR where a generic
  // kernel needs it) are computed there (setup.hip)
  auto op = std::make_unique<aggmg_op>();
  op->m = m;
  op->n = n;
  op->nnz = nnz;
  op->kind = kind;
  CHECK(setup_csc_upload(ctx, m, n, colptr, rowval, nzval, one_based, &op->csc));
  *out = op.release();
  return AGGMG_OK;
}

extern "C" int aggmg_op_free(aggmg_ctx* ctx, aggmg_op* op) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!op) return AGGMG_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  delete op;  // the destructor frees the device arrays
  return AGGMG_OK;
}

extern "C" int aggmg_op_shape(aggmg_ctx* ctx, const aggmg_op* op, int64_t* m, int64_t* n, int64_t* nnz) {
  if (!ctx || !op) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_op_shape: NULL");
  if (m) *m = op->m;
  if (n) *n = op->n;
  if (nnz) *nnz = op->nnz;
  return AGGMG_OK;
}

extern "C" int aggmg_op_download(aggmg_ctx* ctx, const aggmg_op* op_, int transposed, int32_t* rowptr,
                                 int32_t* colind, double* vals) {
  if (!ctx || !op_) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_op_download: NULL");
  aggmg_op* op = const_cast<aggmg_op*>(op_);
  if (transposed && op->kind != AGGMG_OP_TRANSFER)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_op_download: orientation not stored for this op");
  if (!transposed) CHECK(op_ensure_csr(ctx, op));  // the row-gather form is built on first use
  const CsrDev& d = transposed ? op->csc : op->csr;
  if (rowptr) HIPCHK(hipMemcpyAsync(rowptr, d.rowptr, (d.nrows + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (colind && d.nnz) HIPCHK(hipMemcpyAsync(colind, d.colind, d.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (vals && d.nnz) HIPCHK(hipMemcpyAsync(vals, d.vals, d.nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

// (kept for ABI compatibility: the library holds no host copy of an operator any more)
extern "C" int aggmg_op_release_host(aggmg_ctx* ctx, aggmg_op* op) {
  if (!ctx || !op) return AGGMG_ERR_ARGUMENT;
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// smoothers (set-up on the device: setup.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int aggmg_blockjacobi_setup(aggmg_ctx* ctx, aggmg_op* A, int64_t m, int64_t nb,
                                       const int64_t* blockinds, int one_based, int kind,
                                       aggmg_smoother** out) {
  if (!ctx || !A || !out || !blockinds) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_blockjacobi_setup: NULL argument");
  *out = nullptr;
  if (A->m != A->n) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_blockjacobi_setup: operator is not square");
  if (m <= 0 || nb < 0 || m > 64) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_blockjacobi_setup: block size must be in 1..64");
  if (kind < 0 || kind > 2) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_blockjacobi_setup: unknown kind");
  if (nb * m >= ((int64_t)1 << 31)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_blockjacobi_setup: nb * m >= 2^31");
  HIPCHK(hipSetDevice(ctx->device));
  auto sm = std::make_unique<aggmg_smoother>();
  sm->kind = kind == 1 ? 2 : 1;  // (kind 2, block Gauss-Seidel, shares the block data of kind 0)
  sm->A = A;
  sm->N = A->m;
  sm->m = m;
  sm->nb = nb;
  // index lists -> blocks A[inds, inds] -> pivoted LU -> inverses, and the fused block-tridiagonal form where
  // the lists are contiguous and the operator fits (hybrid Schwarz never takes the fused form)
  CHECK(setup_block_smoother(ctx, sm.get(), blockinds, one_based, sm->kind == 1));
  // overlapping element blocks of a CG mesh (cg_smoother :addSchwarz / :hybridSchwarz): the lists are the
  // element chain -- the sweeps then run in the fused chain kernel (apply_smoother keeps the generic kernel);
  // kind 2 on such lists: red-black ELEMENT Gauss-Seidel (extension), fused chain kernel only
  if (!sm->btd && m >= 2 && m <= 9 && nb >= 1 && A->m == nb * (m - 1) + 1) {
    CHECK(cgt_build(ctx, sm.get(), blockinds, m, nb, one_based));
    if (sm->cgt) CHECK(cgt_attach_schwarz(ctx, sm.get(), kind == 2 ? 3 : (kind == 1 ? 2 : 1)));
    if (sm->cgt && !sm->cgt->sw) {  // (not attached: no point-Jacobi chain for a block smoother)
      sm->cgt.reset();
      A->cgt.reset();
    }
  }
  if (kind == 2) {
    // two colours order a sweep only when elements couple to their direct neighbours alone
    if (!sm->btd && !sm->cgt) {  // reachable with ordinary input; sm's destructor releases what was allocated
      return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                  "aggmg_blockjacobi_setup: red-black block Gauss-Seidel needs contiguous blocks and a "
                  "block-tridiagonal operator, or the element chain of a CG mesh");
    }
    sm->gs = true;
  }
  *out = sm.release();
  return AGGMG_OK;
}

// BlockDiagonal / BlockDiagonalLU (src/block_diagonal.jl:11-21): a block-diagonal matrix given by its
// dense blocks, applied (mul!, :166-176) or solved with (ldiv!, :299-309) through the same batched
// small-block kernel as the block smoother.  blocks: nb blocks of m x m, each column-major (a Julia
// Matrix{Float64}); contiguous aligned index lists as the BlockDiagonal(mBlocks) constructor makes.
extern "C" int aggmg_blockdiag_setup(aggmg_ctx* ctx, int64_t m, int64_t nb, const double* blocks, int factorize,
                                     aggmg_smoother** out) {
  if (!ctx || !out || (!blocks && nb > 0)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_blockdiag_setup: NULL argument");
  *out = nullptr;
  if (m <= 0 || m > 64 || nb < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_blockdiag_setup: block size must be in 1..64");
  if (m * nb >= ((int64_t)1 << 31)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_blockdiag_setup: size >= 2^31");
  HIPCHK(hipSetDevice(ctx->device));
  auto sm = std::make_unique<aggmg_smoother>();
  sm->kind = 1;
  sm->A = nullptr;
  sm->N = m * nb;
  sm->m = m;
  sm->nb = nb;
  sm->contiguous = true;
  std::vector<int32_t> inds((size_t)nb * m);
  for (int64_t i = 0; i < nb * m; ++i) inds[i] = (int32_t)i;
  CHECK(sm->inds.upload(ctx, inds));
  CHECK(sm->binv.alloc(ctx, nb * m * m));
  if (factorize) {
    DevArray<double> raw;  // the column-major blocks as given; inverted on the device (K6)
    CHECK(raw.alloc(ctx, nb * m * m));
    if (nb) HIPCHK(hipMemcpyAsync(raw, blocks, (size_t)nb * m * m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    int64_t sing = -1;
    CHECK(setup_invert_blocks(ctx, nb, (int)m, raw, 1, sm->binv, &sing));
    if (sing >= 0)
      return fail(ctx, AGGMG_ERR_SINGULAR, "aggmg_blockdiag_setup: singular block " + std::to_string(sing + 1) + " (SingularException)");
  } else {
    std::vector<double> mats((size_t)nb * m * m);
    for (int64_t k = 0; k < nb; ++k)
      for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < m; ++j) mats[k * m * m + i * m + j] = blocks[k * m * m + j * m + i];  // column- to row-major
    if (nb) HIPCHK(hipMemcpyAsync(sm->binv, mats.data(), mats.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  *out = sm.release();
  return AGGMG_OK;
}

extern "C" int aggmg_jacobi_setup(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother** out) {
  if (!ctx || !A || !out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_jacobi_setup: NULL argument");
  *out = nullptr;
  if (A->m != A->n) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_jacobi_setup: operator is not square");
  HIPCHK(hipSetDevice(ctx->device));
  auto sm = std::make_unique<aggmg_smoother>();
  sm->kind = 0;
  sm->A = A;
  sm->N = A->m;
  CHECK(setup_jacobi_diag(ctx, A, &sm->diag));  // A[i,i], 0.0 when not stored
  if (ctx->detect_chain) CHECK(cgt_detect(ctx, sm.get()));   // AGGMG_OPT_DETECT_CHAIN
  *out = sm.release();
  return AGGMG_OK;
}

extern "C" int aggmg_smoother_free(aggmg_ctx* ctx, aggmg_smoother* sm) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!sm) return AGGMG_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  delete sm;  // the destructor frees the device arrays
  return AGGMG_OK;
}

extern "C" int aggmg_smoother_is_structured(aggmg_ctx* ctx, const aggmg_smoother* sm, int* out) {
  if (!ctx || !sm || !out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_is_structured: NULL");
  *out = (sm->btd || sm->cgt || sm->patch) ? 1 : 0;
  return AGGMG_OK;
}

// an integer tuning knob from the environment
static int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : dflt;
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
template <int MODE>
static int launch_csr(aggmg_ctx* ctx, const CsrDev& A, const double* x, const double* b, const double* dg,
                      double alpha, double* y) {
  if (A.nrows == 0) return AGGMG_OK;
  // (single passes stay on the stream kernel also for banded operators: measured on the config-2 matrix, the window
  // kernel's extra LDS and barrier make one sweep 121 us against 105 us; it pays from two sweeps per launch on)
  // every row short: one thread per row, no LDS staging -- AGGMG_CSR_ROWTHREAD=1 (the default until the stream kernel's
  // blocks were reshaped: 92 us against its 75 us on config 2's residual; kept for A/B runs, the same bits)
  static const bool rowthread = env_int("AGGMG_CSR_ROWTHREAD", 0) != 0;
  if (rowthread && A.maxrow >= 0 && A.maxrow <= kRowThreadMax && A.nrows < ((int64_t)1 << 31) * kThreads) {
    const unsigned nb = (unsigned)((A.nrows + kThreads - 1) / kThreads);
    static const bool bandrow = env_int("AGGMG_CSR_BANDROW", 1) != 0;
    if (bandrow && A.bw >= 0 && A.bw <= kBandMaxBw && A.nrows == A.ncols && y != x)   // banded: the x window through LDS
      hipLaunchKernelGGL((csr_rowthread_band_kernel<MODE>), dim3(nb), dim3(kThreads), 0, ctx->stream, A.view(), A.bw, x, b, dg, alpha, y);
    else
      hipLaunchKernelGGL((csr_rowthread_kernel<MODE>), dim3(nb), dim3(kThreads), 0, ctx->stream, A.view(), x, b, dg, alpha, y);
    HIPCHK(hipGetLastError());
    return AGGMG_OK;
  }
  if (A.rowblk) {
    hipLaunchKernelGGL((csr_stream_kernel<MODE>), dim3((unsigned)A.nblk), dim3(kThreads), 0, ctx->stream, A.view(),
                       (const int32_t*)A.rowblk, x, b, dg, alpha, y);
    HIPCHK(hipGetLastError());
    return AGGMG_OK;
  }
  const int lpr = A.lpr;
  const int64_t rows_per_block = kThreads / lpr;
  const int64_t nblk = (A.nrows + rows_per_block - 1) / rows_per_block;
  if (nblk >= ((int64_t)1 << 31)) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "grid too large");
  dim3 grid((unsigned)nblk), block(kThreads);
  CsrView v = A.view();
  if (!with_block_size<csr_lanes_form, 64>(lpr, [&](auto l) {
        hipLaunchKernelGGL((csr_row_kernel<decltype(l)::value, MODE>), grid, block, 0, ctx->stream, v, x, b, dg, alpha, y);
      }))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "bad lanes-per-row");
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// n point-Jacobi sweeps u <- u + alpha D^-1 (b - A u) from src into dst (dst != src; tmp: a second vector of the
// same length, may be clobbered).  Banded operators take up to their band_sweeps (<= kBandSweeps) sweeps per launch (csr_band_kernel), the
// others one; the launches ping-pong so that the last one lands in dst.
// rout / fused (optional): the residual b - A dst wanted next -- a banded operator's last launch forms it in the same pass
// (one sweep less per launch so that the halo holds) and *fused says so; otherwise the caller launches it.
static int launch_csr_jacobi_sweeps(aggmg_ctx* ctx, const CsrDev& A, const double* src, const double* b, const double* dg,
                                    Damping alpha, int n, double* dst, double* tmp, double* rout = nullptr, bool* fused = nullptr) {
  if (fused) *fused = false;
  if (n <= 0 || A.nrows == 0) return AGGMG_OK;
  const bool want_r = rout && fused && A.bandblk && A.band_sweeps >= 2;
  const int per = A.bandblk ? (want_r ? A.band_sweeps - 1 : A.band_sweeps) : 1;
  const int nl = (n + per - 1) / per;
  int left = n;
  for (int l = 0; l < nl; ++l) {
    // even out the sweeps over the launches (3 + 3 rather than 4 + 2: every launch pays its halo)
    const int s = (left + (nl - l) - 1) / (nl - l);
    double* out = ((nl - 1 - l) % 2 == 0) ? dst : tmp;
    if (out == src) return fail(ctx, AGGMG_ERR_ARGUMENT, "point-Jacobi sweeps: source and destination alias");
    const bool with_r = want_r && l == nl - 1;
    if (A.bandblk && (s > 1 || with_r)) {
      hipLaunchKernelGGL((csr_band_kernel<kJacobi>), dim3((unsigned)A.nbandblk), dim3(kThreads), 0, ctx->stream, A.view(),
                         (const int32_t*)A.bandblk, A.bw, s, src, b, dg, alpha.from(n - left).launch(s), out, with_r ? rout : (double*)nullptr);
      HIPCHK(hipGetLastError());
      if (with_r) *fused = true;
    } else {
      CHECK(launch_csr<kJacobi>(ctx, A, src, b, dg, alpha.at(n - left), out));
    }
    src = out;
    left -= s;
  }
  return AGGMG_OK;
}

template <int M, bool CMP>
struct BtdTile {
  // Threads per workgroup and slabs per thread.  A tile of TE = (NT / M) * NS elements wants to be
  // large (the halo costs 2 * halo / TE redundant work) while the per-thread register arrays
  // (NS x (2..3) x M doubles) must stay small enough for >= 6-7 waves per SIMD: the sweeps only hide
  // behind other workgroups' loads at that occupancy (measured: NS 4 -> 2 at M = 4 is 9 % per cycle).
#ifndef AGGMG_NT4
#define AGGMG_NT4 256
#endif
#ifndef AGGMG_NS4
#define AGGMG_NS4 2
#endif
#ifndef AGGMG_NS2
#define AGGMG_NS2 1
#endif
  static constexpr int NT = (M == 4) ? AGGMG_NT4 : kThreads;
  static constexpr int NS = (M == 1) ? 2 : (M == 2) ? AGGMG_NS2 : (M == 3) ? 3 : (M == 4) ? AGGMG_NS4 : (M <= 7) ? 3 : 2;
  static constexpr int EPS = NT / M;
  static constexpr int TE = EPS * NS;
  static constexpr int kM = M;
  static constexpr bool kCmp = CMP;
};

// Which tiles of a level a launch covers: all of them, only those holding elements [0, head) and
// [tail, ne) ("ends"), or only the others ("middle").
struct TileSel {
  int mode = 0;  // 0 all, 1 ends, 2 middle
  int64_t head = 0, tail = 0;
};

// the structured transfer of a level as the fused kernel's prolongation input / restriction output
static void xfer_in(FusedArgs& a, const TransferBtd& t) {
  a.lf1_in = t.lf1;
  a.mc_in = t.mc;
  a.rho_in = t.rho;
  a.par_in = t.rho ? nullptr : t.parent;
}
// agglomerates of different sizes: the elements a tile may move to stand on an agglomerate boundary (-1: none)
static int xfer_agg_shift(const TransferBtd& t) {
  // (AGGMG_AGG_ALIGN=0: the two-part atomic restriction for every size, as before r03)
  static const int max_shift = env_int("AGGMG_AGG_ALIGN", 1) ? 8 : -1;
  return (!t.rho && t.maxagg >= 1 && t.maxagg - 1 <= max_shift) ? t.maxagg - 1 : -1;
}
static void xfer_out(FusedArgs& a, const TransferBtd& t) {
  a.lf1_out = t.lf1;
  a.mc_out = t.mc;
  a.rho_out = t.rho;
  a.par_out = t.rho ? nullptr : t.parent;
  a.first_out = t.rho ? nullptr : t.first;
  a.nec_out = t.nec;
  a.agg_shift = xfer_agg_shift(t);
}

// A fused launch on the host: the kernel's argument struct and, beside it, the factors of its sweeps -- a kernel argument
// of their own (SweepWeights, kernels.hpp)
struct FusedLaunch : FusedArgs {
  SweepWeights wts;
  ElemRecTab rec = {nullptr, 0};   // the level's packed class records (DictDev::rec), set with the dictionary; or null
};

// What the element-thread kernel (elem_kernels.hpp) asks of a launch's arguments, on a level with compressed couplings
// and blocks of 4 rows: a dictionary launch of block-Jacobi sweeps -- at least one -- over all tiles of the level, two-mode
// transfers of equal agglomerates, a residual that is restricted and not stored.  (Its tile is the caller's to plan.)
static bool elem_thread_args(const aggmg_ctx* ctx, const FusedArgs& a, bool chk, int sel_mode) {
  return ctx->elem_threads && a.lv.cls && a.lv.bsym && !a.gs && !chk && a.nsweeps >= 1 && sel_mode == 0 && !a.r_out &&
         !a.par_in && !a.par_out && !a.ld_out && (!a.lf_in || a.mc_in == 2) && (!a.lf_out || a.mc_out == 2) &&
         (!a.do_residual || a.lf_out);
}
// ... and of those launches the ones that keep the class records in LDS (AGGMG_OPT_ELEMENT_RECORDS_LDS; btd_elem_rec_kernel,
// btd_elem_rec_replay_up_kernel): the level has its packed records, no more classes than the option allows, and a
// residual comes from the lossless symmetric form (the record holds no full rows)
static bool elem_record_args(const aggmg_ctx* ctx, const FusedLaunch& a) {
  return a.rec.rec && a.rec.nclasses >= 1 && a.rec.nclasses <= ctx->elem_rec_cap && (!a.do_residual || (a.lv.dup && a.lv.corr));
}

template <int M, bool CMP>
static int launch_btd_t(aggmg_ctx* ctx, FusedLaunch a, int halo, const TileSel& sel, CgtChk* chk_io) {
  using T = BtdTile<M, CMP>;
  const bool vr = (a.lf_out || a.ld_out) && a.par_out;
  const int align = ((a.lf_out || a.ld_out) && !vr) ? a.rho_out : 1;
  if (a.gs) halo += a.nsweeps;  // two half-sweeps per sweep, one element of halo each
  if (vr && (sel.mode == 1 || sel.mode == 2))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "tile selection on a level with agglomerates of different sizes");
  const bool chk = a.chk_part != nullptr;   // checkpoint variant (multigrid's per-cycle residual test inside the launch)
  // The element-thread kernel (elem_kernels.hpp, AGGMG_OPT_ELEMENT_THREADS) in place of the row-thread dictionary variant,
  // the one place that chooses: blocks of 4 rows, a dictionary launch (fused_dictionary's conditions, checked again
  // below) of block-Jacobi sweeps -- at least one -- over all tiles of the level, whose residual is restricted and not stored.
  // Its tile is one slab of kElemThreads elements, planned like any other.
  bool elem = false;
  if constexpr (M == 4 && CMP)
    elem = elem_thread_args(ctx, a, chk, sel.mode) && fused_tile_plan(kElemThreads, halo, align, vr, a.agg_shift).owned > 0;
  const FusedTilePlan plan = fused_tile_plan(elem ? kElemThreads : T::TE, halo, align, vr, a.agg_shift);   // host_plan.hpp
  a.agg_shift = plan.agg_shift;
  if (vr && plan.agg_shift < 0)   // agglomerates cut by a tile boundary are summed from two tiles
    HIPCHK(hipMemsetAsync(a.rc_out, 0, (size_t)a.nec_out * a.mc_out * sizeof(double), ctx->stream));
  const int owned = plan.owned;
  if (owned <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "fused tile too small for the requested halo");
  a.owned = owned;
  a.halo_left = plan.halo_left;
  const TileSubset sub = fused_tile_subset(a.lv.ne, owned, sel.mode == 3 ? 0 : sel.mode, sel.head, sel.tail);   // host_plan.hpp (3: every tile)
  const int64_t ntiles = sub.ntiles;
  a.tile_split = sub.split;
  a.tile_skip = sub.skip;
  if (chk_io) chk_io->ntiles = ntiles;
  if (ntiles == 0) return AGGMG_OK;
  if (chk && a.gs) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: checkpoint launch with Gauss-Seidel sweeps");
  // every tile stores its sums at chk_part[(checkpoint * ntiles + tile) * 2]: never past what was reserved
  if (chk && (!chk_io || ntiles > chk_io->cap))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: checkpoint launch of more tiles than its partial sums have room for");
  a.chk_tiles = ntiles;
  if (chk) {   // measurement aid (tools/exp_outer_loop.py): the checkpoint variant's code with no checkpoint ever due
    static const int never = env_int("AGGMG_CHK_NEVER", 0);
    if (never) {
      a.chk_sweep = 1 << 29;
      a.chk_final = 0;
    }
  }
  if (a.chk_stride < 1) a.chk_stride = 1 << 30;   // a single checkpoint, after chk_sweep sweeps
  // (checkpoint variant: + the wave sums of a reduction, + -- compressed couplings -- the thread-private slots the
  // residual rows' operator entries are parked in between a checkpoint and the later residuals of the launch)
  const size_t lds = (size_t)2 * (T::TE + 2) * M * sizeof(double) +
                     (chk ? ((size_t)2 * (T::NT / 64) + (CMP ? (size_t)T::NT * T::NS * (M + 1) : 0)) * sizeof(double) : 0);
  constexpr bool kGrp = btd_sym_form(M, CMP);
  const bool sym = kGrp && a.lv.bsym;
  // the lossless symmetric form of the residual's entries: block-Jacobi launches that form the explicit residual
  constexpr bool kSres = btd_sres_form(M, CMP);
  const bool sres = kSres && a.lv.dup && !a.gs && !chk && a.do_residual && (a.r_out || a.lf_out);
  // instantiations per (M, CMP): symmetric packing x (block-Jacobi / red-black GS / block-Jacobi with checkpoint)
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(T::NT), lds, ctx->stream, static_cast<const FusedArgs&>(a), a.wts);
  };
  if constexpr (kSres) {
    // the operator dictionary (fused_dictionary put its arrays in place of the full ones): block-Jacobi launches
    if (sym && a.lv.cls) {
      if (a.gs || chk) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: dictionary launch of a Gauss-Seidel / checkpoint variant");
      // the variant indexes the transfer's rows by class only on its two-mode, equal-agglomerate paths
      if (a.par_in || a.par_out || a.ld_out || (a.lf_in && a.mc_in != 2) || (a.lf_out && a.mc_out != 2))
        return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: dictionary launch with a transfer the variant does not index by class");
      if constexpr (M == 4) {
        if (elem && elem_record_args(ctx, a)) {
          auto go_rec = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(kElemThreads), elem_rec_lds_bytes<M>(a.rec.nclasses), ctx->stream,
                               static_cast<const FusedArgs&>(a), a.wts, a.rec);
          };
          if (a.do_residual)
            go_rec(btd_elem_rec_kernel<M, true>);
          else
            go_rec(btd_elem_rec_kernel<M, false>);
          HIPCHK(hipGetLastError());
          ++ctx->elem_launches;
          ++ctx->elem_rec_launches;
          return AGGMG_OK;
        }
        if (elem) {
          auto go_elem = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(kElemThreads), elem_lds_bytes<M>(), ctx->stream,
                               static_cast<const FusedArgs&>(a), a.wts);
          };
          if (sres)
            go_elem(btd_elem_dict_kernel<M, true>);
          else
            go_elem(btd_elem_dict_kernel<M, false>);
          HIPCHK(hipGetLastError());
          ++ctx->elem_launches;
          return AGGMG_OK;
        }
      }
      if (sres)
        go(btd_fused_kernel<M, CMP, T::NS, true, T::NT, false, false, true, true>);
      else
        go(btd_fused_kernel<M, CMP, T::NS, true, T::NT, false, false, false, true>);
      HIPCHK(hipGetLastError());
      return AGGMG_OK;
    }
  }
  if constexpr (kGrp) {
    if (sym) {
      if (a.gs)
        go(btd_fused_kernel<M, CMP, T::NS, true, T::NT, true>);
      else if (chk)
        go(btd_fused_kernel<M, CMP, T::NS, true, T::NT, false, true>);
      else if (sres)
        go(btd_fused_kernel<M, CMP, T::NS, true, T::NT, false, false, kSres>);
      else
        go(btd_fused_kernel<M, CMP, T::NS, true, T::NT, false>);
      HIPCHK(hipGetLastError());
      return AGGMG_OK;
    }
  }
  if (a.gs)
    go(btd_fused_kernel<M, CMP, T::NS, false, T::NT, true>);
  else if (chk)
    go(btd_fused_kernel<M, CMP, T::NS, false, T::NT, false, true>);
  else
    go(btd_fused_kernel<M, CMP, T::NS, false, T::NT, false>);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

template <int M, bool CMP>
static int btd_max_halo() {
  return (BtdTile<M, CMP>::TE - 8) / 2;
}

// f(BtdTile<M, CMP>()) for the form of btd_form (forms.hpp) that serves b; false when there is none.
template <class F>
static bool btd_with_tile(const BtdDev& b, F&& f) {
  return with_form<btd_form>(b.m, b.cmp, [&](auto t) { f(BtdTile<decltype(t)::kM, decltype(t)::kCmp>()); });
}

static int launch_btd(aggmg_ctx* ctx, const BtdDev& b, const FusedLaunch& a, int halo, const TileSel& sel = TileSel(),
                      CgtChk* chk = nullptr) {
  int rc = AGGMG_OK;
  if (!btd_with_tile(b, [&](auto t) { rc = launch_btd_t<decltype(t)::kM, decltype(t)::kCmp>(ctx, a, halo, sel, chk); }))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "block size not instantiated for the fused kernel");
  return rc;
}

static int btd_tile_elems(const BtdDev& b) {
  int te = 0;
  btd_with_tile(b, [&](auto t) { te = decltype(t)::TE; });
  return te;
}

static FusedArgs btd_args(const BtdDev& b) {
  FusedArgs a;
  std::memset(&a, 0, sizeof(a));
  a.lv = BtdLevel{b.binv, b.dblk, b.bsym, b.dup, b.corr, b.scol, b.pcol, b.qrow, b.sub, b.sup, b.P, b.Q, b.ne, b.c_sub, b.r_sup};
  return a;
}

// ---- the arguments of a fused launch, part by part: every launch has the sweeps; an ascent adds the prolongation in
// front of them, a descent the residual and its restriction behind them, a launch between two cycles both -----------
// gs: 0 block Jacobi, 1 red-black Gauss-Seidel even elements first, 2 odd ones first
static FusedLaunch fused_sweeps(const BtdDev& b, const double* u_in, const double* rhs, double* u_out, Damping alpha, int nsweeps,
                              int gs = 0) {
  FusedLaunch a;
  static_cast<FusedArgs&>(a) = btd_args(b);
  a.u_in = u_in;
  a.b = rhs;
  a.u_out = u_out;
  a.wts = alpha.launch(nsweeps);
  a.nsweeps = nsweeps;
  a.gs = gs;
  return a;
}
// u_in + L uc before the sweeps
static void fused_ascent(FusedArgs& a, const Level& l, const double* uc) {
  a.lf_in = l.tb->lf;
  a.uc = uc;
  xfer_in(a, *l.tb);
}
// lf applied to r, or (L'D) applied to B^{-1} r (the kernel then reads neither D nor L): the one place that chooses
static bool restrict_with_ld(const aggmg_hier* h, const Level& l) {
  return l.tb->ld && h->restriction == AGGMG_RESTRICT_PRECONDITIONED;
}
// rc = L' (b - A u) after the sweeps
static void fused_descent(FusedArgs& a, const aggmg_hier* h, const Level& l, double* rc) {
  a.do_residual = 1;
  if (restrict_with_ld(h, l))
    a.ld_out = l.tb->ld;
  else
    a.lf_out = l.tb->lf;
  a.rc_out = rc;
  xfer_out(a, *l.tb);
}
// The level's operator dictionary in place of its full arrays (after fused_ascent / fused_descent): the default-mode
// block-Jacobi launches of a cycle -- no checkpoint, no (L'D) restriction -- on a level that has one.  The variant reads
// the same bits from the dictionary (btd_fused_kernel<..., DICT = true>).
static void fused_dictionary(FusedLaunch& a, const Level& l) {
  const DictDev* d = l.dict.get();
  if (!d || a.gs || a.chk_part || a.ld_out || a.par_in || a.par_out || !a.lv.bsym) return;
  if ((a.lf_in && a.mc_in != 2) || (a.lf_out && a.mc_out != 2)) return;
  a.lv.bsym = d->bsym;
  a.lv.qrow = d->qrow;
  a.lv.qmir = d->qmir;
  a.lv.dup = d->dup;
  a.lv.corr = d->corr;
  a.lv.scol = d->scol;
  a.lv.dblk = d->dblk;
  a.lv.cls = d->cls;
  if (d->rec) a.rec = ElemRecTab{d->rec, d->nclasses};
  // (lf_in / lf_out also say that there is a prolongation / a restriction: never null then)
  if (a.lf_in) (d->lf_unit ? a.lf1_in : a.lf_in) = d->lf;
  if (a.lf_out) (d->lf_unit ? a.lf1_out : a.lf_out) = d->lf;
}
// Checkpoints of a launch (the checkpoint variants of the fused kernel and of the chain kernel): after `sweep`,
// sweep + stride, ... sweeps, and (final) after the last one; ntiles comes back from the launch.
static void fused_chk(FusedArgs& a, const CgtChk& c) {
  a.chk_sweep = c.sweep;
  a.chk_stride = c.stride;
  a.chk_final = c.final;
  a.chk_exact = c.exact;
  a.chk_part = c.part;
}

// Max sweeps fused into one launch: the halo costs 2*S/TE redundant work.
static int btd_max_sweeps(const BtdDev& b, int extra) {
  const int te = btd_tile_elems(b);
  int s = std::min(8, te / 8) - extra;
  return std::max(1, s);
}

// does a launch of nsweeps sweeps (+ a residual) fit the halo budget of smoother sm's tiles?
static bool btd_fits(const aggmg_smoother& sm, int nsweeps, int residual) {
  return (sm.gs ? 2 : 1) * nsweeps + residual <= btd_max_sweeps(*sm.btd, 0);
}

// ... and does that launch have a tile (host_plan.hpp, the planner launch_btd_t runs)?  tout: the transfer it restricts
// through, or null.  Where it has none the callers take their unfused sequence.
static bool btd_launch_ok(const aggmg_smoother& sm, int nsweeps, int residual, const TransferBtd* tout) {
  if (!btd_fits(sm, nsweeps, residual)) return false;
  TileQuery q;
  q.launch = kTileFused;
  q.te = btd_tile_elems(*sm.btd);
  q.halo = (sm.gs ? 2 : 1) * nsweeps + residual;
  if (tout) {
    q.var_agg = tout->rho == 0;
    q.align = tout->rho ? tout->rho : 1;
    q.agg_shift = xfer_agg_shift(*tout);
  }
  return launch_has_tile(q);
}

// structured: nsweeps sweeps from u_in (may be nullptr = zero) into u_out (!= u_in)
// chk: the launch -- it has to be a single one -- forms these checkpoints (one more element of halo for their residual rows)
static int btd_smooth(aggmg_ctx* ctx, const BtdDev& b, const double* u_in, const double* rhs, Damping alpha,
                      int nsweeps, double* u_out, int level, int64_t N, int gs = 0, CgtChk* chk = nullptr) {
  const int smax = std::max(1, btd_max_sweeps(b, 0) / (gs ? 2 : 1));
  const double* src = u_in;
  int left = nsweeps;
  if (left == 0) {
    if (u_in)
      HIPCHK(hipMemcpyAsync(u_out, u_in, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    else
      HIPCHK(hipMemsetAsync(u_out, 0, N * sizeof(double), ctx->stream));
    return AGGMG_OK;
  }
  // chunk chain: src -> (scratch0 / scratch1 alternating) -> ... -> u_out
  const int nchunks = (left + smax - 1) / smax;
  if (chk && nchunks > 1) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: checkpoints in a chunked run of sweeps");
  WorkLease t0, t1;
  if (nchunks > 1) {
    CHECK(scratch_lease(ctx, kScratchPing, N, "btd_smooth", &t0));
    if (nchunks > 2) CHECK(scratch_lease(ctx, kScratchPong, N, "btd_smooth", &t1));
  }
  for (int c = 0; c < nchunks; ++c) {
    const int s = std::min(left, smax);
    double* dst = (c == nchunks - 1) ? u_out : (((nchunks - 1 - c) % 2 == 1) ? t0.get() : t1.get());
    FusedLaunch a = fused_sweeps(b, src, rhs, dst, alpha.from(nsweeps - left), s, gs);
    if (chk) fused_chk(a, *chk);
    {
      ProfScope ps(ctx, AGGMG_KIND_SMOOTH, level);
      CHECK(launch_btd(ctx, b, a, s + (chk ? 1 : 0), TileSel(), chk));
    }
    src = dst;
    left -= s;
  }
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// element-patch Schwarz (patch_kernels.hpp)
// ---------------------------------------------------------------------------------------------
static_assert(kPatchMaxSweeps == kSweepWeights, "a patch launch takes as many sweeps as its weights array holds");

// (the forms the patch kernels are instantiated for: patch_form, forms.hpp.  None of them needs scratch: DESIGN.md section 19)

// The arguments of s sweeps from src into dst.  A smoother with an operator dictionary gets its arrays in place of the full
// ones -- the same bits, read by the element's class -- and launches the dictionary kernels (patch_cls).
static PatchArgs patch_args(const PatchDev& P, const double* src, const double* rhs, double* dst, int s) {
  const BtdDev& b = *P.btd;
  PatchArgs a{b.dblk, b.scol, b.qrow, b.sub, b.sup, P.zrows, P.ne, b.c_sub, b.r_sup, src, rhs, dst, s, 0, 0};
  if (const PatchDictDev* d = P.dict.get()) {
    a.dblk = d->dblk;
    a.scol = d->scol;
    a.qrow = d->qrow;
    a.sub = d->sub;
    a.sup = d->sup;
    a.zrows = d->zrows;
  }
  return a;
}
static const uint16_t* patch_cls(const PatchDev& P) { return P.dict ? P.dict->cls.get() : nullptr; }

// What every patch launch does before and around its kernel: the planner's tile (host_plan.hpp) into a, the tiles sel
// chooses of a's elements (fused_tile_subset; default: all), and go(Form<M, CMP>, tiles, lds bytes) for the smoother's
// form among those of Pred (forms.hpp).  go launches `what`'s kernel on its own argument struct, which holds a.
template <auto Pred, class Go>
static int launch_patch_tiles(aggmg_ctx* ctx, const PatchDev& P, PatchArgs& a, const PatchTilePlan& plan, const TileSel& sel,
                              const char* what, Go&& go) {
  if (!P.btd || !Pred(P.m, P.btd->cmp))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, std::string("internal: block size not instantiated for the ") + what + " kernel");
  if (plan.owned <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, std::string("internal: ") + what + " launch without a tile");
  a.owned = plan.owned;
  a.halo = plan.halo;
  const TileSubset sub = fused_tile_subset(a.ne, plan.owned, sel.mode == 3 ? 0 : sel.mode, sel.head, sel.tail);
  if (sub.ntiles == 0) return AGGMG_OK;
  with_form<Pred>(P.m, P.btd->cmp, [&](auto f) {
    static_assert(PatchSlabs<decltype(f)::kM>::NS == patch_slabs(decltype(f)::kM), "the planner sizes the tile the kernel is instantiated for");
    go(f, sub, plan.lds_bytes);
  });
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int launch_patch(aggmg_ctx* ctx, const PatchDev& P, PatchArgs a, const SweepWeights& wts) {
  const uint16_t* cls = patch_cls(P);
  return launch_patch_tiles<patch_form>(ctx, P, a, patch_tile_plan(P.m, a.nsweeps), TileSel(), "patch sweep", [&](auto f, const TileSubset& t, size_t lds) {
    using F = decltype(f);
    constexpr int NS = PatchSlabs<F::kM>::NS;
    const dim3 grid((unsigned)t.ntiles), block(kThreads);
    if (cls) {
      if (P.hybrid)
        hipLaunchKernelGGL((patch_sweep_dict_kernel<F::kM, F::kCmp, NS, true>), grid, block, lds, ctx->stream, a, wts, cls);
      else
        hipLaunchKernelGGL((patch_sweep_dict_kernel<F::kM, F::kCmp, NS, false>), grid, block, lds, ctx->stream, a, wts, cls);
    } else if (P.hybrid)
      hipLaunchKernelGGL((patch_sweep_kernel<F::kM, F::kCmp, NS, true>), grid, block, lds, ctx->stream, a, wts);
    else
      hipLaunchKernelGGL((patch_sweep_kernel<F::kM, F::kCmp, NS, false>), grid, block, lds, ctx->stream, a, wts);
  });
}

// the multiplicative two-colour sweeps (aggmg_patch_gs_setup): patch_gs_kernel in the tile of patch_gs_tile_plan
static int launch_patch_gs(aggmg_ctx* ctx, const PatchDev& P, const PatchArgs& a, const SweepWeights& wts, bool reverse) {
  const uint16_t* cls = patch_cls(P);
  PatchGsArgs g{a, reverse ? 1 : 0};
  return launch_patch_tiles<patch_form>(ctx, P, g.p, patch_gs_tile_plan(P.m, a.nsweeps), TileSel(), "multiplicative patch sweep",
                                        [&](auto f, const TileSubset& t, size_t lds) {
    using F = decltype(f);
    constexpr int NS = PatchSlabs<F::kM>::NS;
    const dim3 grid((unsigned)t.ntiles), block(kThreads);
    if (cls)
      hipLaunchKernelGGL((patch_gs_dict_kernel<F::kM, F::kCmp, NS>), grid, block, lds, ctx->stream, g, wts, cls);
    else
      hipLaunchKernelGGL((patch_gs_kernel<F::kM, F::kCmp, NS>), grid, block, lds, ctx->stream, g, wts);
  });
}

// the one-launch ascent of a multiplicative patch level (patch_gs_up_kernel): prolongation and nsweeps <= patch_gs_max_sweeps
// reverse sweeps on the tiles sel chooses, the same tile plan
static int launch_patch_gs_up(aggmg_ctx* ctx, const PatchDev& P, PatchGsUpArgs u, const SweepWeights& wts, const TileSel& sel) {
  const uint16_t* cls = patch_cls(P);
  return launch_patch_tiles<patch_form>(ctx, P, u.g.p, patch_gs_tile_plan(P.m, u.g.p.nsweeps), sel, "multiplicative patch ascent",
                                        [&](auto f, const TileSubset& t, size_t lds) {
    using F = decltype(f);
    constexpr int NS = PatchSlabs<F::kM>::NS;
    const dim3 grid((unsigned)t.ntiles), block(kThreads);
    u.tile_split = t.split;
    u.tile_skip = t.skip;
    if (cls)
      hipLaunchKernelGGL((patch_gs_up_dict_kernel<F::kM, F::kCmp, NS>), grid, block, lds, ctx->stream, u, wts, cls);
    else
      hipLaunchKernelGGL((patch_gs_up_kernel<F::kM, F::kCmp, NS>), grid, block, lds, ctx->stream, u, wts);
  });
}

// nsweeps sweeps from u_in (may be nullptr = zero) into u_out (!= u_in), in launches of up to patch_max_sweeps
// (multiplicative: patch_gs_max_sweeps; reverse: its colours in the order 1, 0 -- post-smoothing; the others ignore it)
static int patch_smooth(aggmg_ctx* ctx, const PatchDev& P, const double* u_in, const double* rhs, Damping alpha, int nsweeps,
                        double* u_out, int level, bool reverse = false) {
  const int64_t N = P.ne * P.m;
  if (nsweeps == 0) {
    if (u_in && u_in != u_out)
      HIPCHK(hipMemcpyAsync(u_out, u_in, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    else if (!u_in)
      HIPCHK(hipMemsetAsync(u_out, 0, N * sizeof(double), ctx->stream));
    return AGGMG_OK;
  }
  const int smax = P.multiplicative ? patch_gs_max_sweeps(P.m) : patch_max_sweeps(P.m);
  const int nchunks = patch_chunks(nsweeps, smax);
  if (nchunks == 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: patch sweeps without a tile");
  // chunk chain: src -> (scratch0 / scratch1 alternating) -> ... -> u_out
  WorkLease t0, t1;
  if (nchunks > 1) {
    CHECK(scratch_lease(ctx, kScratchPing, N, "patch_smooth", &t0));
    if (nchunks > 2) CHECK(scratch_lease(ctx, kScratchPong, N, "patch_smooth", &t1));
  }
  const double* src = u_in;
  for (int c = 0; c < nchunks; ++c) {
    const int s = patch_chunk_sweeps(nsweeps, smax, c);
    double* dst = (c == nchunks - 1) ? u_out : (((nchunks - 1 - c) % 2 == 1) ? t0.get() : t1.get());
    const PatchArgs a = patch_args(P, src, rhs, dst, s);
    {
      ProfScope ps(ctx, AGGMG_KIND_SMOOTH, level);
      if (P.multiplicative)
        CHECK(launch_patch_gs(ctx, P, a, alpha.from(c * smax).launch(s), reverse));
      else
        CHECK(launch_patch(ctx, P, a, alpha.from(c * smax).launch(s)));
    }
    src = dst;
  }
  return AGGMG_OK;
}

// ---- the patch sweeps on K columns (patch_multi_kernels.hpp, patch_schwarz_multi_kernels.hpp; DESIGN.md sections 22, 25) ----
// the levels patch_gs_multi_kernel serves: multiplicative sweeps on a K-column form (multi_form, forms.hpp); the hybrid /
// additive ones of patch_sweep_multi_kernel: patch_schwarz_multi_form_ok
static bool patch_multi_form_ok(const PatchDev& P) { return P.multiplicative && P.btd && multi_form(P.m, P.btd->cmp); }
static bool patch_schwarz_multi_form_ok(const PatchDev& P) { return !P.multiplicative && P.btd && multi_form(P.m, P.btd->cmp); }

static int launch_patch_gs_multi(aggmg_ctx* ctx, const PatchDev& P, PatchGsMultiArgs m, const SweepWeights& wts) {
  if (!P.multiplicative) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column patch sweep launch on an additive smoother");
  const uint16_t* cls = patch_cls(P);
  const int kb = col_group(m.kc);
  const PatchTilePlan plan = (m.kc >= 1 && m.kc <= kb) ? patch_gs_multi_tile_plan(P.m, m.g.p.nsweeps, kb) : PatchTilePlan();
  return launch_patch_tiles<multi_form>(ctx, P, m.g.p, plan, TileSel(), "K-column multiplicative patch sweep",
                                        [&](auto f, const TileSubset& t, size_t lds) {
    using F = decltype(f);
    with_col_group(m.kc, [&](auto g) {
      constexpr int KB = decltype(g)::value;
      if (cls)
        hipLaunchKernelGGL((patch_gs_multi_kernel<F::kM, F::kCmp, KB, true>), dim3((unsigned)t.ntiles), dim3(kThreads), lds, ctx->stream, m, wts, cls);
      else
        hipLaunchKernelGGL((patch_gs_multi_kernel<F::kM, F::kCmp, KB, false>), dim3((unsigned)t.ntiles), dim3(kThreads), lds, ctx->stream, m, wts, cls);
    });
    ++ctx->patch_multi_launches;
  });
}

// the hybrid / additive sweeps (patch_sweep_multi_kernel) in the tile of patch_schwarz_multi_tile_plan
static int launch_patch_schwarz_multi(aggmg_ctx* ctx, const PatchDev& P, PatchSchwarzMultiArgs m, const SweepWeights& wts) {
  if (P.multiplicative) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column hybrid patch sweep launch on a multiplicative smoother");
  const uint16_t* cls = patch_cls(P);
  const int kb = col_group(m.kc);
  const PatchTilePlan plan = (m.kc >= 1 && m.kc <= kb) ? patch_schwarz_multi_tile_plan(P.m, m.p.nsweeps, kb) : PatchTilePlan();
  return launch_patch_tiles<multi_form>(ctx, P, m.p, plan, TileSel(), "K-column hybrid patch sweep",
                                        [&](auto f, const TileSubset& t, size_t lds) {
    using F = decltype(f);
    const dim3 grid((unsigned)t.ntiles), block(kThreads);
    with_col_group(m.kc, [&](auto g) {
      constexpr int KB = decltype(g)::value;
      if (cls) {
        if (P.hybrid)
          hipLaunchKernelGGL((patch_sweep_multi_kernel<F::kM, F::kCmp, KB, true, true>), grid, block, lds, ctx->stream, m, wts, cls);
        else
          hipLaunchKernelGGL((patch_sweep_multi_kernel<F::kM, F::kCmp, KB, false, true>), grid, block, lds, ctx->stream, m, wts, cls);
      } else if (P.hybrid)
        hipLaunchKernelGGL((patch_sweep_multi_kernel<F::kM, F::kCmp, KB, true, false>), grid, block, lds, ctx->stream, m, wts, cls);
      else
        hipLaunchKernelGGL((patch_sweep_multi_kernel<F::kM, F::kCmp, KB, false, false>), grid, block, lds, ctx->stream, m, wts, cls);
    });
    ++ctx->patch_schwarz_multi_launches;
  });
}

// the most sweeps one K-column launch of the smoother's kind takes (0: no tile)
static int patch_multi_max_sweeps(const PatchDev& P) {
  return P.multiplicative ? patch_gs_multi_max_sweeps(P.m) : patch_schwarz_multi_max_sweeps(P.m);
}

// a zeroed argument block of a K-column sweep kernel with the tail the two kinds share: the column strides, the columns
template <class Args>
static Args patch_multi_args(ColsIn src, ColsIn B, ColsOut dst, int kc) {
  Args m;
  std::memset(&m, 0, sizeof(m));
  m.ld_uin = src.ld;
  m.ld_b = B.ld;
  m.ld_uout = dst.ld;
  m.kc = kc;
  return m;
}
// nsweeps >= 1 sweeps on kc <= 8 columns from U0 (null: zero) into U, in launches of up to patch_multi_max_sweeps, each
// with its slice of the weights, as patch_smooth chunks a single column's run: patch_gs_multi_kernel for a multiplicative
// smoother, patch_sweep_multi_kernel for a hybrid / additive one (which ignores `reverse`, as its single-column sweeps do).
// A chunked run alternates between U and `other` (kc columns, neither U0 nor U; null: leased from the context's scratch)
// so that the last launch writes U.
static int patch_smooth_multi(aggmg_ctx* ctx, const PatchDev& P, ColsIn U0, ColsIn B, Damping alpha, int nsweeps, bool reverse,
                              ColsOut U, ColsOut other, int kc, int level) {
  const int64_t N = P.ne * P.m;
  // (hybrid / additive: no launch of more columns than ctx->patch_schwarz_multi_cols -- each slice of the group its own run)
  if (!P.multiplicative && kc > ctx->patch_schwarz_multi_cols) {
    for (int c0 = 0; c0 < kc; c0 += ctx->patch_schwarz_multi_cols)
      CHECK(patch_smooth_multi(ctx, P, U0.at(c0), B.at(c0), alpha, nsweeps, reverse, U.at(c0), other.at(c0),
                               std::min(ctx->patch_schwarz_multi_cols, kc - c0), level));
    return AGGMG_OK;
  }
  const int smax = patch_multi_max_sweeps(P);
  const int nchunks = patch_chunks(nsweeps, smax);
  if (nchunks == 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column patch sweeps without a tile");
  WorkLease t0;
  if (nchunks > 1 && !other.p) {
    CHECK(scratch_lease(ctx, kScratchPing, N * kc, "patch_smooth_multi", &t0));
    other = ColsOut(t0.get(), N);
  }
  ColsIn src = U0;
  for (int c = 0; c < nchunks; ++c) {
    const int s = patch_chunk_sweeps(nsweeps, smax, c);
    const ColsOut dst = ((nchunks - 1 - c) % 2 == 0) ? U : other;
    const SweepWeights wts = alpha.from(c * smax).launch(s);
    ProfScope ps(ctx, AGGMG_KIND_SMOOTH, level);
    if (P.multiplicative) {
      PatchGsMultiArgs m = patch_multi_args<PatchGsMultiArgs>(src, B, dst, kc);
      m.g.p = patch_args(P, src.p, B.p, dst.p, s);
      m.g.reverse = reverse ? 1 : 0;
      CHECK(launch_patch_gs_multi(ctx, P, m, wts));
    } else {
      PatchSchwarzMultiArgs m = patch_multi_args<PatchSchwarzMultiArgs>(src, B, dst, kc);
      m.p = patch_args(P, src.p, B.p, dst.p, s);
      CHECK(launch_patch_schwarz_multi(ctx, P, m, wts));
    }
    src = dst;
  }
  return AGGMG_OK;
}

// index lists of the patches {e, .., e + width - 1}, e = 0 .. ne - width (a level of fewer elements: one patch of all)
static void patch_lists(int64_t m, int64_t ne, int width, std::vector<int64_t>* lists, int64_t* bm, int64_t* nb) {
  const int64_t w = std::min<int64_t>(width, ne);
  *bm = w * m;
  *nb = ne - w + 1;
  lists->resize((size_t)(*nb * *bm));
  for (int64_t p = 0; p < *nb; ++p)
    for (int64_t j = 0; j < *bm; ++j) (*lists)[p * *bm + j] = p * m + j;
}

// The fused form of a patch smoother on the element blocks eb of A: the patch blocks assembled from them, inverted, and
// their rows laid out per DoF row (zrows); then the smoother's operator dictionary where the option is on.  The hybrid /
// additive sweeps (patch_sweep_kernel) and the multiplicative ones (patch_gs_kernel) read the same arrays.
static int patch_fused_setup(aggmg_ctx* ctx, aggmg_op* A, int64_t m, int64_t ne, const std::shared_ptr<BtdDev>& eb, bool hybrid,
                             bool multiplicative, const char* who, aggmg_smoother** out) {
  auto sm = std::make_unique<aggmg_smoother>();
  sm->kind = hybrid ? 2 : 1;   // (multiplicative: 1 -- aggmg_smoother_patch_info's hybrid stays 0)
  sm->A = A;
  sm->N = A->m;
  sm->m = 2 * m;
  sm->nb = ne - 1;
  sm->overlapping = true;
  sm->patch_width = 2;
  auto P = std::make_shared<PatchDev>();
  P->m = (int)m;
  P->ne = ne;
  P->hybrid = hybrid;
  P->multiplicative = multiplicative;
  P->btd = eb;
  {
    const int64_t words = (ne - 1) * 4 * m * m;
    DevArray<double> blocks, zinv;
    CHECK(blocks.alloc(ctx, words));
    CHECK(zinv.alloc(ctx, words));
    hipLaunchKernelGGL(patch_assemble_kernel, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream,
                       words, (int)m, eb->cmp ? 1 : 0, eb->c_sub, eb->r_sup, (const double*)eb->dblk, (const double*)eb->scol,
                       (const double*)eb->qrow, (const double*)eb->sub, (const double*)eb->sup, blocks.get());
    HIPCHK(hipGetLastError());
    int64_t sing = -1;
    CHECK(setup_invert_blocks(ctx, ne - 1, (int)(2 * m), blocks, 0, zinv, &sing));
    if (sing >= 0)
      return fail(ctx, AGGMG_ERR_SINGULAR,
                  std::string(who) + ": singular patch " + std::to_string(sing + 1) + " (SingularException)");
    const int64_t zw = A->m * 4 * m;
    CHECK(P->zrows.alloc(ctx, zw));
    hipLaunchKernelGGL(patch_zrows_kernel, dim3((unsigned)((zw + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, zw,
                       (int)m, ne, (const double*)zinv, P->zrows.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the temporaries go out of scope
  }
  // the smoother's distinct operator records, where they are few (AGGMG_OPT_OPERATOR_DICTIONARY)
  if (ctx->op_dict) CHECK(setup_patch_dictionary(ctx, *P));
  sm->patch = P;
  *out = sm.release();
  return AGGMG_OK;
}

extern "C" int aggmg_patch_schwarz_setup(aggmg_ctx* ctx, aggmg_op* A, int64_t m, int64_t ne, int width, int hybrid,
                                         aggmg_smoother** out) {
  if (!ctx || !A || !out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_schwarz_setup: NULL argument");
  *out = nullptr;
  if (A->m != A->n) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_patch_schwarz_setup: operator is not square");
  if (width < 2 || width > 4) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_schwarz_setup: width must be 2, 3 or 4");
  if (m < 1 || ne < 1 || m * width > 64)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_schwarz_setup: rows per element must be in 1 .. 64 / width, elements >= 1");
  if (A->m != m * ne) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_patch_schwarz_setup: operator size is not m * ne");
  if (A->m * width >= ((int64_t)1 << 31)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_schwarz_setup: width * m * ne >= 2^31");
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<int64_t> lists;
  int64_t bm = 0, nb = 0;
  // the fused form: patches of two elements on an operator that is block tridiagonal in the element blocking, in a block
  // size the kernel is instantiated for.  The element blocks come from the block-Jacobi set-up of the element lists
  // (scatter, pattern detection, A->btd); that smoother itself is not kept.
  std::shared_ptr<BtdDev> eb;
  if (width == 2 && ne >= 2 && m <= 9) {
    patch_lists(m, ne, 1, &lists, &bm, &nb);
    aggmg_smoother* elem = nullptr;
    const int st = aggmg_blockjacobi_setup(ctx, A, m, ne, lists.data(), 0, 0, &elem);
    if (st != AGGMG_OK && st != AGGMG_ERR_SINGULAR) return st;   // (a singular element block: the patches may still be regular)
    if (elem && elem->btd && patch_form((int)m, elem->btd->cmp) && patch_max_sweeps((int)m) >= 1) eb = elem->btd;
    if (elem) CHECK(aggmg_smoother_free(ctx, elem));
  }
  if (!eb) {   // the generic route on the lists, as everywhere: the same results to round-off
    patch_lists(m, ne, width, &lists, &bm, &nb);
    CHECK(aggmg_blockjacobi_setup(ctx, A, bm, nb, lists.data(), 0, hybrid ? 1 : 0, out));
    (*out)->patch_width = width;
    return AGGMG_OK;
  }
  return patch_fused_setup(ctx, A, m, ne, eb, hybrid != 0, false, "aggmg_patch_schwarz_setup", out);
}

extern "C" int aggmg_patch_gs_setup(aggmg_ctx* ctx, aggmg_op* A, int64_t m, int64_t ne, aggmg_smoother** out) {
  if (!ctx || !A || !out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_gs_setup: NULL argument");
  *out = nullptr;
  if (A->m != A->n) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_patch_gs_setup: operator is not square");
  if (m < 1 || ne < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_gs_setup: rows per element and elements must be >= 1");
  if (A->m != m * ne) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_patch_gs_setup: operator size is not m * ne");
  if (A->m * 2 >= ((int64_t)1 << 31)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_gs_setup: 2 * m * ne >= 2^31");
  // the fused form or none: the sweeps exist as patch_gs_kernel only
  if (ne < 2)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_patch_gs_setup: a level of one element has no patch of two elements");
  if (m > 9 || patch_gs_max_sweeps((int)m) < 1)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                "aggmg_patch_gs_setup: the sweep kernel is not instantiated for " + std::to_string(m) + " rows per element");
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<int64_t> lists;
  int64_t bm = 0, nb = 0;
  patch_lists(m, ne, 1, &lists, &bm, &nb);
  aggmg_smoother* elem = nullptr;
  const int st = aggmg_blockjacobi_setup(ctx, A, m, ne, lists.data(), 0, 0, &elem);
  if (st != AGGMG_OK && !elem) return st;   // (the element blocks come from that set-up: without them, its error stands)
  std::shared_ptr<BtdDev> eb = elem ? elem->btd : nullptr;
  if (elem) CHECK(aggmg_smoother_free(ctx, elem));
  if (!eb)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_patch_gs_setup: the operator is not block tridiagonal in the element blocking");
  if (!patch_form((int)m, eb->cmp))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                "aggmg_patch_gs_setup: the sweep kernel is not instantiated for " + std::to_string(m) + " rows per element with " +
                    (eb->cmp ? "compressed" : "dense") + " couplings");
  return patch_fused_setup(ctx, A, m, ne, eb, false, true, "aggmg_patch_gs_setup", out);
}

extern "C" int aggmg_smoother_patch_kind(aggmg_ctx* ctx, const aggmg_smoother* sm, int* kind) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!sm || !kind) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_patch_kind: NULL argument");
  if (!sm->patch_width)
    *kind = 0;
  else if (sm->patch && sm->patch->multiplicative)
    *kind = 3;
  else
    *kind = sm->kind == 2 ? 2 : 1;
  return AGGMG_OK;
}

extern "C" int aggmg_smoother_patch_info(aggmg_ctx* ctx, const aggmg_smoother* sm, int* width, int* hybrid, int* fused) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!sm || !width || !hybrid || !fused) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_patch_info: NULL argument");
  *width = sm->patch_width;   // 0: not an element-patch Schwarz smoother
  *hybrid = sm->patch_width && sm->kind == 2 ? 1 : 0;
  *fused = sm->patch ? 1 : 0;
  return AGGMG_OK;
}

extern "C" int aggmg_smoother_patch_dictionary(aggmg_ctx* ctx, const aggmg_smoother* sm, int* nclasses) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!sm || !nclasses) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_patch_dictionary: NULL argument");
  *nclasses = (sm->patch && sm->patch->dict) ? sm->patch->dict->nclasses : 0;
  return AGGMG_OK;
}

extern "C" int aggmg_patch_gs_tile_plan(int m, int nsweeps, int* tile_elems, int* owned, int* halo, int* max_sweeps) {
  if (!tile_elems || !owned || !halo || !max_sweeps) return AGGMG_ERR_ARGUMENT;
  const PatchTilePlan p = patch_gs_tile_plan(m, nsweeps);   // host_plan.hpp: what launch_patch_gs_t runs
  *tile_elems = p.te;
  *owned = p.owned;
  *halo = p.halo;
  *max_sweeps = patch_gs_max_sweeps(m);
  return AGGMG_OK;
}

extern "C" int aggmg_patch_gs_multi_tile_plan(int m, int nsweeps, int kb, int* tile_elems, int* owned, int* halo, int* max_sweeps) {
  if (!tile_elems || !owned || !halo || !max_sweeps) return AGGMG_ERR_ARGUMENT;
  const PatchTilePlan p = patch_gs_multi_tile_plan(m, nsweeps, kb);   // host_plan.hpp: what launch_patch_gs_multi_t runs
  *tile_elems = p.te;
  *owned = p.owned;
  *halo = p.halo;
  *max_sweeps = patch_gs_multi_max_sweeps(m);
  return AGGMG_OK;
}

extern "C" int aggmg_patch_schwarz_multi_tile_plan(int m, int nsweeps, int kb, int* tile_elems, int* owned, int* halo, int* max_sweeps) {
  if (!tile_elems || !owned || !halo || !max_sweeps) return AGGMG_ERR_ARGUMENT;
  const PatchTilePlan p = patch_schwarz_multi_tile_plan(m, nsweeps, kb);   // host_plan.hpp: what launch_patch_schwarz_multi runs
  *tile_elems = p.te;
  *owned = p.owned;
  *halo = p.halo;
  *max_sweeps = patch_schwarz_multi_max_sweeps(m);
  return AGGMG_OK;
}

extern "C" int aggmg_chain_multi_tile_plan(int m, int nsweeps, int restrict_kind, int rho, int kb, int* tile_blocks, int* owned,
                                           int* halo_left, int* halo_right, int* max_sweeps) {
  if (!tile_blocks || !owned || !halo_left || !halo_right || !max_sweeps) return AGGMG_ERR_ARGUMENT;
  const ChainMultiPlan p = chain_multi_tile_plan(m, nsweeps, restrict_kind, rho, kb);   // host_plan.hpp: what cgt_multi_launch_t runs
  *tile_blocks = p.te;
  *owned = p.owned;
  *halo_left = p.halo_left;
  *halo_right = p.halo_right;
  *max_sweeps = chain_multi_max_sweeps(m);
  return AGGMG_OK;
}

extern "C" int aggmg_chain_multi_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_chain_multi_launches: NULL argument");
  *count = ctx->chain_multi_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_patch_multi_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_multi_launches: NULL argument");
  *count = ctx->patch_multi_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_patch_schwarz_multi_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_patch_schwarz_multi_launches: NULL argument");
  *count = ctx->patch_schwarz_multi_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_patch_tile_plan(int m, int nsweeps, int* tile_elems, int* owned, int* max_sweeps) {
  if (!tile_elems || !owned || !max_sweeps) return AGGMG_ERR_ARGUMENT;
  const PatchTilePlan p = patch_tile_plan(m, nsweeps);   // host_plan.hpp: what launch_patch_t runs
  *tile_elems = p.te;
  *owned = p.owned;
  *max_sweeps = patch_max_sweeps(m);
  return AGGMG_OK;
}

// generic: one sweep u_out = u_in + alpha * S^{-1}(b - A u_in); u_out may alias u_in for block
// smoothers, must differ for point Jacobi.
static int generic_sweep(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* u_in, const double* rhs,
                         double alpha, double* u_out, int level) {
  const int64_t N = A->m;
  if (sm->patch) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: generic sweep of a fused element-patch Schwarz smoother");
  if (sm->kind == 0) {
    ProfScope ps(ctx, AGGMG_KIND_JACOBI, level);
    CHECK(op_ensure_csr(ctx, A));
    return launch_csr<kJacobi>(ctx, A->csr, u_in, rhs, sm->diag, alpha, u_out);
  }
  CHECK(op_ensure_csr(ctx, A));
  // (AGGMG_BLOCK_SWEEP=0: the earlier form -- CSR residual, zeroed vector, batched block apply with atomic adds where the
  // lists overlap, update: four launches -- for A/B runs)
  static const bool onepass = env_int("AGGMG_BLOCK_SWEEP", 1) != 0;
  if (onepass && A->csr.maxrow >= 0 && A->csr.maxrow <= 4 * kRowThreadMax && sm->m <= kThreads) {
    // residual rows and block solves in ONE pass (block_sweep_kernel): the residual never reaches HBM
    const int bpw = kThreads / (int)sm->m;
    const unsigned nwg = (unsigned)((sm->nb + bpw - 1) / bpw);
    const bool partition = !sm->overlapping && sm->nb * sm->m == N && sm->kind == 1;   // every row in exactly one block
    ProfScope ps(ctx, AGGMG_KIND_BLOCK_APPLY, level);
    if (partition && u_out != u_in) {
      CHECK(setup_block_order(ctx, sm));
      if (nwg)
        hipLaunchKernelGGL((block_sweep_kernel<true>), dim3(nwg), dim3(kThreads), 0, ctx->stream, A->csr.view(), sm->binv, sm->inds,
                           (int)sm->m, sm->nb, u_in, rhs, alpha, u_out);
      HIPCHK(hipGetLastError());
      return AGGMG_OK;
    }
    CHECK(setup_block_cover(ctx, sm));
    WorkLease Y;
    CHECK(scratch_lease(ctx, kScratchPong, std::max<int64_t>(N, sm->nb * sm->m), "generic_sweep", &Y));
    if (nwg)
      hipLaunchKernelGGL((block_sweep_kernel<false>), dim3(nwg), dim3(kThreads), 0, ctx->stream, A->csr.view(), sm->binv, sm->inds,
                         (int)sm->m, sm->nb, u_in, rhs, alpha, Y.get());
    HIPCHK(hipGetLastError());
    const unsigned nb2 = (unsigned)((N + kThreads - 1) / kThreads);
    if (nb2)
      hipLaunchKernelGGL(block_combine_kernel, dim3(nb2), dim3(kThreads), 0, ctx->stream, N, (const int32_t*)sm->cover_ptr,
                         (const uint32_t*)sm->cover_idx, (const double*)Y, u_in, sm->kind == 2 ? sm->counts : nullptr, alpha, u_out);
    HIPCHK(hipGetLastError());
    return AGGMG_OK;
  }
  WorkLease lr, ly;
  CHECK(scratch_lease(ctx, kScratchPong, N, "generic_sweep", &lr));
  CHECK(scratch_lease(ctx, kScratchStage, N, "generic_sweep", &ly));
  double *r = lr, *y = ly;
  {
    ProfScope ps(ctx, AGGMG_KIND_RESIDUAL, level);
    CHECK(launch_csr<kResidual>(ctx, A->csr, u_in, rhs, nullptr, 0.0, r));
  }
  ProfScope ps(ctx, AGGMG_KIND_BLOCK_APPLY, level);
  HIPCHK(hipMemsetAsync(y, 0, N * sizeof(double), ctx->stream));
  const int64_t nthreads = sm->nb * sm->m;
  const unsigned nblk = (unsigned)((nthreads + kThreads - 1) / kThreads);
  if (nblk) {
    if (sm->overlapping)
      hipLaunchKernelGGL((block_apply_kernel<true>), dim3(nblk), dim3(kThreads), 0, ctx->stream, sm->binv,
                         sm->inds, (int)sm->m, sm->nb, r, y);
    else
      hipLaunchKernelGGL((block_apply_kernel<false>), dim3(nblk), dim3(kThreads), 0, ctx->stream, sm->binv,
                         sm->inds, (int)sm->m, sm->nb, r, y);
    HIPCHK(hipGetLastError());
  }
  const unsigned nb2 = (unsigned)((N + kThreads - 1) / kThreads);
  if (nb2) {
    hipLaunchKernelGGL(axpy_scaled_kernel, dim3(nb2), dim3(kThreads), 0, ctx->stream, N, u_in, y,
                       sm->kind == 2 ? sm->counts : nullptr, alpha, u_out);
    HIPCHK(hipGetLastError());
  }
  return AGGMG_OK;
}

// nsweeps generic point-Jacobi sweeps from src into dst (dst may be src); `other` is a second vector of the level
static int generic_jacobi(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* src, const double* rhs, Damping alpha,
                          int nsweeps, double* dst, double* other, double* rout = nullptr, bool* fused = nullptr) {
  const int64_t N = A->m;
  if (fused) *fused = false;
  if (nsweeps <= 0) {
    if (src != dst) HIPCHK(hipMemcpyAsync(dst, src, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return AGGMG_OK;
  }
  const bool want_r = rout && fused && A->csr.bandblk && A->csr.band_sweeps >= 2;
  const int per = A->csr.bandblk ? (want_r ? A->csr.band_sweeps - 1 : A->csr.band_sweeps) : 1;
  const int nl = (nsweeps + per - 1) / per;
  // the launches alternate between dst and other and end in dst: the first one writes `other` when their number is
  // even -- a source that is the first target has to move out of the way
  double* first = ((nl - 1) % 2 == 0) ? dst : other;
  if (first == src) {
    double* spare = first == dst ? other : dst;
    if (nl == 1) {   // one launch, in place: through the spare vector
      CHECK(launch_csr_jacobi_sweeps(ctx, A->csr, src, rhs, sm->diag, alpha, nsweeps, spare, dst, rout, fused));
      HIPCHK(hipMemcpyAsync(dst, spare, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      return AGGMG_OK;
    }
    HIPCHK(hipMemcpyAsync(spare, src, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    src = spare;
  }
  return launch_csr_jacobi_sweeps(ctx, A->csr, src, rhs, sm->diag, alpha, nsweeps, dst, other, rout, fused);
}

// n sweeps of a generic smoother from src (nullptr = zero) into dst.  Sweep s writes `work`, the last one dst: with
// work == dst (aggmg_smooth_dev, the descent) every sweep but the first runs in place in dst; with work == src (the
// ascent) every sweep but the last in src.  Part of the contract: generic_sweep takes the one-pass block sweep only where
// input and output differ.  Point Jacobi: generic_jacobi between dst and `other` (rout / resid_done: the banded form's residual).
static int generic_sweeps(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* src, const double* rhs, Damping damp,
                          int n, double* dst, double* work, double* other, int level, double* rout = nullptr,
                          bool* resid_done = nullptr) {
  const int64_t N = A->m;
  if (resid_done) *resid_done = false;
  if (!src) {
    HIPCHK(hipMemsetAsync(dst, 0, N * sizeof(double), ctx->stream));
    src = dst;
  }
  if (n == 0) {
    if (src != dst) HIPCHK(hipMemcpyAsync(dst, src, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return AGGMG_OK;
  }
  if (sm->kind == 0) {   // point Jacobi: several sweeps per launch where the operator is banded
    CHECK(op_ensure_csr(ctx, A));
    ProfScope ps(ctx, AGGMG_KIND_JACOBI, level);
    return generic_jacobi(ctx, A, sm, src, rhs, damp, n, dst, other, rout, resid_done);
  }
  for (int s = 0; s < n; ++s) {
    double* d = (s == n - 1) ? dst : work;
    CHECK(generic_sweep(ctx, A, sm, src, rhs, damp.at(s), d, level));
    src = d;
  }
  return AGGMG_OK;
}

static int check_pair(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const char* who) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!A || !sm) return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": NULL handle");
  if (A->m != A->n || sm->N != A->m)
    return fail(ctx, AGGMG_ERR_DIMENSION, std::string(who) + ": operator / smoother size mismatch");
  return AGGMG_OK;
}

static int smooth_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* u_in, const double* b, Damping alpha,
                      int nsweeps, double* u_out) {
  CHECK(check_pair(ctx, A, sm, "aggmg_smooth"));
  if (!b || !u_out || nsweeps < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smooth: bad argument");
  const int64_t N = A->m;
  if (N == 0) return AGGMG_OK;
  const bool chain = sm->cgt && sm->A == A;   // CG chain form: fused point-Jacobi sweeps
  const bool patch = sm->patch && sm->A == A;   // fused element-patch Schwarz sweeps
  if (sm->patch && !patch) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smooth: the smoother was set up on another operator");
  if (chain || patch || (sm->btd && sm->A == A)) {
    // (the fused forms want u_out != u_in: an in-place request is staged through scratch, an extra copy)
    WorkLease stage;
    if (u_out == u_in) CHECK(scratch_lease(ctx, kScratchStage, N, "aggmg_smooth", &stage));
    double* dst = stage.held() ? stage.get() : u_out;
    if (chain)
      CHECK(cgt_smooth_ext(ctx, *sm->cgt, u_in, b, alpha, nsweeps, dst, 0));
    else if (patch)
      CHECK(patch_smooth(ctx, *sm->patch, u_in, b, alpha, nsweeps, dst, 0));
    else
      CHECK(btd_smooth(ctx, *sm->btd, u_in, b, alpha, nsweeps, dst, 0, N, sm->gs ? 1 : 0));
    if (dst != u_out) HIPCHK(hipMemcpyAsync(u_out, dst, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return AGGMG_OK;
  }
  WorkLease t;   // point Jacobi ping-pongs through it
  CHECK(scratch_lease(ctx, kScratchPing, N, "aggmg_smooth", &t));
  return generic_sweeps(ctx, A, sm, u_in, b, alpha, nsweeps, u_out, u_out, t, 0);
}

extern "C" int aggmg_smooth_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* u_in,
                                const double* b, double alpha, int nsweeps, double* u_out) {
  return smooth_dev(ctx, A, sm, u_in, b, Damping(alpha), nsweeps, u_out);
}

// EXTENSION (no reference counterpart): sweep s damped by w[s] -- the launches of aggmg_smooth_dev, each with its slice of w
extern "C" int aggmg_smooth_weighted_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* u_in,
                                         const double* b, const double* w, int nsweeps, double* u_out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (nsweeps < 0 || (nsweeps > 0 && !w)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smooth_weighted: bad argument");
  for (int s = 0; s < nsweeps; ++s)
    if (!std::isfinite(w[s])) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smooth_weighted: weight is not finite");
  // (w is read while the launches are enqueued, not after; a run of zero sweeps has no array to point at)
  return smooth_dev(ctx, A, sm, u_in, b, Damping(0.0, nsweeps ? w : nullptr), nsweeps, u_out);
}

extern "C" int aggmg_residual_dev(aggmg_ctx* ctx, aggmg_op* A, const double* u, const double* b, double* r_out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!A || !u || !b || !r_out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual: NULL argument");
  ProfScope ps(ctx, AGGMG_KIND_RESIDUAL, 0);
  if (A->cgt && r_out != u && r_out != b) return cgt_residual_ext(ctx, *A->cgt, u, b, r_out);
  if (A->btd && r_out != u && r_out != b) {  // index-free block-tridiagonal form, one fused pass
    FusedLaunch a = fused_sweeps(*A->btd, u, b, nullptr, 0.0, 0);
    a.do_residual = 1;
    a.r_out = r_out;
    return launch_btd(ctx, *A->btd, a, 1);
  }
  CHECK(op_ensure_csr(ctx, A));
  return launch_csr<kResidual>(ctx, A->csr, u, b, nullptr, 0.0, r_out);
}

extern "C" int aggmg_restrict_dev(aggmg_ctx* ctx, aggmg_op* L, const double* r, double* rc_out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!L || !r || !rc_out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_restrict: NULL argument");
  if (L->kind != AGGMG_OP_TRANSFER) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_restrict: operator was not uploaded as a transfer");
  CHECK(op_ensure_csc_blocks(ctx, L));
  ProfScope ps(ctx, AGGMG_KIND_RESTRICT, 0);
  return launch_csr<kSpmvSet>(ctx, L->csc, r, nullptr, nullptr, 0.0, rc_out);
}

extern "C" int aggmg_prolong_add_dev(aggmg_ctx* ctx, aggmg_op* L, const double* uc, double* u_inout) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!L || !uc || !u_inout) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_prolong_add: NULL argument");
  CHECK(op_ensure_csr(ctx, L));
  ProfScope ps(ctx, AGGMG_KIND_PROLONG, 0);
  return launch_csr<kSpmvAdd>(ctx, L->csr, uc, nullptr, nullptr, 0.0, u_inout);
}

// ---------------------------------------------------------------------------------------------
// host-pointer wrappers
// ---------------------------------------------------------------------------------------------
struct DevVec {
  aggmg_ctx* ctx;
  DevArray<double> p;
  explicit DevVec(aggmg_ctx* c) : ctx(c) {}
  ~DevVec() {
    if (p) (void)hipStreamSynchronize(ctx->stream);   // a launch may still read it
  }
  int alloc(int64_t n, const double* host) {
    CHECK(p.alloc(ctx, n));
    if (host && n) HIPCHK(hipMemcpyAsync(p, host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return AGGMG_OK;
  }
  int fetch(int64_t n, double* host) {
    if (n) HIPCHK(hipMemcpyAsync(host, p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return AGGMG_OK;
  }
};

extern "C" int aggmg_smooth(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, double* u_inout, const double* b,
                            double alpha, int nsweeps) {
  CHECK(check_pair(ctx, A, sm, "aggmg_smooth"));
  if (!u_inout || !b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smooth: NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t N = A->m;
  DevVec du(ctx), db(ctx), dout(ctx);
  CHECK(du.alloc(N, u_inout));
  CHECK(db.alloc(N, b));
  CHECK(dout.alloc(N, nullptr));
  CHECK(aggmg_smooth_dev(ctx, A, sm, du.p, db.p, alpha, nsweeps, dout.p));
  return dout.fetch(N, u_inout);
}

extern "C" int aggmg_residual(aggmg_ctx* ctx, aggmg_op* A, const double* u, const double* b, double* r_out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!A || !u || !b || !r_out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual: NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  DevVec du(ctx), db(ctx), dr(ctx);
  CHECK(du.alloc(A->n, u));
  CHECK(db.alloc(A->m, b));
  CHECK(dr.alloc(A->m, nullptr));
  CHECK(aggmg_residual_dev(ctx, A, du.p, db.p, dr.p));
  return dr.fetch(A->m, r_out);
}

extern "C" int aggmg_restrict(aggmg_ctx* ctx, aggmg_op* L, const double* r, double* rc_out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!L || !r || !rc_out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_restrict: NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  DevVec dr(ctx), dc(ctx);
  CHECK(dr.alloc(L->m, r));
  CHECK(dc.alloc(L->n, nullptr));
  CHECK(aggmg_restrict_dev(ctx, L, dr.p, dc.p));
  return dc.fetch(L->n, rc_out);
}

extern "C" int aggmg_prolong_add(aggmg_ctx* ctx, aggmg_op* L, const double* uc, double* u_inout) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!L || !uc || !u_inout) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_prolong_add: NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  DevVec dc(ctx), du(ctx);
  CHECK(dc.alloc(L->n, uc));
  CHECK(du.alloc(L->m, u_inout));
  CHECK(aggmg_prolong_add_dev(ctx, L, dc.p, du.p));
  return du.fetch(L->m, u_inout);
}

extern "C" int aggmg_smoother_apply(aggmg_ctx* ctx, aggmg_smoother* sm, const double* B, int64_t N, int64_t ncols,
                                    double alpha, double* Y) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!sm || !B || !Y) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_apply: NULL argument");
  if (N != sm->N || ncols < 0) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_smoother_apply: DimensionMismatch");
  HIPCHK(hipSetDevice(ctx->device));
  DevVec dB(ctx), dY(ctx), dT(ctx);
  CHECK(dB.alloc(N * ncols, B));
  CHECK(dY.alloc(N * ncols, nullptr));
  CHECK(dT.alloc(N, nullptr));
  const unsigned nb2 = (unsigned)((N + kThreads - 1) / kThreads);
  for (int64_t c = 0; c < ncols && N > 0; ++c) {
    const double* bc = dB.p + c * N;
    double* yc = dY.p + c * N;
    ProfScope ps(ctx, AGGMG_KIND_BLOCK_APPLY, 0);
    if (sm->patch) {
      // fused element-patch Schwarz: one sweep of weight alpha from the zero iterate is alpha * S^{-1} b
      CHECK(patch_smooth(ctx, *sm->patch, nullptr, bc, Damping(alpha), 1, yc, 0));
    } else if (sm->kind == 0) {
      // alpha * (Diagonal \ B): reuse the scaled-axpy kernel with counts := diag
      hipLaunchKernelGGL(axpy_scaled_kernel, dim3(nb2), dim3(kThreads), 0, ctx->stream, N, (const double*)nullptr,
                         bc, (const double*)sm->diag, alpha, yc);
    } else if (sm->overlapping) {
      // overlapping lists (additive / hybrid Schwarz, src/smoother.jl:6-46): the block results kept apart, then added
      // up per row in list order -- no atomics, the same bits run to run (r03: atomic adds into a zeroed vector)
      CHECK(setup_block_cover(ctx, sm));
      WorkLease lease;
      CHECK(scratch_lease(ctx, kScratchPong, std::max<int64_t>(N, sm->nb * sm->m), "aggmg_smoother_apply", &lease));
      double* Yf = lease;
      const unsigned nblk = (unsigned)((sm->nb * sm->m + kThreads - 1) / kThreads);
      if (nblk)
        hipLaunchKernelGGL(block_apply_flat_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, sm->binv, sm->inds, (int)sm->m,
                           sm->nb, bc, Yf);
      hipLaunchKernelGGL(block_combine_kernel, dim3(nb2), dim3(kThreads), 0, ctx->stream, N, (const int32_t*)sm->cover_ptr,
                         (const uint32_t*)sm->cover_idx, (const double*)Yf, (const double*)nullptr,
                         sm->kind == 2 ? (const double*)sm->counts : (const double*)nullptr, alpha, yc);
    } else {
      HIPCHK(hipMemsetAsync(dT.p, 0, N * sizeof(double), ctx->stream));
      const unsigned nblk = (unsigned)((sm->nb * sm->m + kThreads - 1) / kThreads);
      if (nblk)   // (lists that do not overlap: the branch above took the others)
        hipLaunchKernelGGL((block_apply_kernel<false>), dim3(nblk), dim3(kThreads), 0, ctx->stream, sm->binv,
                           sm->inds, (int)sm->m, sm->nb, bc, dT.p);
      hipLaunchKernelGGL(axpy_scaled_kernel, dim3(nb2), dim3(kThreads), 0, ctx->stream, N, (const double*)nullptr,
                         (const double*)dT.p, sm->kind == 2 ? (const double*)sm->counts : (const double*)nullptr,
                         alpha, yc);
    }
    HIPCHK(hipGetLastError());
  }
  return dY.fetch(N * ncols, Y);
}

// ---------------------------------------------------------------------------------------------
// coarsest-level direct solve (host, banded LU with partial pivoting = dgbtf2 / dgbtrs order)
// ---------------------------------------------------------------------------------------------
static bool banded_fits(int64_t kl, int64_t ku, int64_t n);   // the band storage stays below the solver's bound

static int banded_factor(aggmg_ctx* ctx, const HostCsr& h, int64_t n, BandedLU* f) {
  int kl = 0, ku = 0;
  for (int64_t i = 0; i < n; ++i)
    for (int32_t p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p) {
      const int64_t j = h.colind[p];
      kl = std::max<int64_t>(kl, i - j);
      ku = std::max<int64_t>(ku, j - i);
    }
  const int64_t ldab = 2 * (int64_t)kl + ku + 1;
  if (!banded_fits(kl, ku, n))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                "coarsest operator bandwidth too large for the host banded solver (kl=" + std::to_string(kl) +
                    ", ku=" + std::to_string(ku) + ", n=" + std::to_string(n) + ")");
  f->n = n;
  f->kl = kl;
  f->ku = ku;
  f->ldab = (int)ldab;
  f->ab.assign((size_t)ldab * n, 0.0);
  f->ipiv.assign(n, 0);
  const int kv = ku + kl;
  auto AB = [&](int64_t r, int64_t c) -> double& { return f->ab[(size_t)c * ldab + r]; };
  for (int64_t i = 0; i < n; ++i)
    for (int32_t p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p) {
      const int64_t j = h.colind[p];
      AB(kv + i - j, j) = h.vals[p];
    }
  int64_t ju = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t km = std::min<int64_t>(kl, n - 1 - j);
    int64_t jp = 0;
    double best = std::fabs(AB(kv, j));
    for (int64_t i = 1; i <= km; ++i) {
      const double v = std::fabs(AB(kv + i, j));
      if (v > best) {
        best = v;
        jp = i;
      }
    }
    f->ipiv[j] = (int32_t)(j + jp);
    if (AB(kv + jp, j) == 0.0)
      return fail(ctx, AGGMG_ERR_SINGULAR, "coarsest operator is singular (SingularException)");
    ju = std::max(ju, std::min<int64_t>(j + ku + jp, n - 1));
    if (jp != 0)
      for (int64_t c = j; c <= ju; ++c) std::swap(AB(kv + jp - (c - j), c), AB(kv - (c - j), c));
    if (km > 0) {
      const double rp = 1.0 / AB(kv, j);
      for (int64_t i = 1; i <= km; ++i) AB(kv + i, j) *= rp;
      for (int64_t c = j + 1; c <= ju; ++c) {
        const double t = AB(kv - (c - j), c);
        if (t != 0.0)
          for (int64_t i = 1; i <= km; ++i) AB(kv + i - (c - j), c) -= AB(kv + i, j) * t;
      }
    }
  }
  return AGGMG_OK;
}

static void banded_solve(const BandedLU& f, double* b) {
  const int64_t n = f.n, ldab = f.ldab;
  const int kl = f.kl, kv = f.ku + f.kl;
  auto AB = [&](int64_t r, int64_t c) -> double { return f.ab[(size_t)c * ldab + r]; };
  if (kl > 0)
    for (int64_t j = 0; j < n - 1; ++j) {
      const int64_t lm = std::min<int64_t>(kl, n - 1 - j);
      const int64_t l = f.ipiv[j];
      if (l != j) std::swap(b[l], b[j]);
      const double bj = b[j];
      for (int64_t i = 1; i <= lm; ++i) b[j + i] -= bj * AB(kv + i, j);
    }
  for (int64_t j = n - 1; j >= 0; --j) {
    b[j] /= AB(kv, j);
    const double bj = b[j];
    const int64_t lo = std::max<int64_t>(0, j - kv);
    for (int64_t i = lo; i < j; ++i) b[i] -= bj * AB(kv - (j - i), j);
  }
}

// ---------------------------------------------------------------------------------------------
// coarsest-level direct solve on the device: block cyclic reduction (factored once on the device,
// setup_cr in setup.hip; solved per cycle here)
// ---------------------------------------------------------------------------------------------
static int cr_stage_threads() {
  static const int t = std::min(std::max(env_int("AGGMG_CR_THREADS", kCrThreads), 64), kCrThreads);
  return t;
}

#ifdef AGGMG_CR_TRACE
// tracing build only (tools/cr_trace.py builds it beside the product library): constant-clock stamps per workgroup
static unsigned long long* g_cr_trace = nullptr;
static constexpr size_t kCrTraceWords = (size_t)3 * kCrTraceWgs * 16;
extern "C" int aggmg_debug_cr_trace(aggmg_ctx* ctx, unsigned long long* out, int clear) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!g_cr_trace) {
    HIPCHK(hipMalloc((void**)&g_cr_trace, kCrTraceWords * 8));
    HIPCHK(hipMemset(g_cr_trace, 0, kCrTraceWords * 8));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (out) HIPCHK(hipMemcpy(out, g_cr_trace, kCrTraceWords * 8, hipMemcpyDeviceToHost));
  if (clear) HIPCHK(hipMemset(g_cr_trace, 0, kCrTraceWords * 8));
  return AGGMG_OK;
}
#endif

// AGGMG_CR_FUSE_TAIL=1 (experiment): the last forward stage's last-arriving workgroup solves the tail system
static bool cr_fuse_tail() {
  static const bool on = [] {
    const char* e = std::getenv("AGGMG_CR_FUSE_TAIL");
    return e && e[0] == '1';
  }();
  return on;
}

// kc columns in h->crw, which cr_multi_workspace has laid out for h->crw_cols >= kc of them
static CrRun cr_run_cols(const aggmg_hier* h, int kc) {
  const CrDev& cr = h->cr;
  std::vector<CrMultiStage> ws;
  CrMultiStage wt;
  cr_multi_layout(cr.st, cr.tail, cr.m, h->crw_cols, &ws, &wt);
  double* const w = h->crw;
  auto at = [&](int64_t stride, int64_t off) -> double* { return stride ? w + off : nullptr; };
  CrRun run;
  run.kc = kc;
  run.st.reserve(ws.size());
  for (const CrMultiStage& W : ws) {
    double* const part = w + W.part_off;
    run.st.push_back({part, part + W.part / 3, part + 2 * (W.part / 3), at(W.stack, W.stack_off), at(W.mid, W.mid_off), W.part,
                      W.stack, W.mid});
  }
  run.tail.mid = at(wt.mid, wt.mid_off);
  run.tail.cs_mid = wt.mid;
  return run;
}

// the arguments of a launch of stage S (or the tail) on the run's entry R for it; what depends on where the stage's input
// and output lie (cs_d, cs_x, dstride, ostride, c0) is the caller's
enum CrKind { kCrForward = 0, kCrTail = 1, kCrBackward = 2 };   // (the tracing build's trace_kind)
static CrStageArgs cr_make_args(const CrDev& cr, const CrStagePlan& S, const CrRunStage& R, CrKind kind) {
  CrStageArgs A;
  std::memset(&A, 0, sizeof(A));
#ifdef AGGMG_CR_TRACE
  A.trace = g_cr_trace;
  A.trace_kind = kind;
#endif
  A.q = S.q;
  for (int l = 0; l < S.q; ++l) A.lv[l] = cr.lv[S.l0 + l];
  A.nsteps = S.nsteps;
  for (int s = 0; s <= kCrMaxSteps; ++s) {
    A.step_a[s] = S.step_a[s];
    A.lds_off[s] = S.lds_off[s];
    A.lds_xoff[s] = S.lds_xoff[s];
  }
  A.lds_total = S.lds_total;
  A.n_out = S.n_out;
  A.stack = R.stack;
  A.stack_stride = S.stack_stride;
  A.mid = R.mid;
  for (int s = 0; s <= kCrMaxSteps; ++s) A.mid_off[s] = S.mid_off[s];
  A.tail = kind == kCrTail ? 1 : 0;
  A.lu_last = cr.lu_last;
  A.perm_last = cr.perm_last;
  A.cs_o = A.cs_xq = R.cs_part;
  A.cs_stack = R.cs_stack;
  A.cs_mid = R.cs_mid;
  return A;
}

// the tail system: parallel cyclic reduction when set-up prepared it, the register-blocked reduction otherwise
template <int M>
static void cr_launch_tail(aggmg_ctx* ctx, CrDev& cr, const CrStageArgs& T, size_t tail_lds, const double* d, const double* db,
                           double* x, int kc = 1) {
  if constexpr (M <= 2) {
    if (cr.pcr.valid) {
      PcrArgs P;
      std::memset(&P, 0, sizeof(P));
      P.mult = cr.pcr.mult;
      P.lu = cr.pcr.lu;
      P.perm = cr.pcr.perm;
      P.n = cr.pcr.n;
      P.L = cr.pcr.L;
      P.dstride = T.dstride;
      P.cs_d = T.cs_d;
      P.cs_x = T.cs_x;
#ifdef AGGMG_CR_TRACE
      P.trace = g_cr_trace;
#endif
      const unsigned threads = (unsigned)((cr.pcr.n + 63) / 64 * 64);
      const size_t lds = (size_t)2 * (cr.pcr.n + 1) * M * sizeof(double);
      if (cr.pcr.pre) {
        P.lv0 = cr.lv[cr.tail.l0];
        P.n_full = (int)cr.tail.n_in;
        hipLaunchKernelGGL((cr_pcr_tail_kernel<M, true>), dim3(1, kc), dim3(threads), lds, ctx->stream, P, d, db, x);
      } else {
        hipLaunchKernelGGL((cr_pcr_tail_kernel<M, false>), dim3(1, kc), dim3(threads), lds, ctx->stream, P, d, db, x);
      }
      return;
    }
  }
  hipLaunchKernelGGL((cr_tail_kernel<M>), dim3(1, kc), dim3(kCrThreads), tail_lds, ctx->stream, T, d, db, x);
}

// where a launch of stage S finds the stage's table and class indices (S.dict.take; AGGMG_OPT_COARSE_DICTIONARY)
static CrDictArgs cr_make_dict_args(const CrStage& S) {
  CrDictArgs D;
  std::memset(&D, 0, sizeof(D));
  D.tab = S.dict_tab;
  D.cidx = S.dict_idx;
  for (int l = 0; l < S.q; ++l) {
    D.tab_e[l] = S.dict.tab_e[l];
    D.tab_o[l] = S.dict.tab_o[l];
    D.idx_e[l] = S.dict.idx_e[l];
    D.idx_o[l] = S.dict.idx_o[l];
  }
  D.tab_words = S.dict.tab_words;
  D.idx_count = S.dict.idx_count;
  D.tab_off = S.dict.tab_off;
  D.idx_off = S.dict.idx_off;
  return D;
}

// one launch of stage S's forward / backward kernel: chunks A.c0 .. A.c0 + grid of kc columns; a stage that took the
// dictionary form runs the kernels that read its factors from LDS
template <int M, bool FUSE_TAIL = false>
static void cr_launch_forward(aggmg_ctx* ctx, const CrStage& S, const CrStageArgs& A, unsigned grid, int kc, const double* d,
                              const double* db, double* partR, double* partL, const CrStageArgs& T, size_t tail_lds = 0,
                              double* xt = nullptr, unsigned int* ticket = nullptr) {
  if constexpr (cr_dict_form(M)) {
    if (S.dict.take) {
      hipLaunchKernelGGL((cr_stage_forward_dict_kernel<M, FUSE_TAIL>), dim3(grid, kc), dim3(cr_stage_threads()),
                         std::max(S.dict.lds_bytes, tail_lds), ctx->stream, A, cr_make_dict_args(S), d, db, partR, partL, T, xt,
                         ticket);
      ++ctx->coarse_dict_launches;
      return;
    }
  }
  hipLaunchKernelGGL((cr_stage_forward_kernel<M, FUSE_TAIL>), dim3(grid, kc), dim3(cr_stage_threads()),
                     std::max((size_t)A.lds_total * sizeof(double), tail_lds), ctx->stream, A, d, db, partR, partL, T, xt, ticket);
}
template <int M>
static void cr_launch_backward(aggmg_ctx* ctx, const CrStage& S, const CrStageArgs& A, unsigned grid, int kc, const double* d,
                               const double* db, const double* xq, double* x) {
  if constexpr (cr_dict_form(M)) {
    if (S.dict.take) {
      hipLaunchKernelGGL((cr_stage_backward_dict_kernel<M>), dim3(grid, kc), dim3(cr_stage_threads()), S.dict.lds_bytes,
                         ctx->stream, A, cr_make_dict_args(S), d, db, xq, x);
      ++ctx->coarse_dict_launches;
      return;
    }
  }
  hipLaunchKernelGGL((cr_stage_backward_kernel<M>), dim3(grid, kc), dim3(cr_stage_threads()), (size_t)A.lds_total * sizeof(double),
                     ctx->stream, A, d, db, xq, x);
}

// Stages s0.. and the tail for the right-hand sides d (+ db) of stage s0's input system into x, for the run's columns:
// forward launches stage by stage, the tail system (AGGMG_CR_FUSE_TAIL=1, one column: in the last forward launch's
// last-arriving workgroup), then the back substitutions in reverse.  Stage s0 reads and writes the caller's vectors, every
// later stage the boundary system of the stage before it.
// cs_in / cs_out: doubles between consecutive columns of d (db) / x
// dstride: doubles between consecutive blocks of d / db (0 = M; 2 M: the chunk-interleaved boundary rows of an
// element-partitioned run, gathered in place)
template <int M>
static int cr_walk(aggmg_ctx* ctx, CrDev& cr, const CrRun& run, int s0, const double* d, const double* db, double* x,
                   int64_t cs_in, int64_t cs_out, int dstride) {
  const int ns = (int)cr.st.size(), kc = run.kc;
  CrStageArgs T = cr_make_args(cr, cr.tail, run.tail, kCrTail);
  const size_t tail_lds = (size_t)cr.tail.lds_total * sizeof(double);
  if (s0 >= ns) {
    T.dstride = dstride;
    T.cs_d = cs_in;
    T.cs_x = cs_out;
    cr_launch_tail<M>(ctx, cr, T, tail_lds, d, db, x, kc);
    HIPCHK(hipGetLastError());
    return AGGMG_OK;
  }
  struct Io {
    const double *d, *db;
    double* x;
    int64_t cs_d, cs_x;
    int dstride;
  };
  auto io = [&](int s) -> Io {
    if (s == s0) return {d, db, x, cs_in, cs_out, dstride};
    const CrRunStage& P = run.st[s - 1];
    return {P.partR, P.partL, P.xq, P.cs_part, P.cs_part, 0};
  };
  const bool fuse_tail = kc == 1 && cr_fuse_tail();
  for (int s = s0; s < ns; ++s) {
    const CrRunStage& R = run.st[s];
    const Io in = io(s);
    CrStageArgs A = cr_make_args(cr, cr.st[s], R, kCrForward);
    A.cs_d = in.cs_d;
    A.dstride = in.dstride;
    const unsigned grid = (unsigned)std::max<int64_t>(A.n_out, 1);
    if (s == ns - 1 && fuse_tail) {
      cr_launch_forward<M, true>(ctx, cr.st[s], A, grid, kc, in.d, in.db, R.partR, R.partL, T, tail_lds, R.xq, cr.ticket);
    } else {
      cr_launch_forward<M>(ctx, cr.st[s], A, grid, kc, in.d, in.db, R.partR, R.partL, T);
      if (s == ns - 1) {
        T.cs_d = T.cs_x = R.cs_part;
        cr_launch_tail<M>(ctx, cr, T, tail_lds, R.partR, R.partL, R.xq, kc);
      }
    }
  }
  for (int s = ns - 1; s >= s0; --s) {
    const Io in = io(s);
    CrStageArgs A = cr_make_args(cr, cr.st[s], run.st[s], kCrBackward);
    A.cs_d = in.cs_d;
    A.cs_x = in.cs_x;
    A.dstride = in.dstride;
    cr_launch_backward<M>(ctx, cr.st[s], A, (unsigned)std::max<int64_t>(A.n_out, 1), kc, in.d, in.db, run.st[s].xq, in.x);
  }
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// ---- stage 0 for the chunks of a block range alone (element-partitioned runs: every rank eliminates / back-substitutes
// only the stage-0 chunks of its own blocks; the boundary system in between is gathered and solved redundantly: cr_walk
// from stage 1).  The boundary rows are the caller's: partR / partL written (block stride ostride, 0 = M), xq read ------
template <int M>
static int cr_chunks(aggmg_ctx* ctx, CrDev& cr, bool backward, const double* d_owned, int64_t blk_lo, int64_t blk_hi,
                     double* partR, double* partL, const double* xq, double* x_owned, int ostride) {
  const CrStage& S = cr.st[0];
  CrStageArgs A = cr_make_args(cr, S, cr_run_stage(S), backward ? kCrBackward : kCrForward);
  A.ostride = ostride;
  A.c0 = blk_lo >> S.q;
  const int64_t c1 = (blk_hi + ((int64_t)1 << S.q) - 1) >> S.q;
  const unsigned grid = (unsigned)std::max<int64_t>(c1 - A.c0, 0);
  if (!grid) return AGGMG_OK;
  const double* d0 = d_owned - blk_lo * M;  // global block indexing; only owned blocks are touched
  if (backward) {
    cr_launch_backward<M>(ctx, S, A, grid, 1, d0, nullptr, xq, x_owned - blk_lo * M);
  } else {
    CrStageArgs T;
    std::memset(&T, 0, sizeof(T));
    cr_launch_forward<M>(ctx, S, A, grid, 1, d0, nullptr, partR, partL, T);
  }
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// f(std::integral_constant<int, M>) -> status, for the factorisation's block size
template <class F>
static int cr_with_m(aggmg_ctx* ctx, const CrDev& cr, F&& f) {
  int rc = AGGMG_OK;
  if (!with_block_size<cr_form>(cr.m, [&](auto m) { rc = f(m); }))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "cyclic reduction block size not instantiated");
  return rc;
}

// phase 0: chunk forward, 1: boundary system, 2: chunk backward; pstride: block stride of partR / partL
static int cr_phase(aggmg_ctx* ctx, CrDev& cr, int phase, const double* d_owned, int64_t blk_lo, int64_t blk_hi,
                    double* partR, double* partL, const double* xq, double* x_owned, int pstride = 0) {
  ProfScope ps(ctx, AGGMG_KIND_COARSE, 0);
  return cr_with_m(ctx, cr, [&](auto m) {
    constexpr int M = decltype(m)::value;
    if (phase == 1) return cr_walk<M>(ctx, cr, cr.run, 1, partR, partL, const_cast<double*>(xq), 0, 0, pstride);
    return cr_chunks<M>(ctx, cr, phase == 2, d_owned, blk_lo, blk_hi, partR, partL, xq, x_owned, pstride);
  });
}

// the K-column buffers (cr_run_cols) and staging vectors: grown to the largest group asked for; a call with no more
// columns than before allocates nothing
static int cr_multi_workspace(aggmg_ctx* ctx, aggmg_hier* h, int64_t cols, bool staging) {
  const CrDev& cr = h->cr;
  if (h->crw_cols < cols) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    h->crw_cols = 0;
    std::vector<CrMultiStage> st;
    CrMultiStage tail;
    CHECK(h->crw.alloc(ctx, cr_multi_layout(cr.st, cr.tail, cr.m, cols, &st, &tail), true));   // (partL[0] of every column is never written: stays zero)
    h->crw_cols = cols;
  }
  if (staging && h->crw_stage_cols < cols) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    h->crw_stage_cols = 0;
    CHECK(h->crw_stage.alloc(ctx, 2 * cols * cr_even(cr.n0 * cr.m), true));   // (the pad rows of d0 are never written: stay zero)
    h->crw_stage_cols = cols;
  }
  return AGGMG_OK;
}

// the staging launches, rows x kc columns.  Element-chain order: the operator's numbering -> block order and back
static dim3 cr_cols_grid(int64_t n, int kc) { return dim3((unsigned)((n + kCrThreads - 1) / kCrThreads), kc); }
static void cr_chain_gather(aggmg_ctx* ctx, const CgtDev& g, int64_t n, int kc, const double* B, int64_t ldb, double* d0, int64_t sp) {
  hipLaunchKernelGGL(cr_chain_gather_kernel<kCrThreads>, cr_cols_grid(n, kc), dim3(kCrThreads), 0, ctx->stream, B, ldb,
                     (const int32_t*)g.perm, d0, sp, n);
}
static void cr_chain_scatter(aggmg_ctx* ctx, const CgtDev& g, int kc, const double* x0, int64_t sp, double* X, int64_t ldx) {
  hipLaunchKernelGGL(cr_chain_scatter_kernel<kCrThreads>, cr_cols_grid(g.N, kc), dim3(kCrThreads), 0, ctx->stream, x0, sp,
                     (const int32_t*)g.inv, X, ldx, g.N);
}
static void cr_cols_copy(aggmg_ctx* ctx, int64_t n, int kc, const double* src, int64_t ld_src, double* dst, int64_t ld_dst) {
  hipLaunchKernelGGL(cr_cols_copy_kernel<kCrThreads>, cr_cols_grid(n, kc), dim3(kCrThreads), 0, ctx->stream, src, ld_src, dst, ld_dst, n);
}

// Column j < kc of X (leading dimension ldx) = the solve of column j of B (ldb), in the operator's numbering; one launch
// sequence for the group (EXTENSION: the K-column cycle's coarsest level), every column with the bits of a one-column call
// (which passes ldb = ldx = 0).  Workgroup (chunk, col) of every launch runs what workgroup `chunk` of a one-column launch
// runs, on column col's vectors (cr_kernels.hpp).
// The caller's columns are used in place unless the system is padded (N no multiple of M), B and X overlap (one column:
// are the same vector), the blocks are in element-chain order, or a column of a group lies off the 16 bytes the kernels'
// paired loads and stores assume of a vector.  Then the walk runs on block-ordered staging vectors with zero pad rows -- one column: cr.d0 / cr.x0, filled and
// emptied by copies; a group: h->crw_stage, by one copy launch each way; chain order: by the gather / scatter launches.
template <int M>
static int cr_solve_cols(aggmg_ctx* ctx, aggmg_hier* h, const double* B, int64_t ldb, double* X, int64_t ldx, int kc) {
  CrDev& cr = h->cr;
  const int64_t Npad = cr.n0 * M;
  const bool aligned = kc == 1 || ((((uintptr_t)B | (uintptr_t)X) & 15) == 0 && ldb % 2 == 0 && ldx % 2 == 0);
  const bool overlap = kc == 1 ? B == X : B < X + ((kc - 1) * ldx + cr.N) && X < B + ((kc - 1) * ldb + cr.N);
  const bool direct = !cr.chain && Npad == cr.N && aligned && !overlap;
  if (kc > 1) {
    CHECK(cr_multi_workspace(ctx, h, kc, !direct));
  } else if (!direct && !cr.d0) {  // in-place call on an unpadded system: staging vectors on first use
    for (DevArray<double>* p : {&cr.d0, &cr.x0}) CHECK(p->alloc(ctx, Npad));
  }
  const double* d = B;
  double* x = X;
  int64_t cs_in = ldb, cs_out = ldx;
  if (!direct) {
    const int64_t sp = kc == 1 ? 0 : cr_even(Npad);
    double* d0 = kc == 1 ? cr.d0.get() : h->crw_stage.get();
    x = kc == 1 ? cr.x0.get() : h->crw_stage + h->crw_stage_cols * sp;
    if (cr.chain) {
      cr_chain_gather(ctx, *cr.chain, Npad, kc, B, ldb, d0, sp);
    } else if (kc == 1) {
      if (Npad > cr.N) HIPCHK(hipMemsetAsync(d0 + cr.N, 0, (Npad - cr.N) * sizeof(double), ctx->stream));
      HIPCHK(hipMemcpyAsync(d0, B, cr.N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
      cr_cols_copy(ctx, cr.N, kc, B, ldb, d0, sp);
    }
    d = d0;
    cs_in = cs_out = sp;
  }
  CrRun cols;
  if (kc > 1) cols = cr_run_cols(h, kc);
  CHECK(cr_walk<M>(ctx, cr, kc == 1 ? cr.run : cols, 0, d, nullptr, x, cs_in, cs_out, 0));
  if (cr.chain) {
    cr_chain_scatter(ctx, *cr.chain, kc, x, cs_out, X, ldx);
  } else if (!direct && kc == 1) {
    HIPCHK(hipMemcpyAsync(X, x, cr.N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  } else if (!direct) {
    cr_cols_copy(ctx, cr.N, kc, x, cs_out, X, ldx);
  }
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int cr_solve(aggmg_ctx* ctx, aggmg_hier* h, const double* B, int64_t ldb, double* X, int64_t ldx, int kc) {
  ProfScope ps(ctx, AGGMG_KIND_COARSE, (int)h->lv.size() - 1);
  return cr_with_m(ctx, h->cr, [&](auto m) { return cr_solve_cols<decltype(m)::value>(ctx, h, B, ldb, X, ldx, kc); });
}

// ---------------------------------------------------------------------------------------------
// the coarsest factorisation, accepted on evidence
// ---------------------------------------------------------------------------------------------
static bool banded_fits(int64_t kl, int64_t ku, int64_t n) { return (double)(2 * kl + ku + 1) * (double)n * 8.0 <= 8e9; }

// keeps or discards h->cr (and its parallel tail) on probe solves; the backward error goes to h->cr_probe_backward_error
static int coarse_accept(aggmg_ctx* ctx, aggmg_hier* h) {
  const int nlv = (int)h->lv.size();
  aggmg_op* Ac = h->lv[nlv - 1].A;
  const bool chain = (bool)h->cr.chain;
  static const bool probe = [] {
    const char* e = std::getenv("AGGMG_CR_PROBE");   // =0: debugging aid, accept the factorisation unchecked
    return !(e && e[0] == '0');
  }();
  if (h->cr.valid && probe) {
    // The cyclic reduction pivots inside the m x m blocks only (the reference's UMFPACK pivots across the whole
    // matrix, src/solvers.jl:39): accept the factorisation on evidence, not on the per-block condition monitor
    // alone -- solve one probe system and keep it only if the backward error is at round-off level.
    Level& lc = h->lv[nlv - 1];
    const int64_t Nc = lc.N;
    const double tol = 1e-10;
    // the operator's products.  Operator order: the deterministic gather of the uploaded CSC arrays, which relies on the
    // block-tridiagonal pattern the set-up has established.  Chain order: the row-gather CSR in the OPERATOR's numbering --
    // not the chain arrays the blocks were packed from, where a packing or permutation mistake would cancel
    auto product = [&](const double* w, double* d) -> int {
      if (chain) return launch_csr<kSpmvSet>(ctx, Ac->csr, w, nullptr, nullptr, 0.0, d);
      HIPCHK(hipMemsetAsync(d, 0, (size_t)Nc * sizeof(double), ctx->stream));
      return setup_band_matvec_add(ctx, Ac, h->cr.m, w, 1.0, d);
    };
    auto residual = [&](const double* x, const double* d, double* r) -> int {
      if (chain) return launch_csr<kResidual>(ctx, Ac->csr, x, d, nullptr, 0.0, r);
      HIPCHK(hipMemcpyAsync(r, d, (size_t)Nc * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      return setup_band_matvec_add(ctx, Ac, h->cr.m, x, -1.0, r);
    };
    auto probe_once = [&]() -> int {
      double nd = 0.0, nr = 0.0;
      CHECK(setup_probe_vector(ctx, Nc, lc.u[1]));
      CHECK(product(lc.u[1], lc.rhs));                                          // d = A w (deterministic gather)
      CHECK(cr_solve(ctx, h, lc.rhs, 0, lc.u[0], 0, 1));                        // x = CR(d)
      CHECK(residual(lc.u[0], lc.rhs, lc.tmp));                                 // r = d - A x
      CHECK(aggmg_norm2_dev(ctx, lc.rhs, Nc, &nd));
      CHECK(aggmg_norm2_dev(ctx, lc.tmp, Nc, &nr));
      h->cr_probe_backward_error = nd > 0.0 ? nr / nd : 0.0;
      for (double* p : {lc.u[0].get(), lc.u[1].get(), lc.rhs.get(), lc.tmp.get()}) HIPCHK(hipMemsetAsync(p, 0, (size_t)lc.Nalloc * sizeof(double), ctx->stream));
      return AGGMG_OK;
    };
    CHECK(probe_once());
    if (!(h->cr_probe_backward_error < tol) && h->cr.pcr.valid) {  // the tail once more in its register-blocked form
      h->cr.pcr.valid = false;
      CHECK(probe_once());
    }
    if (!(h->cr_probe_backward_error < tol)) cr_discard(&h->cr);              // NaN included
    static const bool pcr_guard = [] {
      const char* e = std::getenv("AGGMG_CR_PCR_GUARD");   // =0: testing aid, keep the parallel tail unexamined
      return !(e && e[0] == '0');
    }();
    if (h->cr.valid && h->cr.pcr.valid && pcr_guard) {
      // The parallel cyclic reduction of the tail accumulates like an inverse; on an ill-conditioned tail system (a
      // small coarsest operator taken as a whole: Neumann end, Dirichlet penalty) its residual for a right-hand side
      // with a large smooth solution was measured at 5000 x the register-blocked form's (1.8e-8 against 3.4e-12 of
      // ||d||, tests/exp_pcr_accuracy.py), on the boundary systems of the benchmarked hierarchies at 1 - 4 x.  So it
      // is kept on evidence as well: both forms solve one such system, and the parallel one stays only where its
      // residual is within 8 x of the other's.
      auto smooth_residual = [&](double* res) -> int {
        double nd = 0.0, nr = 0.0;
        CHECK(setup_smooth_vector(ctx, Nc, lc.rhs));
        CHECK(cr_solve(ctx, h, lc.rhs, 0, lc.u[0], 0, 1));
        CHECK(residual(lc.u[0], lc.rhs, lc.tmp));
        CHECK(aggmg_norm2_dev(ctx, lc.rhs, Nc, &nd));
        CHECK(aggmg_norm2_dev(ctx, lc.tmp, Nc, &nr));
        *res = nd > 0.0 ? nr / nd : 0.0;
        return AGGMG_OK;
      };
      double rp = 0.0, rc = 0.0;
      CHECK(smooth_residual(&rp));
      h->cr.pcr.valid = false;
      CHECK(smooth_residual(&rc));
      h->cr.pcr.valid = rp <= 8.0 * rc + 1e-15;   // (NaN: false)
      for (double* p : {lc.u[0].get(), lc.u[1].get(), lc.rhs.get(), lc.tmp.get()}) HIPCHK(hipMemsetAsync(p, 0, (size_t)lc.Nalloc * sizeof(double), ctx->stream));
    }
  }
  return AGGMG_OK;
}

// The coarsest operator in element-chain order (AGGMG_COARSE_DEVICE_CHAIN; AGGMG_COARSE_AUTO where the band is too wide
// for the host solver): the chain form a smoother left on the operator, or -- AGGMG_OPT_DETECT_CHAIN -- the one found from
// its pattern; the same cyclic reduction on its blocks; the same probe.  Leaves h->cr invalid and says *why otherwise.
static int coarse_factor_chain(aggmg_ctx* ctx, aggmg_hier* h, std::string* why) {
  aggmg_op* Ac = h->lv.back().A;
  cr_discard(&h->cr);
  std::shared_ptr<CgtDev> g = Ac->cgt;
  if (!g && ctx->detect_chain) {   // a throw-away point-Jacobi smoother: the detection wants one; the operator stays as it was
    aggmg_smoother probe_sm;
    probe_sm.A = Ac;
    probe_sm.N = Ac->m;
    const int st = cgt_detect(ctx, &probe_sm);
    Ac->cgt = nullptr;
    CHECK(st);
    g = probe_sm.cgt;
  }
  if (!g) {
    // the wording only: does the operator have the size and the entry count of a CG chain of a degree above 8 (the bounds
    // of cgt_detect)?  No chain form is built for those
    int64_t big = 0;
    for (int64_t p = 9; p <= 64 && !big && Ac->m == Ac->n; ++p) {
      if ((Ac->m - 1) % p || Ac->m < 3) continue;
      const double full = (double)((Ac->m - 1) / p) * (double)((p + 1) * (p + 1));
      if ((double)Ac->nnz <= full && (double)Ac->nnz >= 0.5 * full) big = p;
    }
    *why = std::string("the coarsest operator has no element-chain form (no chain smoother was built on it") +
           (ctx->detect_chain ? ", none detected in its pattern)" : ", AGGMG_OPT_DETECT_CHAIN is off)");
    if (big)
      *why += "; its size and entry count would fit a chain with blocks of m = " + std::to_string(big) +
              " rows, and m > 8 is not covered";
    return AGGMG_OK;
  }
  if (g->m < 1 || g->m > 8) {   // (no CgtDev of today has such blocks)
    *why = "the element chain has blocks of m = " + std::to_string(g->m) + " rows; m > 8 is not covered";
    return AGGMG_OK;
  }
  CHECK(setup_cr_chain(ctx, *g, &h->cr));
  if (!h->cr.valid) {
    *why = "a pivot block of the chain-ordered operator is singular or close to it";
    return AGGMG_OK;
  }
  h->cr.chain = g;
  const bool had_csr = (bool)Ac->csr.rowptr;
  CHECK(op_ensure_csr(ctx, Ac));
  const int st = coarse_accept(ctx, h);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (!had_csr) Ac->csr = CsrDev();   // built for the probe alone: the operator holds what it held before
  CHECK(st);
  if (!h->cr.valid) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.3e", h->cr_probe_backward_error);
    *why = std::string("the probe solve refused the factorisation (backward error ") + buf + ", bound 1e-10)";
  }
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// hierarchy + V-cycle
// ---------------------------------------------------------------------------------------------
extern "C" int aggmg_hier_free(aggmg_ctx* ctx, aggmg_hier* h) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h) return AGGMG_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  delete h;  // the destructor frees the level vectors, transfers and the coarsest factorisation
  return AGGMG_OK;
}

static bool pair_level_ok(const aggmg_hier* h, int k);   // (with the two-level launches, below)

extern "C" int aggmg_hier_create(aggmg_ctx* ctx, int nlevels, aggmg_op* const* stiffness,
                                 aggmg_smoother* const* smoothers, aggmg_op* const* interpolation,
                                 int coarse_mode, aggmg_hier** out) {
  if (!ctx || !out || !stiffness) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_create: NULL argument");
  *out = nullptr;
  if (nlevels < 1 || nlevels > 16) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_create: nlevels must be in 1..16");
  if (nlevels > 1 && (!smoothers || !interpolation))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_create: smoothers / interpolation missing");
  if (coarse_mode != AGGMG_COARSE_HOST_BANDED && coarse_mode != AGGMG_COARSE_DEVICE_CR &&
      coarse_mode != AGGMG_COARSE_AUTO && coarse_mode != AGGMG_COARSE_EXTERNAL && coarse_mode != AGGMG_COARSE_DEVICE_CHAIN)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_create: unknown coarse_mode");
  HIPCHK(hipSetDevice(ctx->device));
  std::unique_ptr<aggmg_hier> h(new aggmg_hier());
  h->restriction = default_restriction();
  h->coarse_mode = coarse_mode;
  h->lv.resize(nlevels);
  for (int k = 0; k < nlevels; ++k)
    if (!stiffness[k] || stiffness[k]->m != stiffness[k]->n)
      return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_hier_create: stiffness must be square (and not NULL)");
  for (int k = 0; k < nlevels; ++k) {
    Level& l = h->lv[k];
    l.A = stiffness[k];
    l.N = l.A->m;
    l.Nalloc = l.N;
    if (k < nlevels - 1) {
      l.S = smoothers[k];
      l.L = interpolation[k];
      if (!l.S || !l.L) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_create: NULL smoother / interpolation");
      if (l.S->N != l.N) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_hier_create: smoother size mismatch at level " + std::to_string(k + 1));
      if (l.L->m != l.N || l.L->n != stiffness[k + 1]->m)
        return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_hier_create: interpolation size mismatch at level " + std::to_string(k + 1));
      if (l.L->kind != AGGMG_OP_TRANSFER) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_create: interpolation must be uploaded with AGGMG_OP_TRANSFER");
      if (l.S->cgt && l.S->A == l.A) l.Nalloc = std::max(l.N, l.S->cgt->ne * l.S->cgt->m);  // block order incl. padding
    }
    for (DevArray<double>* p : {&l.u[0], &l.u[1], &l.rhs, &l.tmp}) CHECK(p->alloc(ctx, l.Nalloc, true));
  }
  // structured transfers between consecutive levels whose fine side runs the fused kernel
  for (int k = 0; k + 1 < nlevels; ++k) {
    Level& l = h->lv[k];
    const BtdDev* eb = level_btd(l);   // the block-Jacobi smoother's form, or the element blocks of a patch smoother
    if (!eb) continue;
    int hint = 0;
    if (k + 2 < nlevels && level_btd(h->lv[k + 1])) hint = level_btd(h->lv[k + 1])->m;
    auto tb = std::make_unique<TransferBtd>();
    bool ok = false;
    // every fine row's stored columns must lie in the mc modes of coarse element (fine element) / rho
    CHECK(setup_transfer_btd(ctx, l.L, eb, eb->m, eb->ne, hint, tb.get(), &ok));
    if (ok) l.tb = std::move(tb);
    // the level's distinct operator records, where they are few (AGGMG_OPT_OPERATOR_DICTIONARY): block-Jacobi levels,
    // and the transfer launches of a patch level (patch_down / patch_up)
    if (l.tb && ctx->op_dict) CHECK(setup_op_dictionary(ctx, *eb, *l.tb, &l.dict));
  }
  // the same for the levels a two-level launch may take (pair_ok: below the finest, above the coarsest)
  for (int k = 1; ctx->op_dict && k + 1 < nlevels; ++k) {
    Level& l = h->lv[k];
    if (pair_level_ok(h.get(), k)) CHECK(setup_pair_dictionary(ctx, *l.S->btd, *l.tb, &l.pdict));
  }
  // CG chain levels: structured transfer to the next level; a level is fused when it has both
  for (int k = 0; k + 1 < nlevels; ++k) {
    Level& l = h->lv[k];
    if (!(l.S->cgt && l.S->A == l.A)) continue;
    const Level& c = h->lv[k + 1];
    const CgtDev* coarse = (c.S && c.S->cgt && c.S->A == c.A) ? c.S->cgt.get() : nullptr;
    int hint = 0;
    if (c.S && c.S->btd && c.S->A == c.A) hint = c.S->btd->m;
    auto tc = std::make_unique<TransferCgt>();
    bool ok = false;
    CHECK(cgt_build_transfer(ctx, l.L, *l.S->cgt, coarse, hint, tc.get(), &ok));
    if (ok) {
      l.tc = std::move(tc);
      l.cgt_fused = true;
      // the level's distinct operator records, where they are few (AGGMG_OPT_OPERATOR_DICTIONARY)
      if (ctx->op_dict) CHECK(setup_cgt_dictionary(ctx, *l.S->cgt, *l.tc, &l.cdict));
    }
  }
  // a fused chain level below a fused chain level keeps its rhs / result in block order
  for (int k = 0; k + 2 < nlevels; ++k)
    if (h->lv[k].cgt_fused && h->lv[k].tc->type == kTrChain && h->lv[k + 1].cgt_fused) h->lv[k + 1].native_io = true;
  // coarsest level: factor once (unless the caller solves it elsewhere)
  if (coarse_mode == AGGMG_COARSE_DEVICE_CHAIN) {
    std::string why;
    CHECK(coarse_factor_chain(ctx, h.get(), &why));
    if (!h->cr.valid) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_hier_create: AGGMG_COARSE_DEVICE_CHAIN: " + why);
  } else if (coarse_mode != AGGMG_COARSE_EXTERNAL) {
    aggmg_op* Ac = h->lv[nlevels - 1].A;
    std::string chain_why;   // AUTO: why the chain order was tried and refused
    if (coarse_mode != AGGMG_COARSE_HOST_BANDED) {
      int hint = 0, band[2] = {0, 0};
      if (nlevels >= 2 && h->lv[nlevels - 2].tb) hint = h->lv[nlevels - 2].tb->mc;
      CHECK(setup_cr(ctx, Ac, hint, &h->cr, band));
      CHECK(coarse_accept(ctx, h.get()));
      if (!h->cr.valid && coarse_mode == AGGMG_COARSE_DEVICE_CR)
        return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                    "aggmg_hier_create: coarsest operator is not block-tridiagonal with well-conditioned pivot "
                    "blocks; device cyclic reduction not applicable");
      // AUTO, and only where the host banded LU below would refuse the operator for its band (a CG operator in the
      // reference's vertices-first numbering): the element-chain order first.  Every other operator keeps its route.
      if (!h->cr.valid && Ac->m > 0 && !banded_fits(band[0], band[1], Ac->m)) {
        const double probe_before = h->cr_probe_backward_error;
        CHECK(coarse_factor_chain(ctx, h.get(), &chain_why));
        if (!h->cr.valid) h->cr_probe_backward_error = probe_before;
      }
    }
    if (!h->cr.valid) {  // host banded LU with partial pivoting: the one set-up path that reads the operator back
      HostCsr hc;
      CHECK(op_host_csr(ctx, Ac, &hc));
      const int st = banded_factor(ctx, hc, Ac->m, &h->coarse);
      if (st != AGGMG_OK && !chain_why.empty()) ctx->err += "; the element-chain order was not taken: " + chain_why;
      CHECK(st);
      h->h_coarse.assign(Ac->m, 0.0);
    }
  }
  *out = h.release();
  return AGGMG_OK;
}

static int coarse_solve(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs_dev, double* u_dev) {
  if (h->cr.valid) return cr_solve(ctx, h, rhs_dev, 0, u_dev, 0, 1);
  const int64_t n = h->coarse.n;
  HIPCHK(hipMemcpyAsync(h->h_coarse.data(), rhs_dev, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  auto t0 = std::chrono::steady_clock::now();
  banded_solve(h->coarse, h->h_coarse.data());
  HIPCHK(hipMemcpyAsync(u_dev, h->h_coarse.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  h->last_coarse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return AGGMG_OK;
}

// the coarsest solve of a column group (at most kMultiKB columns): one launch sequence on the device factorisation;
// column by column on the host banded LU, under AGGMG_CR_FUSE_TAIL=1 (its ticket counts the chunks of one solve) and for
// a group of one -- the same bits either way
static int coarse_solve_multi(aggmg_ctx* ctx, aggmg_hier* h, ColsIn B, ColsOut X, int kc) {
  if (h->cr.valid && kc > 1 && !cr_fuse_tail()) return cr_solve(ctx, h, B.p, B.ld, X.p, X.ld, kc);
  for (int j = 0; j < kc; ++j) CHECK(coarse_solve(ctx, h, B.at(j).p, X.at(j).p));
  return AGGMG_OK;
}

// ---- two levels in one launch (pair_kernels.hpp): the small agglomerated levels ------------------------------
#ifndef AGGMG_PAIR_NSA
#define AGGMG_PAIR_NSA 2   // measured (tools/exp_pair_tiles.sh): 2 / 1 slabs 0.356 ms per cycle of a rank's share, 3 / 2: 0.362, 4 / 2: 0.371
#endif
#ifndef AGGMG_PAIR_NSB
#define AGGMG_PAIR_NSB 1
#endif
constexpr int kPairM = 2, kPairNSA = AGGMG_PAIR_NSA, kPairNSB = AGGMG_PAIR_NSB;   // slabs per thread (tuning: tools/exp_pair_tiles.sh)
constexpr int kPairTEA = (kThreads / kPairM) * kPairNSA, kPairTEB = (kThreads / 2) * kPairNSB;

static bool pair_level_ok(const aggmg_hier* h, int k) {
  const Level& l = h->lv[k];
  return level_path(h, k) == LevelPath::FusedBtd && !l.S->gs && !l.S->btd->cmp && l.S->btd->m == kPairM && l.S->btd->bsym &&
         l.tb->mc == 2 && l.tb->rho > 0 && l.S->btd->ne == (int64_t)l.tb->rho * l.tb->nec;
}

// levels k and k + 1 (both smoothed, both below the finest: their iterates start at zero on the way down) in one launch
// of the descent (up = false) or of the ascent: the level kinds allow it and the launch has a tile for these ratios
// and sweeps (host_plan.hpp, the planners launch_pair_down / launch_pair_up run); otherwise one launch per level
static bool pair_ok(const aggmg_ctx* ctx, const aggmg_hier* h, int k, int nsweeps, bool up) {
  const int n = (int)h->lv.size();
  if (!ctx->pair_levels || k < 1 || k + 2 > n - 1 || nsweeps < 1 || nsweeps > 8) return false;
  const Level& a = h->lv[k];
  const Level& b = h->lv[k + 1];
  if (!pair_level_ok(h, k) || !pair_level_ok(h, k + 1) || b.S->btd->ne != a.tb->nec) return false;
  if (h->restriction == AGGMG_RESTRICT_PRECONDITIONED && (a.tb->ld || b.tb->ld)) return false;
  TileQuery q;
  q.launch = up ? kTilePairUp : kTilePairDown;
  q.te = kPairTEA;
  q.te_b = kPairTEB;
  q.halo = nsweeps;
  q.align = a.tb->rho;
  q.rho_bc = b.tb->rho;
  return launch_has_tile(q);
}

static PairArgs pair_args(const aggmg_hier* h, int k, int nsweeps) {
  const Level& a = h->lv[k];
  const Level& b = h->lv[k + 1];
  PairArgs p;
  std::memset(&p, 0, sizeof(p));
  auto lev = [](const BtdDev& d) { return PairLevel{d.bsym, d.dblk, d.sub, d.sup, d.ne}; };
  auto xf = [](const TransferBtd& t) { return PairXfer{t.lf, t.lf1, t.rho, t.nec}; };
  p.A = lev(*a.S->btd);
  p.B = lev(*b.S->btd);
  p.ab = xf(*a.tb);
  p.bc = xf(*b.tb);
  p.nsweeps = nsweeps;
  return p;
}

// The two levels' operator dictionaries in place of their full arrays (after pair_args), when BOTH levels have one:
// btd_pair_*_dict_kernel reads the same bits from them.  Otherwise both keep the full arrays.
static bool pair_dictionary(PairArgs& p, PairDict& d, const Level& a, const Level& b) {
  const PairDictDev *da = a.pdict.get(), *db = b.pdict.get();
  if (!da || !db) return false;
  auto lev = [](const PairDictDev& x, int64_t ne) { return PairLevel{x.bsym, x.dblk, x.sub, x.sup, ne}; };
  auto xf = [](const PairDictDev& x, const PairXfer& t) {
    return PairXfer{x.lf_unit ? nullptr : x.lf.get(), x.lf_unit ? x.lf.get() : nullptr, t.rho, t.nec};
  };
  p.A = lev(*da, p.A.ne);
  p.B = lev(*db, p.B.ne);
  p.ab = xf(*da, p.ab);
  p.bc = xf(*db, p.bc);
  d = PairDict{da->cls, db->cls, da->sback, db->sback};
  return true;
}

// The element-thread kernels (pair_elem_kernels.hpp, AGGMG_OPT_PAIR_ELEMENT_THREADS) in place of the row-thread dictionary
// ones: both levels have their packed records (at most kPairElemMaxClasses classes each) and the element-thread tile has
// a plan for these ratios and sweeps.  p holds the launch's vectors; the plan's tile replaces the row-thread one.
static bool pair_element_threads(const aggmg_ctx* ctx, PairArgs& p, PairElemDict& e, const Level& a, const Level& b, const PairTilePlan& plan) {
  const PairDictDev *da = a.pdict.get(), *db = b.pdict.get();
  if (!ctx->pair_elem_threads || !da || !db || !da->rec || !db->rec || plan.own <= 0) return false;
  e = PairElemDict{da->cls, db->cls, da->rec, db->rec, da->nclasses, db->nclasses};
  p.own = plan.own;
  p.te_a = plan.te_a;
  p.te_b = plan.te_b;
  p.hb = plan.hb;
  return true;
}

static int launch_pair_down(aggmg_ctx* ctx, aggmg_hier* h, int k, int nPre, double alpha) {
  Level& a = h->lv[k];
  Level& b = h->lv[k + 1];
  Level& c = h->lv[k + 2];
  PairArgs p = pair_args(h, k, nPre);
  const SweepWeights wa = a.damp_pre(alpha).launch(nPre), wb = b.damp_pre(alpha).launch(nPre);   // the two levels' factors
  const PairTilePlan plan = pair_down_plan(nPre, p.ab.rho, p.bc.rho, kPairTEA, kPairTEB);   // host_plan.hpp
  if (plan.own <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: paired tile too small");
  p.own = plan.own;
  p.te_b = plan.te_b;
  p.te_a = plan.te_a;
  p.rhs_a = a.rhs;
  p.u_a = a.u[0];
  p.rhs_b = b.rhs;
  p.u_b = b.u[0];
  p.rhs_c = c.rhs;
  int64_t ntiles = (p.B.ne + plan.own - 1) / plan.own;
  if (ntiles == 0) return AGGMG_OK;
  const size_t lds = ((size_t)2 * (kPairTEA + 2) * kPairM + (size_t)kPairTEB * 2) * sizeof(double);
  PairDict d;
  const bool dict = pair_dictionary(p, d, a, b);
  PairElemDict ed;
  const bool elem = dict && pair_element_threads(ctx, p, ed, a, b, pair_down_plan(nPre, p.ab.rho, p.bc.rho, kPairElemTEA, kPairElemTEB));
  ProfScope ps(ctx, AGGMG_KIND_FUSED_DOWN, k);
  if (elem) {
    ntiles = (p.B.ne + p.own - 1) / p.own;
    hipLaunchKernelGGL((btd_pair_down_elem_kernel<kPairElemThreads>), dim3((unsigned)ntiles), dim3(kPairElemThreads),
                       pair_elem_lds_bytes(ed.nca, ed.ncb), ctx->stream, p, wa, wb, ed);
    ++ctx->pair_elem_launches;
  } else if (dict)
    hipLaunchKernelGGL((btd_pair_down_dict_kernel<kPairM, kPairNSA, kPairNSB, kThreads>), dim3((unsigned)ntiles), dim3(kThreads),
                       lds, ctx->stream, p, wa, wb, d);
  else
    hipLaunchKernelGGL((btd_pair_down_kernel<kPairM, kPairNSA, kPairNSB, kThreads>), dim3((unsigned)ntiles), dim3(kThreads), lds,
                       ctx->stream, p, wa, wb);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// levels k + 1 then k; the result of level k goes to dst, the post-smoothed level k + 1 is consumed in LDS.
// part 0: every tile.  part 2 / 1 (element-partitioned runs, levels k + 1, k + 2 = the coarsest): the tiles that read none of
// the first gh_lo / last gh_hi elements of level k + 2 -- the neighbours' ghost blocks of the coarsest solution, still
// travelling -- and the remaining tiles at the two ends.
static int launch_pair_up(aggmg_ctx* ctx, aggmg_hier* h, int k, int nPost, double alpha, double* dst, int part = 0, int64_t gh_lo = 0,
                          int64_t gh_hi = 0) {
  const int n = (int)h->lv.size();
  Level& a = h->lv[k];
  Level& b = h->lv[k + 1];
  Level& c = h->lv[k + 2];
  PairArgs p = pair_args(h, k, nPost);
  const SweepWeights wa = a.damp_post(alpha).launch(nPost), wb = b.damp_post(alpha).launch(nPost);
  PairTilePlan plan = pair_up_plan(nPost, p.ab.rho, kPairTEA, kPairTEB);   // host_plan.hpp
  if (plan.own <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: paired tile too small");
  p.hb = plan.hb;
  p.own = plan.own;
  p.te_a = plan.te_a;
  p.te_b = plan.te_b;
  p.rhs_a = a.rhs;
  p.rhs_b_in = b.rhs;
  p.ua_in = a.u[0];
  p.ub_in = b.u[0];
  p.uc = (k + 2 == n - 1) ? c.u[0] : c.u[1];
  p.u_a = dst;
  p.ub_out = nullptr;   // nothing reads the post-smoothed iterate of level k + 1 but level k's prolongation
  int64_t ntiles = (p.A.ne + plan.own - 1) / plan.own;
  if (part != 0) {   // the tiles touching the ghosts: a prefix tA and a suffix tB
    pair_up_split(&plan, nPost, p.ab.rho, p.bc.rho, p.A.ne, p.bc.nec, gh_lo, gh_hi);
    if (part == 1) {
      p.tile_split = (int)plan.tA;
      p.tile_skip = plan.all - plan.tA - plan.tB;
      ntiles = plan.tA + plan.tB;
    } else {
      p.tile_skip = plan.tA;
      ntiles = plan.all - plan.tA - plan.tB;
    }
  }
  if (ntiles == 0) return AGGMG_OK;
  const size_t lds = ((size_t)2 * (kPairTEA + 2) * kPairM + (size_t)kPairTEB * 2) * sizeof(double);
  PairDict d;
  const bool dict = part == 0 && pair_dictionary(p, d, a, b);   // (the element-partitioned cycle keeps the full arrays)
  PairElemDict ed;
  const bool elem = dict && pair_element_threads(ctx, p, ed, a, b, pair_up_plan(nPost, p.ab.rho, kPairElemTEA, kPairElemTEB));
  ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, k);
  if (elem) {
    ntiles = (p.A.ne + p.own - 1) / p.own;
    hipLaunchKernelGGL((btd_pair_up_elem_kernel<kPairElemThreads>), dim3((unsigned)ntiles), dim3(kPairElemThreads),
                       pair_elem_lds_bytes(ed.nca, ed.ncb), ctx->stream, p, wa, wb, ed);
    ++ctx->pair_elem_launches;
  } else if (dict)
    hipLaunchKernelGGL((btd_pair_up_dict_kernel<kPairM, kPairNSA, kPairNSB, kThreads>), dim3((unsigned)ntiles), dim3(kThreads),
                       lds, ctx->stream, p, wa, wb, d);
  else
    hipLaunchKernelGGL((btd_pair_up_kernel<kPairM, kPairNSA, kPairNSB, kThreads>), dim3((unsigned)ntiles), dim3(kThreads), lds,
                       ctx->stream, p, wa, wb);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

extern "C" int aggmg_hier_level_paired(aggmg_ctx* ctx, const aggmg_hier* h, int level, int nsweeps, int* paired) {
  if (!ctx || !h || !paired) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_paired: NULL argument");
  *paired = pair_ok(ctx, h, level, nsweeps, false) ? 1 : 0;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_level_paired_up(aggmg_ctx* ctx, const aggmg_hier* h, int level, int nsweeps, int* paired) {
  if (!ctx || !h || !paired) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_paired_up: NULL argument");
  *paired = pair_ok(ctx, h, level, nsweeps, true) ? 1 : 0;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_level_sym_residual(aggmg_ctx* ctx, const aggmg_hier* h, int level, int* on) {
  if (!ctx || !h || !on) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_sym_residual: NULL argument");
  if (level < 0 || level >= (int)h->lv.size()) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_sym_residual: level out of range");
  const Level& l = h->lv[level];
  *on = (l.S && l.S->btd && l.S->btd->dup) ? 1 : 0;
  return AGGMG_OK;
}

extern "C" int aggmg_element_thread_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_element_thread_launches: NULL argument");
  *count = ctx->elem_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_pair_element_thread_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_pair_element_thread_launches: NULL argument");
  *count = ctx->pair_elem_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_coarse_dictionary_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_coarse_dictionary_launches: NULL argument");
  *count = ctx->coarse_dict_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_coarse_dictionary_cap(aggmg_ctx* ctx, int* cap, int* max_cap) {
  if (!ctx || !cap) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_coarse_dictionary_cap: NULL argument");
  *cap = ctx->coarse_dict_cap;
  if (max_cap) *max_cap = kCrDictMaxClasses;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_coarse_dictionary(aggmg_ctx* ctx, const aggmg_hier* h, int capacity, int* nstages, int* taken,
                                            int* first_level, int* nlevels, int* even_classes, int* odd_classes) {
  if (!ctx || !h || !nstages || !taken || !first_level || !nlevels || !even_classes || !odd_classes || capacity < kCrMaxLevels)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_coarse_dictionary: NULL argument or capacity below " + std::to_string(kCrMaxLevels));
  const CrDev& cr = h->cr;
  *nstages = cr.valid ? (int)cr.st.size() : 0;
  for (int i = 0; i < capacity; ++i) taken[i] = first_level[i] = nlevels[i] = 0, even_classes[i] = odd_classes[i] = -1;
  if (!cr.valid) return AGGMG_OK;
  for (size_t s = 0; s < cr.st.size(); ++s) {
    taken[s] = cr.st[s].dict.take ? 1 : 0;
    first_level[s] = cr.st[s].l0;
    nlevels[s] = cr.st[s].q;
  }
  for (size_t l = 0; l < cr.dict_even.size() && l < (size_t)capacity; ++l) {
    even_classes[l] = cr.dict_even[l];
    odd_classes[l] = cr.dict_odd[l];
  }
  return AGGMG_OK;
}

extern "C" int aggmg_element_record_lds_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_element_record_lds_launches: NULL argument");
  *count = ctx->elem_rec_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_element_record_lds_cap(aggmg_ctx* ctx, int* cap, int* max_cap) {
  if (!ctx || !cap) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_element_record_lds_cap: NULL argument");
  *cap = ctx->elem_rec_cap;
  if (max_cap) *max_cap = kElemRecMaxClasses;
  return AGGMG_OK;
}

extern "C" int aggmg_element_record_pack(int nclasses, const double* bsym, const double* qrow, const double* qmir, const double* dup,
                                         const uint32_t* corr, const double* lf, int lf_unit, double* rec, int* words) {
  if (words) *words = kElemRecWords;
  if (nclasses < 0 || (nclasses > 0 && (!bsym || !qrow || !qmir || !lf || !rec || !dup != !corr))) return AGGMG_ERR_ARGUMENT;
  elem_record_pack(nclasses, bsym, qrow, qmir, dup, corr, lf, lf_unit != 0, rec);
  return AGGMG_OK;
}

extern "C" int aggmg_replay_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_replay_launches: NULL argument");
  *count = ctx->replay_launches;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_level_dictionary(aggmg_ctx* ctx, const aggmg_hier* h, int level, int* nclasses) {
  if (!ctx || !h || !nclasses) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_dictionary: NULL argument");
  if (level < 0 || level >= (int)h->lv.size()) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_dictionary: level out of range");
  const Level& l = h->lv[level];
  *nclasses = l.dict ? l.dict->nclasses : (l.cdict ? l.cdict->nclasses : (l.pdict ? l.pdict->nclasses : 0));
  return AGGMG_OK;
}

// ---- sweep-weight schedules (EXTENSION: the reference damps every sweep of every level by the same alpha,
// src/solvers.jl:19-50) ------------------------------------------------------------------------------------------
extern "C" int aggmg_hier_set_sweep_weights(aggmg_ctx* ctx, aggmg_hier* h, int level, const double* pre, int npre,
                                            const double* post, int npost) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_set_sweep_weights: NULL argument");
  if (level < 0 || level >= (int)h->lv.size() - 1)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_set_sweep_weights: level out of range (the coarsest level is solved, not smoothed)");
  if (npre < 0 || npost < 0 || npre > AGGMG_MAX_SWEEP_WEIGHTS || npost > AGGMG_MAX_SWEEP_WEIGHTS)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_set_sweep_weights: between 0 and AGGMG_MAX_SWEEP_WEIGHTS weights per half");
  if ((npre > 0 && !pre) || (npost > 0 && !post)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_set_sweep_weights: NULL argument");
  for (int i = 0; i < npre; ++i)
    if (!std::isfinite(pre[i])) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_set_sweep_weights: weight is not finite");
  for (int i = 0; i < npost; ++i)
    if (!std::isfinite(post[i])) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_set_sweep_weights: weight is not finite");
  Level& l = h->lv[level];
  l.scheduled = npre + npost > 0;
  l.w_pre.assign(pre, pre + npre);
  l.w_post.assign(post, post + npost);
  l.w_mid = l.w_post;
  l.w_mid.insert(l.w_mid.end(), l.w_pre.begin(), l.w_pre.end());
  l.w_replay = l.w_pre;
  l.w_replay.insert(l.w_replay.end(), l.w_post.begin(), l.w_post.end());
  return AGGMG_OK;
}

extern "C" int aggmg_hier_get_sweep_weights(aggmg_ctx* ctx, const aggmg_hier* h, int level, double* pre, int* npre,
                                            double* post, int* npost) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !pre || !npre || !post || !npost) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_get_sweep_weights: NULL argument");
  if (level < 0 || level >= (int)h->lv.size() - 1)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_get_sweep_weights: level out of range");
  const Level& l = h->lv[level];
  *npre = (int)l.w_pre.size();
  *npost = (int)l.w_post.size();
  std::copy(l.w_pre.begin(), l.w_pre.end(), pre);
  std::copy(l.w_post.begin(), l.w_post.end(), post);
  return AGGMG_OK;
}

// A cycle's sweep counts against the schedules of levels k_first .. n - 2 (nPre / nPost < 0: that half is not run by the
// caller): nothing is truncated or padded silently.
static int schedule_check(aggmg_ctx* ctx, const aggmg_hier* h, int nPre, int nPost, int k_first = 0) {
  for (int k = k_first; k < (int)h->lv.size() - 1; ++k) {
    const Level& l = h->lv[k];
    if (!l.scheduled) continue;
    if ((nPre >= 0 && nPre != (int)l.w_pre.size()) || (nPost >= 0 && nPost != (int)l.w_post.size()))
      return fail(ctx, AGGMG_ERR_ARGUMENT, "level " + std::to_string(k) + " has a sweep-weight schedule of " +
                  std::to_string(l.w_pre.size()) + " pre- and " + std::to_string(l.w_post.size()) +
                  " post-smoothing weights; the cycle asks for " + std::to_string(nPre) + " / " + std::to_string(nPost) + " sweeps");
  }
  return AGGMG_OK;
}

// ---- half-cycles of one level, family by family: the chain path's are cgt_down / cgt_up / cgt_mid (cgt.hip), these take
// the same arguments.  Down (src/solvers.jl:28-37): nPre sweeps from uin (null: zeros) into l.u[0], the restricted residual
// into the next level's rhs.  Up (:41-47): the next level's result prolonged onto l.u[0], nPost sweeps into dst. ---------
static const double* coarse_result(const aggmg_hier* h, int k) {   // what level k prolongs from
  return (k + 2 == (int)h->lv.size()) ? h->lv[k + 1].u[0] : h->lv[k + 1].u[1];
}
// the generic launches around a level's sweeps: rc = L' (rhs - A u[0]) through l.tmp (resid_done: it holds the residual
// already), and u[0] += L uc
static int generic_restrict_residual(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* rhs, bool resid_done) {
  Level& l = h->lv[k];
  if (!resid_done) {
    ProfScope ps(ctx, AGGMG_KIND_RESIDUAL, k);
    CHECK(op_ensure_csr(ctx, l.A));
    CHECK(launch_csr<kResidual>(ctx, l.A->csr, l.u[0], rhs, nullptr, 0.0, l.tmp));
  }
  ProfScope ps(ctx, AGGMG_KIND_RESTRICT, k);
  CHECK(op_ensure_csc_blocks(ctx, l.L));
  return launch_csr<kSpmvSet>(ctx, l.L->csc, l.tmp, nullptr, nullptr, 0.0, h->lv[k + 1].rhs);
}
static int generic_prolong_add(aggmg_ctx* ctx, aggmg_hier* h, int k) {
  Level& l = h->lv[k];
  ProfScope ps(ctx, AGGMG_KIND_PROLONG, k);
  CHECK(op_ensure_csr(ctx, l.L));
  return launch_csr<kSpmvAdd>(ctx, l.L->csr, coarse_result(h, k), nullptr, nullptr, 0.0, l.u[0]);
}
static int no_split_ascent(aggmg_ctx* ctx) {
  return fail(ctx, AGGMG_ERR_UNSUPPORTED, "split ascent needs the fused block-tridiagonal fine level (or a multiplicative patch level "
                                          "with a one-ratio transfer and a single launch of post sweeps)");
}

// Block-tridiagonal levels (LevelPath::FusedBtd, BtdTransfer).  One fused launch where the level has the structured
// transfer and the launch a tile; otherwise chunked sweeps and the generic launches around them.
// store = false (a replayed cycle, replay_ok said so): the fused launch keeps the pre-smoothed iterate to itself.
static int btd_down(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* uin, const double* rhs, int nPre, double alpha,
                    bool store = true) {
  Level& l = h->lv[k];
  const BtdDev& B = *l.S->btd;
  const Damping damp = l.damp_pre(alpha);   // the level's schedule, or alpha for every sweep
  const int gs = l.S->gs ? 1 : 0;           // Gauss-Seidel: even elements, then odd ones
  if (l.tb && btd_launch_ok(*l.S, nPre, 1, l.tb.get())) {
    FusedLaunch a = fused_sweeps(B, uin, rhs, store ? l.u[0].get() : nullptr, damp, nPre, gs);
    fused_descent(a, h, l, h->lv[k + 1].rhs);
    fused_dictionary(a, l);
    ProfScope ps(ctx, AGGMG_KIND_FUSED_DOWN, k);
    return launch_btd(ctx, B, a, nPre + 1);   // (+ 1: the residual rows)
  }
  CHECK(btd_smooth(ctx, B, uin, rhs, damp, nPre, l.u[0], k, l.N, gs));
  return generic_restrict_residual(ctx, h, k, rhs, false);
}
// src: the pre-smoothed iterate (default: l.u[0]).  chk: the launch forms a checkpoint's sums -- residual rows of the
// FINAL iterate, one more element of halo -- and reports its tile count there.  sel (level 0): the tiles to run; the
// dictionary serves no selection (the partitioned cycle keeps the full arrays) and no checkpoint (fused_dictionary's own test).
static int btd_up(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* rhs, int nPost, double alpha, double* dst,
                  const double* src = nullptr, CgtChk* chk = nullptr, const TileSel& sel = TileSel()) {
  Level& l = h->lv[k];
  const BtdDev& B = *l.S->btd;
  const Damping damp = l.damp_post(alpha);
  const int gs = l.S->gs ? 2 : 0;   // Gauss-Seidel in the reverse colour order: the cycle stays symmetric
  if (l.tb && btd_launch_ok(*l.S, nPost, 0, nullptr)) {
    FusedLaunch a = fused_sweeps(B, src ? src : l.u[0], rhs, dst, damp, nPost, gs);
    fused_ascent(a, l, coarse_result(h, k));
    if (chk) fused_chk(a, *chk);
    if (sel.mode == 0) fused_dictionary(a, l);
    ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, k);
    return launch_btd(ctx, B, a, nPost + (chk ? 1 : 0), sel, chk);
  }
  if (sel.mode == 1 || sel.mode == 2) return no_split_ascent(ctx);
  if (src || chk) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: unfused ascent from another source or with a checkpoint");
  CHECK(generic_prolong_add(ctx, h, k));
  return btd_smooth(ctx, B, l.u[0], rhs, damp, nPost, dst, k, l.N, gs);
}
// Between two cycles, level 0 (fine_mid_ok said that the launch exists): post-smoothing of one cycle, pre-smoothing and
// restriction of the next in ONE launch, cur -> alt; a checkpoint falls between the two runs of sweeps.
static int btd_mid(aggmg_ctx* ctx, aggmg_hier* h, const double* cur, double* alt, const double* b, int nsweeps, double alpha,
                   CgtChk* chk = nullptr) {
  Level& l = h->lv[0];
  FusedLaunch a = fused_sweeps(*l.S->btd, cur, b, alt, l.damp_mid(alpha), nsweeps);
  fused_ascent(a, l, coarse_result(h, 0));
  fused_descent(a, h, l, h->lv[1].rhs);
  if (chk) fused_chk(a, *chk);
  fused_dictionary(a, l);
  ProfScope ps(ctx, AGGMG_KIND_FUSED_MID, 0);
  return launch_btd(ctx, *l.S->btd, a, nsweeps + 1, TileSel(), chk);
}

// ---- the replayed cycle (AGGMG_OPT_REPLAY_PRESMOOTH; elem_kernels.hpp, btd_elem_replay_up_kernel): level 0's descent
// stores no iterate and its ascent rebuilds it from the cycle's first iterate -- a vector less written and the same
// vector count read, the same bits.  Only aggmg_vcycle_dev asks; every other caller of the half-cycles keeps the stored
// iterate (the loops over cycles, the split entry points, the partitioned and K-column cycles).
// The arguments of level 0's two launches as btd_down / btd_up would build them: x0 stands where the ascent reads l.u[0].
static FusedLaunch replay_down_args(aggmg_hier* h, const double* x0, const double* b, int nPre, double alpha) {
  Level& l = h->lv[0];
  FusedLaunch a = fused_sweeps(*l.S->btd, x0, b, nullptr, l.damp_pre(alpha), nPre);
  fused_descent(a, h, l, h->lv[1].rhs);
  fused_dictionary(a, l);
  return a;
}
static FusedLaunch replay_up_args(aggmg_hier* h, const double* x0, const double* b, int nPre, int nPost, double alpha, double* dst) {
  Level& l = h->lv[0];
  FusedLaunch a = fused_sweeps(*l.S->btd, x0, b, dst, l.damp_replay(alpha), nPre + nPost);
  fused_ascent(a, l, coarse_result(h, 0));
  fused_dictionary(a, l);
  return a;
}
// Does this cycle replay?  Level 0 is a fused block-tridiagonal level (never part of a two-level launch: pair_ok starts
// at level 1) whose descent and ascent are both single launches of the element-thread kernel, there are sweeps on both
// sides and a weight for each, the replaying launch has a tile, and x_out's range is disjoint from x0's -- the ascent
// reads x0's halos while other workgroups store x_out; a partial overlap, harmless on the storing path, would race here.
// Not on a hierarchy whose half-cycle entry points have been used (aggmg_hier::halves_used): an ascent on its own may
// follow a whole cycle and read the iterate that cycle stored.
static bool replay_ok(const aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre, int nPost, double alpha,
                      const double* x_out) {
  if (!ctx->replay_presmooth || !ctx->elem_threads || h->halves_used || h->lv.size() < 2 || level_path(h, 0) != LevelPath::FusedBtd) return false;
  if (nPre < 1 || nPost < 1 || nPre + nPost > kSweepWeights) return false;
  const Level& l = h->lv[0];
  const BtdDev& B = *l.S->btd;
  if (B.m != 4 || !B.cmp || l.S->gs || !l.tb || !btd_launch_ok(*l.S, nPre, 1, l.tb.get()) || !btd_launch_ok(*l.S, nPost, 0, nullptr)) return false;
  const FusedLaunch dn = replay_down_args(h, x0, b, nPre, alpha), up = replay_up_args(h, x0, b, nPre, nPost, alpha, nullptr);
  if (!elem_thread_args(ctx, dn, false, 0) || !elem_thread_args(ctx, up, false, 0)) return false;
  if (fused_tile_plan(kElemThreads, nPre + 1, dn.rho_out, false, dn.agg_shift).owned <= 0 ||
      fused_tile_plan(kElemThreads, nPost, 1, false, up.agg_shift).owned <= 0 ||
      fused_tile_plan(kElemThreads, nPre + nPost, 1, false, up.agg_shift).owned <= 0)
    return false;
  if (x0) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(x0), q = reinterpret_cast<uintptr_t>(x_out), len = (uintptr_t)l.N * sizeof(double);
    if (p < q + len && q < p + len) return false;
  }
  return true;
}
static int btd_replay_up(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre, int nPost, double alpha,
                         double* dst) {
  FusedLaunch a = replay_up_args(h, x0, b, nPre, nPost, alpha, dst);
  const FusedTilePlan plan = fused_tile_plan(kElemThreads, nPre + nPost, 1, false, a.agg_shift);
  if (plan.owned <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: replayed ascent without a tile");
  a.agg_shift = plan.agg_shift;
  a.owned = plan.owned;
  a.halo_left = plan.halo_left;
  const TileSubset sub = fused_tile_subset(a.lv.ne, plan.owned, 0, 0, 0);
  a.tile_split = sub.split;
  a.tile_skip = sub.skip;
  if (sub.ntiles == 0) return AGGMG_OK;
  ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, 0);
  const bool rec = elem_record_args(ctx, a);
  if (rec)
    hipLaunchKernelGGL(btd_elem_rec_replay_up_kernel<4>, dim3((unsigned)sub.ntiles), dim3(kElemThreads),
                       elem_rec_lds_bytes<4>(a.rec.nclasses), ctx->stream, static_cast<const FusedArgs&>(a), a.wts, nPre, a.rec);
  else
    hipLaunchKernelGGL(btd_elem_replay_up_kernel<4>, dim3((unsigned)sub.ntiles), dim3(kElemThreads), elem_lds_bytes<4>(), ctx->stream,
                       static_cast<const FusedArgs&>(a), a.wts, nPre);
  HIPCHK(hipGetLastError());
  ++ctx->elem_launches;
  if (rec) ++ctx->elem_rec_launches;
  ++ctx->replay_launches;
  return AGGMG_OK;
}

// Element-patch Schwarz levels (LevelPath::Patch): chunked patch sweeps, and around them the zero-sweep fused launch of the
// element-block form -- residual + restriction (the launch of aggmg_residual_dev with a restriction behind it), or the
// prolongation -- where the level has the structured transfer and that launch a tile; otherwise the generic launches.
static bool patch_transfer_ok(const Level& l, int residual, const TransferBtd* tout) {
  if (!l.tb) return false;
  const BtdDev& B = *l.S->patch->btd;
  TileQuery q;
  q.launch = kTileFused;
  q.te = btd_tile_elems(B);
  q.halo = residual;
  if (tout) {
    q.var_agg = tout->rho == 0;
    q.align = tout->rho ? tout->rho : 1;
    q.agg_shift = xfer_agg_shift(*tout);
  }
  return launch_has_tile(q);
}
static int patch_down(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* uin, const double* rhs, int nPre, double alpha) {
  Level& l = h->lv[k];
  const PatchDev& P = *l.S->patch;
  CHECK(patch_smooth(ctx, P, uin, rhs, l.damp_pre(alpha), nPre, l.u[0], k));
  if (patch_transfer_ok(l, 1, l.tb.get())) {
    FusedLaunch a = fused_sweeps(*P.btd, l.u[0], rhs, nullptr, 0.0, 0);
    fused_descent(a, h, l, h->lv[k + 1].rhs);
    a.ld_out = nullptr;   // the explicit residual's restriction: (L'D) belongs to the block-Jacobi stencil form
    a.lf_out = l.tb->lf;
    fused_dictionary(a, l);
    ProfScope ps(ctx, AGGMG_KIND_FUSED_DOWN, k);
    return launch_btd(ctx, *P.btd, a, 1);
  }
  return generic_restrict_residual(ctx, h, k, rhs, false);
}
static int patch_up(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* rhs, int nPost, double alpha, double* dst) {
  Level& l = h->lv[k];
  const PatchDev& P = *l.S->patch;
  // (post-smoothing: the multiplicative sweeps run their colours in reverse order, patch_down's in forward order)
  // the prolonged iterate goes through l.tmp: the fused launch wants another vector than its input, the sweeps too
  if (patch_transfer_ok(l, 0, nullptr)) {
    FusedLaunch a = fused_sweeps(*P.btd, l.u[0], rhs, l.tmp, 0.0, 0);
    fused_ascent(a, l, coarse_result(h, k));
    fused_dictionary(a, l);
    {
      ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, k);
      CHECK(launch_btd(ctx, *P.btd, a, 0));
    }
    return patch_smooth(ctx, P, l.tmp, rhs, l.damp_post(alpha), nPost, dst, k, true);
  }
  CHECK(generic_prolong_add(ctx, h, k));
  return patch_smooth(ctx, P, l.u[0], rhs, l.damp_post(alpha), nPost, dst, k, true);
}

// The fine-level ascent of a multiplicative patch level in ONE launch per tile selection (element-partitioned runs: the
// tiles at the two ends on one stream, the ones in between on another -- each writes only its own tiles of dst and no
// scratch vector is shared).  Offered where patch_up would prolong with the zero-sweep fused launch -- whose bits the
// launch repeats -- through a structured transfer of one ratio, and the post sweeps are a single launch with a tile.
static bool patch_split_ok(const aggmg_hier* h, int nPost) {
  if (h->lv.size() < 2 || level_path(h, 0) != LevelPath::Patch) return false;
  const Level& l = h->lv[0];
  const PatchDev& P = *l.S->patch;
  if (!P.multiplicative || !l.tb || l.tb->rho <= 0 || P.ne != (int64_t)l.tb->rho * l.tb->nec) return false;
  if (!patch_transfer_ok(l, 0, nullptr)) return false;
  if (nPost < 1 || nPost > patch_gs_max_sweeps(P.m)) return false;
  TileQuery q;
  q.launch = kTilePatchGs;
  q.te = patch_tile_elems(P.m);
  q.halo = nPost;
  return launch_has_tile(q);
}
static int patch_up_split(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs, int nPost, double alpha, double* dst, const TileSel& sel) {
  Level& l = h->lv[0];
  const PatchDev& P = *l.S->patch;
  PatchGsUpArgs u{};
  u.g.p = patch_args(P, l.u[0], rhs, dst, nPost);
  u.g.reverse = 1;   // post-smoothing: the colours in reverse order
  u.uc = coarse_result(h, 0);
  u.lf = l.tb->lf;
  u.lf1 = l.tb->lf1;
  u.mc = l.tb->mc;
  u.rho = l.tb->rho;
  ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, 0);
  return launch_patch_gs_up(ctx, P, u, l.damp_post(alpha).from(0).launch(nPost), sel);
}

// Generic levels: generic_sweeps between the generic launches.  The descent sweeps in place in l.u[0] (point Jacobi:
// with l.u[1] as its second vector, the banded form's residual straight into l.tmp); the ascent keeps its intermediate
// sweeps in l.u[0] and writes the last one to dst (point Jacobi: with whichever of l.u[1] / l.tmp is not dst).
static int generic_down(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* uin, const double* rhs, int nPre, double alpha) {
  Level& l = h->lv[k];
  bool resid_done = false;
  CHECK(generic_sweeps(ctx, l.A, l.S, uin, rhs, l.damp_pre(alpha), nPre, l.u[0], l.u[0], l.u[1], k, l.tmp, &resid_done));
  return generic_restrict_residual(ctx, h, k, rhs, resid_done);
}
static int generic_up(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* rhs, int nPost, double alpha, double* dst) {
  Level& l = h->lv[k];
  CHECK(generic_prolong_add(ctx, h, k));
  double* other = (dst == l.u[1]) ? l.tmp : l.u[1];
  return generic_sweeps(ctx, l.A, l.S, l.u[0], rhs, l.damp_post(alpha), nPost, dst, l.u[0], other, k);
}

// ---- descend: leaves u[k] in lv[k].u[0] and rhs[n] in lv[n-1].rhs -------------------------------
// (a level that pairs with the next is a FusedBtd level: asking for the pair first loses no chain level)
static int vcycle_down(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre, double alpha,
                       int k_first = 0) {
  const int n = (int)h->lv.size();
  CHECK(schedule_check(ctx, h, nPre, -1, k_first));
  if (k_first == 0) h->fine_iterate_absent = false;   // (this descent stores level 0's pre-smoothed iterate)
  for (int k = k_first; k < n - 1; ++k) {
    const double* rhs = k == 0 ? b : h->lv[k].rhs;
    const double* uin = k == 0 ? x0 : nullptr;  // u[k] = zeros for k > 1 (:29-31)
    if (pair_ok(ctx, h, k, nPre, false)) {   // this level and the next in one launch
      CHECK(launch_pair_down(ctx, h, k, nPre, alpha));
      ++k;
      continue;
    }
    switch (level_path(h, k)) {
      case LevelPath::FusedChain: CHECK(cgt_down(ctx, h, k, uin, rhs, nPre, alpha)); break;
      case LevelPath::FusedBtd:
      case LevelPath::BtdTransfer: CHECK(btd_down(ctx, h, k, uin, rhs, nPre, alpha)); break;
      case LevelPath::Patch: CHECK(patch_down(ctx, h, k, uin, rhs, nPre, alpha)); break;
      case LevelPath::Generic: CHECK(generic_down(ctx, h, k, uin, rhs, nPre, alpha)); break;
      case LevelPath::Coarsest: break;
    }
  }
  return AGGMG_OK;
}

// ---- ascend: expects the coarsest solution in lv[n-1].u[0] ---------------------------------------
// sel (fine level only): which tiles of the level-0 launch to run; with a selection the coarser
// levels are skipped (the caller ran them with k_last = 1)
// csplit (element-partitioned runs): the first launch of the ascent -- it has to be a two-level launch next to the coarsest
// level -- in two parts around the exchange of the coarsest solution's ghost blocks: mode 2 runs ONLY its tiles that read
// no ghost block (nothing else), mode 1 its remaining tiles and then the rest of the ascent, two-level launches all of it
// (no further pairs are split)
struct CoarseSplit {
  int mode = 0;
  int64_t gh_lo = 0, gh_hi = 0;
};
static int vcycle_up(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPost, double alpha, double* x_out,
                     int k_last = 0, const TileSel& sel = TileSel(), const CoarseSplit& cs = CoarseSplit()) {
  const int n = (int)h->lv.size();
  CHECK(schedule_check(ctx, h, -1, nPost, k_last));
  int part = cs.mode;   // of the next two-level launch: the first one is the split one
  for (int k = (sel.mode != 0 ? 0 : n - 2); k >= k_last; --k) {
    const double* rhs = k == 0 ? b : h->lv[k].rhs;
    double* dst = k == 0 ? x_out : h->lv[k].u[1];
    if (sel.mode == 0 && k - 1 >= std::max(k_last, 1) && pair_ok(ctx, h, k - 1, nPost, true)) {   // this level and the finer one in one launch
      CHECK(launch_pair_up(ctx, h, k - 1, nPost, alpha, h->lv[k - 1].u[1], part, cs.gh_lo, cs.gh_hi));
      if (part == 2) return AGGMG_OK;
      part = 0;
      --k;
      continue;
    }
    if (cs.mode != 0)
      return fail(ctx, AGGMG_ERR_UNSUPPORTED, part != 0 ? "split coarse ascent needs a two-level launch next to the coarsest level"
                                                        : "split coarse ascent: unpaired level above the coarse pair");
    const LevelPath path = level_path(h, k);
    const bool btd = path == LevelPath::FusedBtd || path == LevelPath::BtdTransfer;
    if (!btd && (sel.mode == 1 || sel.mode == 2)) {
      // a multiplicative patch level: prolongation and sweeps of the selected tiles in one launch
      if (k == 0 && path == LevelPath::Patch && patch_split_ok(h, nPost)) return patch_up_split(ctx, h, rhs, nPost, alpha, dst, sel);
      return no_split_ascent(ctx);
    }
    switch (path) {
      case LevelPath::FusedChain: CHECK(cgt_up(ctx, h, k, rhs, nPost, alpha, dst)); break;
      case LevelPath::FusedBtd:   // (refuses a selection itself where the fused launch has no tile)
      case LevelPath::BtdTransfer: CHECK(btd_up(ctx, h, k, rhs, nPost, alpha, dst, nullptr, nullptr, sel)); break;
      case LevelPath::Patch: CHECK(patch_up(ctx, h, k, rhs, nPost, alpha, dst)); break;
      case LevelPath::Generic: CHECK(generic_up(ctx, h, k, rhs, nPost, alpha, dst)); break;
      case LevelPath::Coarsest: break;
    }
  }
  return AGGMG_OK;
}

static int vcycle_args(aggmg_ctx* ctx, aggmg_hier* h, const void* a, const void* b2, int n1, int n2) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !a || !b2) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle: NULL argument");
  if (n1 < 0 || n2 < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle: negative sweep count");
  return AGGMG_OK;
}

extern "C" int aggmg_vcycle_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre,
                                int nPost, double alpha, double* x_out) {
  // x0 == NULL: zero initial guess (ldiv!, src/solvers.jl:63-92) -- the fine level starts from zeros like every other
  // level does (:29-31) and reads no iterate at all
  CHECK(vcycle_args(ctx, h, x0 ? x0 : b, b, nPre, nPost));
  if (!x_out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle: NULL argument");
  if (x_out == x0 || x_out == b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle: x_out must not alias x0 or b");
  if (h->coarse_mode == AGGMG_COARSE_EXTERNAL)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle: hierarchy was created with AGGMG_COARSE_EXTERNAL; use "
                                         "aggmg_vcycle_down_dev / aggmg_vcycle_up_dev");
  const int n = (int)h->lv.size();
  CHECK(schedule_check(ctx, h, nPre, nPost));   // (both halves before anything is enqueued)
  h->last_coarse_ms = 0.0;
  // decided once, before anything is enqueued: level 0's descent stores no iterate and its ascent replays the pre-smoothing
  // from x0 (replay_ok).  Level 0's u[0] then holds nothing defined after this call.  Its readers follow a descent of
  // their own call sequence (the ascents of a cycle, the launch between two cycles) -- all but an ascent called on its own
  // after a whole cycle (aggmg_vcycle_up_dev / _up_split_dev), which is refused while fine_iterate_absent says so.
  const bool replay = replay_ok(ctx, h, x0, b, nPre, nPost, alpha, x_out);
  if (replay) {
    h->fine_iterate_absent = true;
    CHECK(btd_down(ctx, h, 0, x0, b, nPre, alpha, false));
    CHECK(vcycle_down(ctx, h, nullptr, b, nPre, alpha, 1));
  } else {
    CHECK(vcycle_down(ctx, h, x0, b, nPre, alpha));
  }
  {  // coarsest solve (src/solvers.jl:39)
    Level& c = h->lv[n - 1];
    const double* rhs = n == 1 ? b : c.rhs;
    double* dst = n == 1 ? x_out : c.u[0];
    CHECK(coarse_solve(ctx, h, rhs, dst));
  }
  if (!replay) return vcycle_up(ctx, h, b, nPost, alpha, x_out);
  CHECK(vcycle_up(ctx, h, b, nPost, alpha, nullptr, 1));
  return btd_replay_up(ctx, h, x0, b, nPre, nPost, alpha, x_out);
}

// ---- K right-hand sides in one pass over the operators (EXTENSION: the reference's multigrid_v_cycle / ldiv! take
// vectors, src/solvers.jl:19,63,84) ------------------------------------------------------------------------------
// The columns go in groups of at most kMultiKB; every non-coarsest level runs the two halves of its kernel family per
// group (block-tridiagonal levels always, patch and chain levels by option; no two-level launches
// here), and the coarsest solve one launch sequence per group (cr_solve).  A hierarchy with a level no family accepts runs
// the single-column cycle on every column instead (a one-level hierarchy, whose cycle is the coarsest solve alone, still
// in groups): the same bits either way (multi_kernels.hpp), aggmg_hier_multi_info says which.
#ifndef AGGMG_MULTI_KB
#define AGGMG_MULTI_KB 8
#endif
#ifndef AGGMG_MULTI_NT
#define AGGMG_MULTI_NT 256
#endif
constexpr int kMultiKB = AGGMG_MULTI_KB, kMultiNT = AGGMG_MULTI_NT;
static_assert(is_col_group(kMultiKB), "column groups of 1, 2, 4 or 8");

// A patch level in column groups -- a multiplicative one under AGGMG_OPT_PATCH_MULTI (patch_gs_multi_kernel), a hybrid /
// additive one under AGGMG_OPT_PATCH_SCHWARZ_MULTI (patch_sweep_multi_kernel): the K-column sweeps and, around them, the
// zero-sweep launches of the K-column transfer kernel on the smoother's element-block form -- where the single-column cycle
// runs its zero-sweep fused launches (patch_transfer_ok), whose bits those repeat.
static bool multi_patch_level_ok(const aggmg_ctx* ctx, const aggmg_hier* h, int k, int nPre, int nPost) {
  const Level& l = h->lv[k];
  const PatchDev& P = *l.S->patch;
  if (!(P.multiplicative ? ctx->patch_multi && patch_multi_form_ok(P) : ctx->patch_schwarz_multi && patch_schwarz_multi_form_ok(P)) || !l.tb)
    return false;
  const TransferBtd& t = *l.tb;
  if (t.mc != 2 || t.rho <= 0 || P.ne != (int64_t)t.rho * t.nec) return false;
  if (!patch_transfer_ok(l, 1, &t) || !patch_transfer_ok(l, 0, nullptr)) return false;
  TileQuery down, up;
  down.launch = up.launch = kTileMulti;
  down.te = up.te = kMultiNT / P.m;
  down.halo = 1;
  down.align = t.rho;
  up.halo = 0;
  if (!launch_has_tile(down) || !launch_has_tile(up)) return false;
  // every chunk of the two runs of sweeps under the K-column plan of the smoother's kind
  const int smax = patch_multi_max_sweeps(P);
  for (int n : {nPre, nPost})
    for (int c = 0; c < patch_chunks(n, smax); ++c) {
      TileQuery q;
      q.launch = P.multiplicative ? kTilePatchGsMulti : kTilePatchSchwarzMulti;
      q.te = P.multiplicative ? patch_gs_multi_tile_elems(P.m) : patch_schwarz_multi_tile_elems(P.m);
      q.halo = patch_chunk_sweeps(n, smax, c);
      if (!launch_has_tile(q)) return false;
    }
  return (nPre == 0 && nPost == 0) || smax >= 1;
}

// A fused chain level in column groups (AGGMG_OPT_CHAIN_MULTI): point-Jacobi sweeps on a block size of chain_dict_form, each half
// one launch of cgt_multi_kernel with a tile (the planner its launcher runs; a group of kMultiKB columns: the tile does not
// depend on the group).
static bool multi_chain_level_ok(const aggmg_ctx* ctx, const aggmg_hier* h, int k, int nPre, int nPost) {
  const Level& l = h->lv[k];
  const CgtDev& g = *l.S->cgt;
  if (!ctx->chain_multi || g.sw != 0 || !chain_dict_form(g.m) || !l.tc || l.tc->type == kTrNone) return false;
  const int smax = chain_multi_max_sweeps(g.m);
  if (nPre > smax || nPost > smax) return false;
  TileQuery down, up;
  down.launch = up.launch = kTileChainMulti;
  down.te = up.te = g.m;
  down.kb = up.kb = kMultiKB;
  down.halo = nPre;
  down.restrict_kind = l.tc->type == kTrChain ? kChainToChain : kChainToAgg;
  down.align = l.tc->type == kTrAgg ? std::max(l.tc->rho, 1) : 1;
  up.halo = nPost;
  return launch_has_tile(down) && launch_has_tile(up);
}

// A fused block-tridiagonal level in column groups (always on): block-Jacobi sweeps on a K-column form, each half one
// launch of btd_multi_kernel where the single-column cycle runs one fused launch.
static bool multi_btd_level_ok(const aggmg_ctx*, const aggmg_hier* h, int k, int nPre, int nPost) {
  const Level& l = h->lv[k];
  const BtdDev& b = *l.S->btd;
  const TransferBtd& t = *l.tb;
  if (l.S->gs || !multi_form(b.m, b.cmp)) return false;
  if (t.mc != 2 || t.rho <= 0 || b.ne != (int64_t)t.rho * t.nec) return false;
  if (t.ld && h->restriction == AGGMG_RESTRICT_PRECONDITIONED) return false;
  // the single-column cycle's launches at this level are single fused launches (no chunked sweeps) ...
  if (!btd_launch_ok(*l.S, nPre, 1, &t) || !btd_launch_ok(*l.S, nPost, 0, nullptr)) return false;
  // ... and the K-column tile holds the same halos
  TileQuery down, up;
  down.launch = up.launch = kTileMulti;
  down.te = up.te = kMultiNT / b.m;
  down.halo = nPre + 1;
  down.align = t.rho;
  up.halo = nPost;
  return launch_has_tile(down) && launch_has_tile(up);
}

// the family that runs level k in column groups, if one does: the switch of vcycle_multi_group
static bool multi_level_ok(const aggmg_ctx* ctx, const aggmg_hier* h, int k, int nPre, int nPost) {
  switch (level_path(h, k)) {
    case LevelPath::FusedChain: return multi_chain_level_ok(ctx, h, k, nPre, nPost);
    case LevelPath::FusedBtd: return multi_btd_level_ok(ctx, h, k, nPre, nPost);
    case LevelPath::Patch: return multi_patch_level_ok(ctx, h, k, nPre, nPost);
    default: return false;   // (the generic kernels; the coarsest level)
  }
}

static bool multi_ok(const aggmg_ctx* ctx, const aggmg_hier* h, int nPre, int nPost) {
  const int n = (int)h->lv.size();
  if (n < 2 || h->coarse_mode == AGGMG_COARSE_EXTERNAL) return false;
  for (int k = 0; k < n - 1; ++k)
    if (!multi_level_ok(ctx, h, k, nPre, nPost)) return false;
  return true;
}

template <int M, bool CMP, bool SYM>
static int launch_multi_t(aggmg_ctx* ctx, MultiArgs m, const SweepWeights& wts, int halo) {
  constexpr int TE = kMultiNT / M;
  const int align = m.a.lf_out ? m.a.rho_out : 1;
  const int owned = multi_tile_owned(TE, halo, align);   // host_plan.hpp, the planner multi_level_ok asks
  if (owned <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column tile too small for the requested halo");
  m.a.owned = owned;
  m.a.halo_left = halo;
  const int64_t ntiles = (m.a.lv.ne + owned - 1) / owned;
  if (ntiles == 0) return AGGMG_OK;
  with_col_group(m.kc, kMultiKB, [&](auto g) {   // (never a group above the cycle's)
    constexpr int KB = decltype(g)::value;
    const size_t lds = (size_t)2 * KB * (TE + 2) * M * sizeof(double);
    hipLaunchKernelGGL((btd_multi_kernel<M, CMP, SYM, KB, kMultiNT>), dim3((unsigned)ntiles), dim3(kMultiNT), lds, ctx->stream, m, wts);
  });
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int launch_multi(aggmg_ctx* ctx, const BtdDev& b, const MultiArgs& m, const SweepWeights& wts, int halo) {
  int rc = AGGMG_OK;
  if (!with_form<multi_form>(b.m, b.cmp, [&](auto f) {
        using F = decltype(f);
        rc = b.bsym ? launch_multi_t<F::kM, F::kCmp, true>(ctx, m, wts, halo) : launch_multi_t<F::kM, F::kCmp, false>(ctx, m, wts, halo);
      }))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: block size not instantiated for the K-column kernel");
  return rc;
}

// ---- the K-column launches of a dictionary level on the element-thread layout (AGGMG_OPT_MULTI_ELEMENT_THREADS,
// multi_elem_kernels.hpp) -----------------------------------------------------------------------------
// Columns of a pass of btd_elem_rec_multi_kernel (profiles/r37_multi_elem_threads.md has the comparison).
#ifndef AGGMG_MULTI_ELEM_KB
#define AGGMG_MULTI_ELEM_KB 1
#endif
constexpr int kMultiElemKB = AGGMG_MULTI_ELEM_KB;

// Does a half of the K-column cycle on block-tridiagonal form b -- f: its launch after fused_ascent / fused_descent and
// fused_dictionary, halo: the half's -- take btd_elem_rec_multi_kernel?  The single-column route's conditions for
// btd_elem_rec_kernel (launch_btd_t): blocks of 4 rows, compressed and symmetric-packed; a dictionary launch the
// element-thread layout serves (elem_thread_args: at least one sweep among them) whose level has its packed class records
// under the cap (elem_record_args: with dup / corr where the launch forms a residual); a tile of kElemThreads elements that
// owns something under the half's halo.  Anything else keeps btd_multi_kernel.
static bool multi_elem_launch_ok(const aggmg_ctx* ctx, const BtdDev& b, const FusedLaunch& f, int halo) {
  if (!ctx->multi_elem_threads || b.m != 4 || !b.cmp || !b.bsym) return false;
  if (!elem_thread_args(ctx, f, false, 0) || !elem_record_args(ctx, f)) return false;
  return fused_tile_plan(kElemThreads, halo, f.lf_out ? f.rho_out : 1, false, f.agg_shift).owned > 0;
}

// One launch of btd_elem_rec_multi_kernel for the m.kc columns of a group: m.a is the dictionary launch
// multi_elem_launch_ok accepted, tiled like the single-column route's (fused_tile_plan, all tiles).
static int launch_multi_elem(aggmg_ctx* ctx, MultiArgs m, const FusedLaunch& f, int halo) {
  constexpr int M = 4;
  const FusedTilePlan plan = fused_tile_plan(kElemThreads, halo, m.a.lf_out ? m.a.rho_out : 1, false, m.a.agg_shift);   // host_plan.hpp
  if (plan.owned <= 0 || m.kc < 1) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column element-thread launch without a tile");
  m.a.agg_shift = plan.agg_shift;
  m.a.owned = plan.owned;
  m.a.halo_left = plan.halo_left;
  const TileSubset sub = fused_tile_subset(m.a.lv.ne, plan.owned, 0, 0, 0);
  m.a.tile_split = sub.split;
  m.a.tile_skip = sub.skip;
  if (sub.ntiles == 0) return AGGMG_OK;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)sub.ntiles), dim3(kElemThreads), elem_rec_multi_lds_bytes<M>(kMultiElemKB, f.rec.nclasses),
                       ctx->stream, m, f.wts, f.rec);
  };
  if (m.a.do_residual)
    go(btd_elem_rec_multi_kernel<M, true, kMultiElemKB>);
  else
    go(btd_elem_rec_multi_kernel<M, false, kMultiElemKB>);
  HIPCHK(hipGetLastError());
  ++ctx->multi_elem_launches;
  return AGGMG_OK;
}

// per-level K-column vectors for groups of `cols` columns (LevelCols: which a level has), multi_ld(h, k) doubles per
// column; a call with no more columns than before allocates nothing
static int multi_workspace(aggmg_ctx* ctx, aggmg_hier* h, int64_t cols) {
  if (h->multi_cols >= cols && !h->mu.empty()) return AGGMG_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (LevelCols& m : h->mu)
    for (DevArray<double>* p : {&m.u, &m.up, &m.rhs, &m.aux}) CHECK(p->reset(ctx));
  h->multi_cols = 0;
  const int n = (int)h->lv.size();
  h->mu.resize(n);
  for (int k = 0; k < n; ++k) {
    LevelCols& m = h->mu[k];
    // a chain level's vectors (and those a chain level keeps in block order) are zero-filled like the level's own
    // (aggmg_hier_create): the kernels rely on zeros in the padding rows of the trailing block
    const bool chain = level_path(h, k) == LevelPath::FusedChain || h->lv[k].native_io;
    auto vec = [&](DevArray<double>& v) { return v.alloc(ctx, multi_ld(h, k) * cols, chain); };
    CHECK(vec(m.u));
    if (k > 0 && k < n - 1) CHECK(vec(m.up));
    if (k > 0) CHECK(vec(m.rhs));
    if (level_path(h, k) == LevelPath::Patch) CHECK(vec(m.aux));
  }
  h->multi_cols = cols;
  return AGGMG_OK;
}

// The argument block of a btd_multi_kernel launch: the fused launch's own (after fused_ascent / fused_descent), kc columns
// and the column strides of its vectors (a null view: the launch has no such vector).
static MultiArgs multi_args(const FusedLaunch& f, int kc, ColsIn uin, ColsIn rhs, ColsOut uout, ColsIn uc, ColsOut rc) {
  MultiArgs m;
  std::memset(&m, 0, sizeof(m));
  m.a = f;
  multi_strides(m, kc, uin, rhs, uout, uc, rc);
  return m;
}

// ---- the halves of a level of the K-column cycle, kc columns each: one pair per family, one argument list (cgt.hip has
// the chain family's, cgt_multi_down / cgt_multi_up) ------------------------------------------------------------------------
// A block-tridiagonal level (multi_btd_level_ok).  Descent: nPre sweeps from uin (null: zero) into the level's u, the
// explicit residual and its restriction into the next level's right-hand sides, one launch -- of btd_multi_kernel on the
// level's full arrays, or (multi_elem_launch_ok) of btd_elem_rec_multi_kernel on its dictionary.
static FusedLaunch btd_multi_down_args(const aggmg_hier* h, int k, ColsIn uin, ColsIn rhs, ColsOut u, ColsOut rc, int nPre, double alpha) {
  const Level& l = h->lv[k];
  FusedLaunch f = fused_sweeps(*l.S->btd, uin.p, rhs.p, u.p, l.damp_pre(alpha), nPre);
  fused_descent(f, h, l, rc.p);   // (lf: multi_btd_level_ok refuses the levels that would take (L'D))
  return f;
}
static int btd_multi_down(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn uin, ColsIn rhs, int nPre, double alpha, int kc) {
  Level& l = h->lv[k];
  const ColsOut u = multi_vec(h, k, &LevelCols::u), rc = multi_vec(h, k + 1, &LevelCols::rhs);
  const FusedLaunch f = btd_multi_down_args(h, k, uin, rhs, u, rc, nPre, alpha);
  ProfScope ps(ctx, AGGMG_KIND_FUSED_DOWN, k);
  FusedLaunch d = f;
  fused_dictionary(d, l);
  if (multi_elem_launch_ok(ctx, *l.S->btd, d, nPre + 1)) return launch_multi_elem(ctx, multi_args(d, kc, uin, rhs, u, ColsIn(), rc), d, nPre + 1);
  return launch_multi(ctx, *l.S->btd, multi_args(f, kc, uin, rhs, u, ColsIn(), rc), f.wts, nPre + 1);
}
// Ascent: prolong-add of the coarse result onto the level's u, nPost sweeps, into dst, one launch.
static FusedLaunch btd_multi_up_args(const aggmg_hier* h, int k, ColsIn u, ColsIn rhs, ColsIn uc, ColsOut dst, int nPost, double alpha) {
  const Level& l = h->lv[k];
  FusedLaunch f = fused_sweeps(*l.S->btd, u.p, rhs.p, dst.p, l.damp_post(alpha), nPost);
  fused_ascent(f, l, uc.p);
  return f;
}
static int btd_multi_up(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn rhs, int nPost, double alpha, ColsOut dst, int kc) {
  Level& l = h->lv[k];
  const ColsIn u = multi_vec(h, k, &LevelCols::u), uc = multi_coarse_result(h, k);
  const FusedLaunch f = btd_multi_up_args(h, k, u, rhs, uc, dst, nPost, alpha);
  ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, k);
  FusedLaunch d = f;
  fused_dictionary(d, l);
  if (multi_elem_launch_ok(ctx, *l.S->btd, d, nPost)) return launch_multi_elem(ctx, multi_args(d, kc, u, rhs, dst, uc, ColsOut()), d, nPost);
  return launch_multi(ctx, *l.S->btd, multi_args(f, kc, u, rhs, dst, uc, ColsOut()), f.wts, nPost);
}

// Which halves of level k of a K-column V(nPre, nPost) cycle btd_elem_rec_multi_kernel would serve: the predicate of the
// two functions above on the launches they would prepare (the vectors do not enter it), on a hierarchy whose K-column
// cycle runs in groups.
extern "C" int aggmg_hier_level_multi_element_threads(aggmg_ctx* ctx, const aggmg_hier* h, int level, int nPre, int nPost, int* down,
                                                      int* up) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !down || !up) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_multi_element_threads: NULL argument");
  if (level < 0 || level >= (int)h->lv.size()) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_multi_element_threads: level out of range");
  if (nPre < 0 || nPost < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_multi_element_threads: negative sweep count");
  *down = *up = 0;
  if (level_path(h, level) != LevelPath::FusedBtd || !multi_ok(ctx, h, nPre, nPost)) return AGGMG_OK;
  const Level& l = h->lv[level];
  FusedLaunch dn = btd_multi_down_args(h, level, ColsIn(), ColsIn(), ColsOut(), ColsOut(), nPre, 1.0);
  FusedLaunch as = btd_multi_up_args(h, level, ColsIn(), ColsIn(), ColsIn(), ColsOut(), nPost, 1.0);
  fused_dictionary(dn, l);
  fused_dictionary(as, l);
  *down = multi_elem_launch_ok(ctx, *l.S->btd, dn, nPre + 1) ? 1 : 0;
  *up = multi_elem_launch_ok(ctx, *l.S->btd, as, nPost) ? 1 : 0;
  return AGGMG_OK;
}

extern "C" int aggmg_multi_element_thread_launches(aggmg_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_multi_element_thread_launches: NULL argument");
  *count = ctx->multi_elem_launches;
  return AGGMG_OK;
}

// The tile of a K-column element-thread launch with `halo` elements of halo each side (nPre + 1 in the descent, nPost in the
// ascent) that restricts to agglomerates of rho elements (1: no restriction): what launch_multi_elem runs.
extern "C" int aggmg_multi_element_tile_plan(int halo, int rho, int* tile_elems, int* owned) {
  if (!tile_elems || !owned || halo < 0 || rho < 1) return AGGMG_ERR_ARGUMENT;
  *tile_elems = kElemThreads;
  *owned = fused_tile_plan(kElemThreads, halo, rho, false, -1).owned;   // host_plan.hpp
  return AGGMG_OK;
}

// A patch level (multi_patch_level_ok), the launches of patch_down / patch_up for kc columns each.  Descent: the pre sweeps
// from uin (null: zero; none at nPre == 0) into the level's u, then the zero-sweep K-column launch on the smoother's element
// blocks -- explicit residual and its restriction into the next level's right-hand sides (always the explicit residual, as
// patch_down).
static int multi_patch_down(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn uin, ColsIn rhs, int nPre, double alpha, int kc) {
  Level& l = h->lv[k];
  const PatchDev& P = *l.S->patch;
  const ColsOut u = multi_vec(h, k, &LevelCols::u), rc = multi_vec(h, k + 1, &LevelCols::rhs);
  if (nPre > 0) CHECK(patch_smooth_multi(ctx, P, uin, rhs, l.damp_pre(alpha), nPre, false, u, multi_vec(h, k, &LevelCols::aux), kc, k));
  // (no sweep: the launch also copies the iterate the ascent starts from)
  const ColsIn src = nPre > 0 ? ColsIn(u) : uin;
  FusedLaunch f = fused_sweeps(*P.btd, src.p, rhs.p, nPre > 0 ? nullptr : u.p, 0.0, 0);
  fused_descent(f, h, l, rc.p);
  f.ld_out = nullptr;   // the explicit residual's restriction, as patch_down
  f.lf_out = l.tb->lf;
  ProfScope ps(ctx, AGGMG_KIND_FUSED_DOWN, k);
  return launch_multi(ctx, *P.btd, multi_args(f, kc, src, rhs, u, ColsIn(), rc), f.wts, 1);
}
// Ascent: the zero-sweep K-column prolong-add of the level's u into its aux, then the reverse sweeps into dst (u, read for
// the last time by the prolongation, is the second vector of a chunked run); no sweep: the prolonged iterate goes to dst
// at once.
static int multi_patch_up(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn rhs, int nPost, double alpha, ColsOut dst, int kc) {
  Level& l = h->lv[k];
  const PatchDev& P = *l.S->patch;
  const ColsOut u = multi_vec(h, k, &LevelCols::u), mid = nPost > 0 ? multi_vec(h, k, &LevelCols::aux) : dst;
  const ColsIn uc = multi_coarse_result(h, k);
  {
    FusedLaunch f = fused_sweeps(*P.btd, u.p, rhs.p, mid.p, 0.0, 0);
    fused_ascent(f, l, uc.p);
    ProfScope ps(ctx, AGGMG_KIND_FUSED_UP, k);
    CHECK(launch_multi(ctx, *P.btd, multi_args(f, kc, u, rhs, mid, uc, ColsOut()), f.wts, 0));
  }
  if (nPost == 0) return AGGMG_OK;
  return patch_smooth_multi(ctx, P, mid, rhs, l.damp_post(alpha), nPost, true, dst, u, kc, k);
}

// kc columns of a K-column cycle whose every non-coarsest level multi_level_ok accepts: X0 (null: zero guesses), B and X
// are the group's columns of the caller's matrices
static int vcycle_multi_group(aggmg_ctx* ctx, aggmg_hier* h, ColsIn X0, ColsIn B, int nPre, int nPost, double alpha, ColsOut X,
                              int kc) {
  const int n = (int)h->lv.size();
  for (int k = 0; k < n - 1; ++k) {   // descent (src/solvers.jl:28-37)
    const ColsIn uin = multi_uin(k, X0), rhs = multi_rhs(h, k, B);
    switch (level_path(h, k)) {
      case LevelPath::FusedChain: CHECK(cgt_multi_down(ctx, h, k, uin, rhs, nPre, alpha, kc)); break;
      case LevelPath::FusedBtd: CHECK(btd_multi_down(ctx, h, k, uin, rhs, nPre, alpha, kc)); break;
      case LevelPath::Patch: CHECK(multi_patch_down(ctx, h, k, uin, rhs, nPre, alpha, kc)); break;
      default: return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column cycle on a level no K-column family runs");
    }
  }
  // coarsest solve (:39): one launch sequence for the group
  CHECK(coarse_solve_multi(ctx, h, multi_vec(h, n - 1, &LevelCols::rhs), multi_vec(h, n - 1, &LevelCols::u), kc));
  for (int k = n - 2; k >= 0; --k) {   // ascent (:41-47)
    const ColsIn rhs = multi_rhs(h, k, B);
    const ColsOut dst = multi_dst(h, k, X);
    switch (level_path(h, k)) {
      case LevelPath::FusedChain: CHECK(cgt_multi_up(ctx, h, k, rhs, nPost, alpha, dst, kc)); break;
      case LevelPath::FusedBtd: CHECK(btd_multi_up(ctx, h, k, rhs, nPost, alpha, dst, kc)); break;
      case LevelPath::Patch: CHECK(multi_patch_up(ctx, h, k, rhs, nPost, alpha, dst, kc)); break;
      default: return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column cycle on a level no K-column family runs");
    }
  }
  return AGGMG_OK;
}

static bool ranges_overlap(const double* a, int64_t na, const double* b, int64_t nb) {
  if (!a || !b) return false;
  return a < b + nb && b < a + na;
}

// The argument checks every K-column entry point makes once its pointers are known to be there, in the order they fire:
// the column count; the entry point's own complaint (`own`: null when it has none); the stride; the output against the
// inputs it must not overlap (`overlap`: the complaint; a null input overlaps nothing); the externally solved coarsest
// level (h: null for an entry point without a hierarchy).
static int multi_entry_check(aggmg_ctx* ctx, const char* who, int64_t N, int64_t ncols, int64_t ld, const char* own, ColsOut out,
                             std::initializer_list<ColsIn> in, const char* overlap, const aggmg_hier* h) {
  auto bad = [&](const std::string& what) { return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": " + what); };
  if (ncols < 1) return bad("ncols must be >= 1");
  if (own) return bad(own);
  if (ld < N) return bad("ld must be >= N (" + std::to_string(N) + ")");
  const int64_t span = (ncols - 1) * ld + N;   // doubles from the first column's start to the last one's end
  for (const ColsIn& v : in)
    if (ranges_overlap(out.p, span, v.p, span)) return bad(overlap);
  if (h && h->coarse_mode == AGGMG_COARSE_EXTERNAL) return bad("hierarchy was created with AGGMG_COARSE_EXTERNAL");
  return AGGMG_OK;
}

// the coarsest-level system for ncols column-major columns, in the cycle's groups
static int coarse_solve_cols(aggmg_ctx* ctx, aggmg_hier* h, ColsIn B, int64_t ncols, ColsOut X) {
  const int64_t group = std::min<int64_t>(ncols, kMultiKB);
  h->last_coarse_ms = 0.0;
  for (int64_t c0 = 0; c0 < ncols; c0 += group) CHECK(coarse_solve_multi(ctx, h, B.at(c0), X.at(c0), (int)std::min<int64_t>(group, ncols - c0)));
  return AGGMG_OK;
}

// x = A_n \ b (src/solvers.jl:39; for a one-level hierarchy the reference's `A \ B`, :120) for ncols columns
extern "C" int aggmg_hier_coarse_solve_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* B, int64_t ncols, int64_t ld,
                                                 double* X) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !B || !X) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_coarse_solve_multi_dev: NULL argument");
  const ColsIn Bc(B, ld);
  const ColsOut Xc(X, ld);
  CHECK(multi_entry_check(ctx, "aggmg_hier_coarse_solve_multi_dev", h->lv.back().N, ncols, ld, nullptr, Xc, {Bc}, "X must not overlap B", h));
  return coarse_solve_cols(ctx, h, Bc, ncols, Xc);
}

extern "C" int aggmg_vcycle_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* X0, const double* B, int64_t ncols,
                                      int64_t ld, int nPre, int nPost, double alpha, double* X) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !B || !X) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_multi_dev: NULL argument");
  const ColsIn X0c(X0, ld), Bc(B, ld);
  const ColsOut Xc(X, ld);
  CHECK(multi_entry_check(ctx, "aggmg_vcycle_multi_dev", h->lv[0].N, ncols, ld, (nPre < 0 || nPost < 0) ? "negative sweep count" : nullptr,
                          Xc, {X0c, Bc}, "X must not overlap X0 or B", h));
  if (h->lv.size() == 1) return coarse_solve_cols(ctx, h, Bc, ncols, Xc);   // the cycle is the coarsest solve (:39)
  if (!multi_ok(ctx, h, nPre, nPost)) {   // column by column: the single-column cycle on every column slice
    for (int64_t j = 0; j < ncols; ++j) CHECK(aggmg_vcycle_dev(ctx, h, X0c.at(j).p, Bc.at(j).p, nPre, nPost, alpha, Xc.at(j).p));
    return AGGMG_OK;
  }
  CHECK(schedule_check(ctx, h, nPre, nPost));
  const int64_t group = std::min<int64_t>(ncols, kMultiKB);
  CHECK(multi_workspace(ctx, h, group));
  h->last_coarse_ms = 0.0;
  for (int64_t c0 = 0; c0 < ncols; c0 += group)
    CHECK(vcycle_multi_group(ctx, h, X0c.at(c0), Bc.at(c0), nPre, nPost, alpha, Xc.at(c0), (int)std::min<int64_t>(group, ncols - c0)));
  return AGGMG_OK;
}

extern "C" int aggmg_hier_multi_info(aggmg_ctx* ctx, const aggmg_hier* h, int64_t ncols, int nPre, int nPost, int* fused,
                                     int* group) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !fused || !group) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_multi_info: NULL argument");
  if (ncols < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_multi_info: ncols must be >= 1");
  if (nPre < 0 || nPost < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_multi_info: negative sweep count");
  const bool f = multi_ok(ctx, h, nPre, nPost);
  *fused = f ? 1 : 0;
  *group = f ? (int)std::min<int64_t>(ncols, kMultiKB) : 1;
  return AGGMG_OK;
}

// EXTENSION: sweeps of a fused multiplicative patch smoother -- under AGGMG_OPT_PATCH_SCHWARZ_MULTI also of a fused hybrid /
// additive one, which has no direction: `reverse` is accepted and ignored -- on ncols columns, in the cycle's column groups
extern "C" int aggmg_smooth_multi_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* U0, const double* B,
                                      int64_t ncols, int64_t ld, const double* weights, int nsweeps, int reverse, double* U) {
  CHECK(check_pair(ctx, A, sm, "aggmg_smooth_multi_dev"));
  if (!B || !U) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smooth_multi_dev: NULL argument");
  const char* own = (nsweeps < 0 || (nsweeps > 0 && !weights)) ? "negative sweep count or no weights" : nullptr;
  for (int s = 0; !own && s < nsweeps; ++s)
    if (!std::isfinite(weights[s])) own = "weight is not finite";
  const int64_t N = A->m;
  const ColsIn U0c(U0, ld), Bc(B, ld);
  const ColsOut Uc(U, ld);
  CHECK(multi_entry_check(ctx, "aggmg_smooth_multi_dev", N, ncols, ld, own, Uc, {U0c, Bc}, "U must not overlap U0 or B", nullptr));
  if (sm->patch && sm->A != A) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smooth_multi_dev: the smoother was set up on another operator");
  if (!sm->patch && sm->patch_width)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                "aggmg_smooth_multi_dev: the element-patch smoother runs the generic route (patches of " + std::to_string(sm->patch_width) +
                    " elements, or an operator the fused set-up does not take), not the fused one: K-column sweeps exist for fused "
                    "patches of two elements");
  if (!sm->patch)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_smooth_multi_dev: the smoother is not a fused element-patch smoother (K-column sweeps "
                                            "exist for the multiplicative patch smoother of aggmg_patch_gs_setup and, under "
                                            "AGGMG_OPT_PATCH_SCHWARZ_MULTI, for the fused smoothers of aggmg_patch_schwarz_setup)");
  const PatchDev& P = *sm->patch;
  if (!P.multiplicative && !ctx->patch_schwarz_multi)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_smooth_multi_dev: the smoother is an additive / hybrid patch smoother, not the multiplicative one "
                                            "(its K-column sweeps are opt-in: AGGMG_OPT_PATCH_SCHWARZ_MULTI)");
  if (!(P.multiplicative ? patch_multi_form_ok(P) : patch_schwarz_multi_form_ok(P)))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                "aggmg_smooth_multi_dev: the K-column sweep kernel is not instantiated for " + std::to_string(P.m) + " rows per element with " +
                    (P.btd->cmp ? "compressed" : "dense") + " couplings (compressed: 2 or 4, dense: 2)");
  if (N == 0) return AGGMG_OK;
  if (nsweeps == 0) {   // the iterate as it is
    if (U0)
      HIPCHK(hipMemcpy2DAsync(U, ld * sizeof(double), U0, ld * sizeof(double), N * sizeof(double), (size_t)ncols, hipMemcpyDeviceToDevice, ctx->stream));
    else
      HIPCHK(hipMemset2DAsync(U, ld * sizeof(double), 0, N * sizeof(double), (size_t)ncols, ctx->stream));
    return AGGMG_OK;
  }
  const int64_t group = std::min<int64_t>(ncols, kMultiKB);
  for (int64_t c0 = 0; c0 < ncols; c0 += group)
    CHECK(patch_smooth_multi(ctx, P, U0c.at(c0), Bc.at(c0), Damping(0.0, weights), nsweeps, reverse != 0, Uc.at(c0), ColsOut(),
                             (int)std::min<int64_t>(group, ncols - c0), 0));
  return AGGMG_OK;
}

// ---- the cycle sequence of aggmg_vcycles_dev and aggmg_multigrid_dev ------------------------------------------------
// Between two cycles the fine level runs post-smoothing of cycle i and pre-smoothing of cycle i+1
// on the same iterate with the same right-hand side, so both go into ONE fused launch
// (prolongation-add -> nPost + nPre sweeps -> restriction): the fine operator is read once per
// cycle instead of twice and the intermediate iterates never travel to HBM.  The arithmetic is
// that of ncycles separate aggmg_vcycle_dev calls.

// levels 1.. of one cycle: rhs_1 is in lv[1].rhs (descend) or every right-hand side is in place already; result u_1
static int coarse_levels(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPre, int nPost, double alpha, bool descend) {
  const int n = (int)h->lv.size();
  if (descend) CHECK(vcycle_down(ctx, h, nullptr, b, nPre, alpha, 1));
  Level& c = h->lv[n - 1];
  CHECK(coarse_solve(ctx, h, c.rhs, c.u[0]));
  if (n > 2) CHECK(vcycle_up(ctx, h, b, nPost, alpha, nullptr, 1));
  return AGGMG_OK;
}

// upper bounds of the tiles of a checkpoint launch (its partial sums: two doubles per tile and checkpoint), from the
// planner the launches run (host_plan.hpp): sweeps = the most any of them takes (+ the residual rows), tout = the
// transfer the one between two cycles restricts through (null: none restricts)
static int64_t btd_chk_tiles(const BtdDev& b, int sweeps, const TransferBtd* tout) {
  return fused_chk_reserve(b.ne, btd_tile_elems(b), sweeps + 1, tout && tout->rho ? tout->rho : 1, tout && !tout->rho,
                           tout ? xfer_agg_shift(*tout) : -1);
}
// (chain kernel: a block of halo per sweep and side, two for the residual, one for the restriction)
static int64_t cgt_chk_tiles(const CgtDev& g, int sweeps, int rho) {
  return chain_chk_reserve(g.ne, cgt_tile_blocks(g.m), 2 * sweeps + 3, std::max(rho, 1));
}

// The fine level of the sequence: the fused block-tridiagonal kernel, or the chain kernel of a CG mesh (cgt.hip).
// chk: the launch forms a checkpoint's sums and reports its tile count there.
struct FineLevel {
  aggmg_ctx* ctx;
  aggmg_hier* h;
  const double* b;
  int nPre, nPost;
  double alpha;
  bool chain() const { return level_path(h, 0) == LevelPath::FusedChain; }
  Level& l0() const { return h->lv[0]; }
  // post-smoothing of one cycle, pre-smoothing and restriction of the next: cur -> alt
  int mid(const double* cur, double* alt, CgtChk* chk) const {
    return (chain() ? cgt_mid : btd_mid)(ctx, h, cur, alt, b, nPost + nPre, alpha, chk);
  }
  // the ascent alone: src -> dst
  int up(const double* src, double* dst, CgtChk* chk) const {
    return chain() ? cgt_up(ctx, h, 0, b, nPost, alpha, dst, src, chk) : btd_up(ctx, h, 0, b, nPost, alpha, dst, src, chk);
  }
  int64_t chk_tiles() const {
    return chain() ? cgt_chk_tiles(*l0().S->cgt, nPost + nPre, l0().tc ? l0().tc->rho : 1)
                 : btd_chk_tiles(*l0().S->btd, nPost + nPre, l0().tb.get());
  }
};

// Does level 0 have the launch between two cycles (cgt_mid / btd_mid) that cycle_loop is built on -- for plain cycles
// (aggmg_vcycles_dev) or with the checkpoints of aggmg_multigrid_dev?  Otherwise the callers run cycle by cycle.
enum class MidFor { PlainCycles, Checkpointed };
static bool fine_mid_ok(const aggmg_hier* h, int nPre, int nPost, MidFor purpose) {
  const bool chk = purpose == MidFor::Checkpointed;
  const Level& l0 = h->lv[0];
  if (h->coarse_mode == AGGMG_COARSE_EXTERNAL) return false;   // the loop runs the coarsest solve itself
  switch (level_path(h, 0)) {
    case LevelPath::FusedChain:
      // sweeps: the checkpoint variant of the chain kernel is point Jacobi's (sw 0); plain cycles take all but red-black GS (3)
      if (chk ? l0.S->cgt->sw != 0 : l0.S->cgt->sw == 3) return false;
      // a checkpoint needs its sweeps in ONE launch; plain cycles chunk a longer run (cgt_mid)
      return !chk || nPost + nPre <= cgt_max_fused_sweeps(*l0.S->cgt);
    case LevelPath::FusedBtd:
      if (l0.S->gs) return false;
      // restriction: checkpoints form residual rows for their norms -- the explicit form alone; plain cycles want the
      // mode's own form to exist (a single descent, btd_down, takes any: without (L'D) it restricts with lf)
      if (h->restriction != AGGMG_RESTRICT_EXPLICIT && (chk || !l0.tb->ld)) return false;
      return btd_launch_ok(*l0.S, nPre + nPost, 1, l0.tb.get());   // (no tile: a ratio the halo leaves no room for)
    case LevelPath::Patch:         // (no launch between two cycles: the loops run cycle by cycle, as on a generic fine level)
    case LevelPath::BtdTransfer:
    case LevelPath::Generic:
    case LevelPath::Coarsest: break;
  }
  return false;
}

// Histories and stopping test of launches with checkpoints (with the outer solver loops below)
struct ChkHist {
  WorkLease hold;                                          // part and mid lie in it (chk_buffers)
  double *part = nullptr, *mid = nullptr, *sc = nullptr;   // on the device: tile sums, their partial reduction, the norms
  int64_t cap = 0;                                       // tiles `part` has room for (per checkpoint)
  const double* u_exact = nullptr;
  double tol_nb = 0.0;
  double *res = nullptr, *err = nullptr;
  int checks = 0;
};
static int chk_collect(aggmg_ctx* ctx, ChkHist& H, int nchk, int64_t ntiles, int* met);

// ncycles cycles from x0 into x_out.  H (or null: no checks): the residual test (and the error norm) of every
// check_every-th cycle and of the last one are formed INSIDE the fine-level launch that post-smooths it; the loop stops
// at the first one that meets the tolerance.  *done: the cycles run.
static int cycle_loop(const FineLevel& f, const double* x0, int ncycles, double* x_out, int check_every, ChkHist* H, int* done) {
  aggmg_ctx* ctx = f.ctx;
  aggmg_hier* h = f.h;
  h->last_coarse_ms = 0.0;
  CHECK(schedule_check(ctx, h, f.nPre, f.nPost));
  CHECK(vcycle_down(ctx, h, x0, f.b, f.nPre, f.alpha, 0));                    // cycle 1: every level down ...
  CHECK(coarse_levels(ctx, h, f.b, f.nPre, f.nPost, f.alpha, false));         // ... the coarsest solve and the coarser levels up
  double* cur = f.l0().u[0];   // pre-smoothed fine iterate of the current cycle
  double* alt = f.l0().u[1];
  for (int it = 1; it <= ncycles; ++it) {
    const bool last = it == ncycles;
    const bool check = H && ((it % check_every == 0) || last);
    CgtChk chk;   // one checkpoint per launch: x_it, after the post-smoothing
    if (check) {
      chk.sweep = f.nPost;
      chk.exact = H->u_exact;
      chk.part = H->part;
      chk.cap = H->cap;
    }
    if (!last) {
      CHECK(f.mid(cur, alt, check ? &chk : nullptr));
      std::swap(cur, alt);
    } else {       // the last ascent: its result is x_ncycles
      CHECK(f.up(cur, x_out, check ? &chk : nullptr));
    }
    if (done) *done = it;
    if (check) {
      int met = -1;
      CHECK(chk_collect(ctx, *H, 1, chk.ntiles, &met));
      if (met >= 0) {   // src/solvers.jl:131
        // x_it passed through LDS only (no store per checked cycle: 8 B/DoF saved every time).  The launch's input --
        // the pre-smoothed iterate of cycle `it`, now in alt -- and the coarse correction are untouched: the
        // ascent once more, alone, gives x_it with the same arithmetic
        if (!last) CHECK(f.up(alt, x_out, nullptr));
        break;
      }
    }
    if (!last) CHECK(coarse_levels(ctx, h, f.b, f.nPre, f.nPost, f.alpha, true));
  }
  return AGGMG_OK;
}

// ncycles V-cycles back to back, x <- V(x, b): the hot loop of multigrid() (src/solvers.jl:124-126) -- cycle_loop
// without checks where the fine level has a fused launch between two cycles.
extern "C" int aggmg_vcycles_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int ncycles,
                                 int nPre, int nPost, double alpha, double* x_out) {
  CHECK(vcycle_args(ctx, h, x0, b, nPre, nPost));
  if (!x_out || ncycles < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycles: bad argument");
  if (x_out == x0 || x_out == b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycles: x_out must not alias x0 or b");
  if (h->coarse_mode == AGGMG_COARSE_EXTERNAL)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycles: hierarchy was created with AGGMG_COARSE_EXTERNAL");
  if (ncycles > 1 && fine_mid_ok(h, nPre, nPost, MidFor::PlainCycles))   // (a single cycle has no launch between two)
    return cycle_loop(FineLevel{ctx, h, b, nPre, nPost, alpha}, x0, ncycles, x_out, 0, nullptr, nullptr);
  // plain sequence; intermediate iterates ping-pong between two vectors owned by the hierarchy
  if (ncycles > 1)
    for (auto& p : h->cyc)
      if (!p) CHECK(p.alloc(ctx, h->lv[0].N));
  const double* src = x0;
  for (int c = 0; c < ncycles; ++c) {
    double* dst = (c == ncycles - 1) ? x_out : h->cyc[c & 1];
    CHECK(aggmg_vcycle_dev(ctx, h, src, b, nPre, nPost, alpha, dst));
    src = dst;
  }
  return AGGMG_OK;
}

extern "C" int aggmg_vcycle_down_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre,
                                     double alpha) {
  CHECK(vcycle_args(ctx, h, x0, b, nPre, 0));
  if (h->lv.size() < 2) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_down_dev: needs at least two levels");
  h->halves_used = true;
  return vcycle_down(ctx, h, x0, b, nPre, alpha);
}

// An ascent called on its own reads level 0's stored pre-smoothed iterate: from now on this hierarchy's cycles store it
// (aggmg_hier::halves_used), and there has to be one -- not after a replayed aggmg_vcycle_dev with no descent since.
static int fine_ascent_alone(aggmg_ctx* ctx, aggmg_hier* h, const char* who) {
  h->halves_used = true;
  if (h->fine_iterate_absent)
    return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": the last aggmg_vcycle_dev on this hierarchy replayed its pre-smoothing "
                "(AGGMG_OPT_REPLAY_PRESMOOTH) and stored no fine-level iterate for an ascent on its own; call aggmg_vcycle_down_dev first");
  return AGGMG_OK;
}

extern "C" int aggmg_vcycle_up_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPost, double alpha,
                                   double* x_out) {
  CHECK(vcycle_args(ctx, h, b, x_out, nPost, 0));
  if (h->lv.size() < 2) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_up_dev: needs at least two levels");
  if (x_out == b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_up_dev: x_out must not alias b");
  CHECK(fine_ascent_alone(ctx, h, "aggmg_vcycle_up_dev"));
  return vcycle_up(ctx, h, b, nPost, alpha, x_out);
}

// Does the fine level have the split ascent for nPost sweeps?  A fused block-tridiagonal level whose ascent is one fused
// launch, or a multiplicative patch level with the one-launch ascent (patch_split_ok).
static bool split_up_ok(const aggmg_hier* h, int nPost) {
  if (h->lv.size() < 2) return false;
  if (level_path(h, 0) == LevelPath::FusedBtd && btd_launch_ok(*h->lv[0].S, nPost, 0, nullptr)) return true;
  return patch_split_ok(h, nPost);
}
extern "C" int aggmg_vcycle_up_split_ok(aggmg_ctx* ctx, const aggmg_hier* h, int nPost, int* ok) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !ok) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_up_split_ok: NULL argument");
  *ok = nPost >= 0 && split_up_ok(h, nPost) ? 1 : 0;
  return AGGMG_OK;
}

// The ascent in three calls: part 0 the coarser levels (n-2 .. 1), part 1 the fine-level tiles that
// hold elements [0, head_elems) and [tail_elem, ne), part 2 the remaining fine-level tiles.  Parts
// 1 and 2 are independent of each other (tiles are), so they may run on different streams; the
// result is bitwise that of aggmg_vcycle_up_dev.
extern "C" int aggmg_vcycle_up_split_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPost, double alpha,
                                         double* x_out, int64_t head_elems, int64_t tail_elem, int part) {
  CHECK(vcycle_args(ctx, h, b, x_out, nPost, 0));
  if (h->lv.size() < 2) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_up_split_dev: needs at least two levels");
  if (x_out == b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_up_split_dev: x_out must not alias b");
  if (part < 0 || part > 3) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_up_split_dev: part is 0, 1, 2 or 3");
  CHECK(fine_ascent_alone(ctx, h, "aggmg_vcycle_up_split_dev"));
  if (part == 3) {   // the finest level alone, every tile (the coarser levels were run by part 0 / aggmg_vcycle_up_coarse_dev)
    TileSel all;
    all.mode = 3;
    return vcycle_up(ctx, h, b, nPost, alpha, x_out, 0, all);
  }
  if (!split_up_ok(h, nPost)) return no_split_ascent(ctx);
  if (part == 0) return h->lv.size() > 2 ? vcycle_up(ctx, h, b, nPost, alpha, x_out, 1) : AGGMG_OK;
  TileSel sel;
  sel.mode = part;  // 1 ends, 2 middle
  sel.head = head_elems;
  sel.tail = tail_elem;
  return vcycle_up(ctx, h, b, nPost, alpha, x_out, 0, sel);
}

extern "C" int aggmg_vcycle_up_coarse_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, int nPost, double alpha, int part,
                                          int64_t ghosts_lo, int64_t ghosts_hi) {
  CHECK(vcycle_args(ctx, h, b, b, nPost, 0));
  if (h->lv.size() < 4) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_vcycle_up_coarse_dev: needs two smoothed levels below the finest");
  if ((part != 1 && part != 2) || ghosts_lo < 0 || ghosts_hi < 0)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle_up_coarse_dev: part is 1 (ends, then the rest) or 2 (middle)");
  // (only hierarchies whose levels below the finest are ONE pair next to the coarsest level: the 4-level shape of the
  // benchmarks; anything else keeps the unsplit ascent)
  if (h->lv.size() != 4) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_vcycle_up_coarse_dev: hierarchy shape not supported");
  CoarseSplit cs;
  cs.mode = part;
  cs.gh_lo = ghosts_lo;
  cs.gh_hi = ghosts_hi;
  return vcycle_up(ctx, h, b, nPost, alpha, nullptr, 1, TileSel(), cs);
}

extern "C" int aggmg_hier_set_restriction(aggmg_ctx* ctx, aggmg_hier* h, int mode) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || (mode != AGGMG_RESTRICT_EXPLICIT && mode != AGGMG_RESTRICT_PRECONDITIONED))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_set_restriction: bad argument");
  if (mode == AGGMG_RESTRICT_PRECONDITIONED) {
    // the rounding error this form puts on the smoothest mode grows like n^2 (x0.009 per cycle at
    // 2^20 fine elements, x0.134 at 2^22, x2.13 -- divergence -- at 2^24): refused where it would
    // exceed ~0.05 per cycle
    const Level& l0 = h->lv[0];
    const int64_t ne = (l0.S && l0.S->btd) ? l0.S->btd->ne : 0;
    if (ne > AGGMG_RESTRICT_PRECONDITIONED_MAX_ELEMS)
      return fail(ctx, AGGMG_ERR_UNSUPPORTED,
                  "aggmg_hier_set_restriction: AGGMG_RESTRICT_PRECONDITIONED is refused above " +
                      std::to_string((long long)AGGMG_RESTRICT_PRECONDITIONED_MAX_ELEMS) +
                      " fine elements (its rounding error on the smoothest mode grows like n^2 and makes the "
                      "multigrid iteration diverge at 2^24); this hierarchy has " + std::to_string((long long)ne));
  }
  h->restriction = mode;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_get_restriction(aggmg_ctx* ctx, const aggmg_hier* h, int* mode) {
  if (!ctx || !h || !mode) return AGGMG_ERR_ARGUMENT;
  *mode = h->restriction;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_coarse_buffers(aggmg_ctx* ctx, aggmg_hier* h, void** rhs_dev, void** sol_dev,
                                         int64_t* n) {
  if (!ctx || !h) return AGGMG_ERR_ARGUMENT;
  Level& c = h->lv.back();
  if (rhs_dev) *rhs_dev = c.rhs;
  if (sol_dev) *sol_dev = c.u[0];
  if (n) *n = c.N;
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// Host <-> device copies of the host-pointer entry points.  The caller's arrays are pageable (a Julia or NumPy
// heap); hipMemcpy stages such memory through ONE pinned buffer on ONE thread -- measured on the MI355X box:
// 13 - 14 GB/s, i.e. 28 ms for the three 134 MB vectors of a config-3 cycle that computes in 0.7 ms, and
// page-locking the arrays for the call (hipHostRegister) costs what it saves.  Here kStageLanes worker threads each
// take a slice of the vector and pipeline it through their own two pinned chunks on their own stream: the host
// memcpy (the part a single thread cannot do at PCIe speed) runs in parallel and overlaps with the DMA.
// ---------------------------------------------------------------------------------------------
#include <thread>
namespace {
constexpr size_t kStageChunk = (size_t)4 << 20;
constexpr int kStageMaxLanes = 8;

int stage_lanes(aggmg_ctx* ctx) {
  if (!ctx->stage.empty()) return (int)ctx->stage.size();
  if (ctx->stage_failed) return -1;  // an earlier attempt could not get its streams / pinned chunks: plain copies from then on
  // (measured on the MI355X box, three 134 MB vectors: 28.5 ms through hipMemcpy, 20.5 ms with 8 lanes, 16.8 ms with 4)
  int n = std::min(4, (int)std::thread::hardware_concurrency());
  if (const char* e = std::getenv("AGGMG_STAGE_THREADS")) n = std::atoi(e);
  n = std::min(std::max(n, 1), kStageMaxLanes);
  // built aside and handed to the context only when every lane is complete: a half-built set must never be seen by
  // a later call (its workers would copy through null buffers)
  std::vector<aggmg_ctx::StageLane> lanes(n);
  bool ok = true;
  for (auto& L : lanes) {
    ok = ok && hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < 2 && ok; ++k) {
      ok = ok && hipHostMalloc(&L.pin[k], kStageChunk, hipHostMallocDefault) == hipSuccess;
      ok = ok && hipEventCreateWithFlags(&L.ev[k], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) break;
  }
  if (!ok) {
    for (auto& L : lanes) {
      for (int k = 0; k < 2; ++k) {
        if (L.ev[k]) (void)hipEventDestroy(L.ev[k]);
        if (L.pin[k]) (void)hipHostFree(L.pin[k]);
      }
      if (L.stream) (void)hipStreamDestroy(L.stream);
    }
    (void)hipGetLastError();
    ctx->stage_failed = true;
    return -1;
  }
  ctx->stage.swap(lanes);
  return n;
}

// one lane's slice [lo, hi) of a copy, chunk by chunk through its two pinned buffers
void stage_slice(int device, aggmg_ctx::StageLane* L, bool to_device, char* dev, char* host, size_t lo, size_t hi, int* status) {
  if (hipSetDevice(device) != hipSuccess) {
    *status = 1;
    return;
  }
  hipError_t e = hipSuccess;
  size_t pend_off[2] = {0, 0}, pend_len[2] = {0, 0};
  int k = 0;
  for (size_t off = lo; off < hi && e == hipSuccess; off += kStageChunk, k ^= 1) {
    const size_t len = std::min(kStageChunk, hi - off);
    if (to_device) {
      e = hipEventSynchronize(L->ev[k]);   // the DMA that last read this buffer (a fresh event is complete)
      if (e != hipSuccess) break;
      std::memcpy(L->pin[k], host + off, len);
      e = hipMemcpyAsync(dev + off, L->pin[k], len, hipMemcpyHostToDevice, L->stream);
      if (e == hipSuccess) e = hipEventRecord(L->ev[k], L->stream);
    } else {
      if (pend_len[k]) {                   // drain what this buffer holds from two chunks ago
        e = hipEventSynchronize(L->ev[k]);
        if (e != hipSuccess) break;
        std::memcpy(host + pend_off[k], L->pin[k], pend_len[k]);
      }
      e = hipMemcpyAsync(L->pin[k], dev + off, len, hipMemcpyDeviceToHost, L->stream);
      if (e == hipSuccess) e = hipEventRecord(L->ev[k], L->stream);
      pend_off[k] = off, pend_len[k] = len;
    }
  }
  if (!to_device)
    for (int j = 0; j < 2 && e == hipSuccess; ++j, k ^= 1)   // oldest first
      if (pend_len[k]) {
        e = hipEventSynchronize(L->ev[k]);
        if (e == hipSuccess) std::memcpy(host + pend_off[k], L->pin[k], pend_len[k]);
        pend_len[k] = 0;
      }
  if (e == hipSuccess) e = hipStreamSynchronize(L->stream);
  *status = e == hipSuccess ? 0 : 1;
}

// nvec copies of `bytes` each, all lanes working on one vector after the other; synchronous
int stage_copy(aggmg_ctx* ctx, bool to_device, int nvec_in, double* const* dev_in, double* const* host_in, size_t bytes) {
  if (!bytes || !nvec_in) return AGGMG_OK;
  // vectors in memory the caller page-locked for good (aggmg_host_register / aggmg_host_alloc): one asynchronous copy
  // each on the compute stream, DMA straight from / to the caller's pages; the rest is staged as pageable memory
  double* dev[4];
  double* host[4];
  int nvec = 0;
  bool direct = false;
  for (int v = 0; v < nvec_in; ++v) {
    if (host_is_pinned(ctx, host_in[v], bytes)) {
      if (to_device) HIPCHK(hipMemcpyAsync(dev_in[v], host_in[v], bytes, hipMemcpyHostToDevice, ctx->stream));
      else HIPCHK(hipMemcpyAsync(host_in[v], dev_in[v], bytes, hipMemcpyDeviceToHost, ctx->stream));
      direct = true;
    } else if (nvec < 4) {
      dev[nvec] = dev_in[v];
      host[nvec] = host_in[v];
      ++nvec;
    }
  }
  if (!nvec) {
    if (direct && !to_device) HIPCHK(hipStreamSynchronize(ctx->stream));   // the caller reads the result next
    return AGGMG_OK;                                                         // (copies in: the cycle is ordered behind them)
  }
  const int lanes = bytes < 4 * kStageChunk ? 0 : stage_lanes(ctx);
  if (lanes <= 0) {   // short vectors (or no pinned memory to be had): the plain copy
    for (int v = 0; v < nvec; ++v) {
      if (to_device) HIPCHK(hipMemcpyAsync(dev[v], host[v], bytes, hipMemcpyHostToDevice, ctx->stream));
      else HIPCHK(hipMemcpyAsync(host[v], dev[v], bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return AGGMG_OK;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));   // the lanes' streams are not ordered with the compute stream
  std::vector<int> status(lanes, 0);
  std::vector<std::thread> th;
  th.reserve(lanes);
  for (int t = 0; t < lanes; ++t)
    th.emplace_back([&, t] {
      for (int v = 0; v < nvec && !status[t]; ++v) {
        size_t lo = 0, hi = 0;
        stage_lane_range(bytes, lanes, t, &lo, &hi);   // host_plan.hpp
        if (hi > lo) stage_slice(ctx->device, &ctx->stage[t], to_device, (char*)dev[v], (char*)host[v], lo, hi, &status[t]);
      }
    });
  for (auto& t : th) t.join();
  for (int st : status)
    if (st) return fail(ctx, AGGMG_ERR_HIP, "host <-> device staging copy failed");
  return AGGMG_OK;
}
}  // namespace

extern "C" int aggmg_vcycle(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int nPre, int nPost,
                            double alpha, double* x_out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !b || !x_out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_vcycle: NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t N = h->lv[0].N;
  const size_t bytes = (size_t)N * sizeof(double);
  // the three device vectors of the host-pointer entry live with the hierarchy (no allocation per call)
  for (auto& p : h->io)
    if (!p) CHECK(p.alloc(ctx, N));
  if (x0) {
    double* dv[2] = {h->io[0], h->io[1]};
    double* hv[2] = {const_cast<double*>(x0), const_cast<double*>(b)};
    CHECK(stage_copy(ctx, true, 2, dv, hv, bytes));
  } else {   // zero initial guess (ldiv!): one vector less over PCIe
    double* dv[1] = {h->io[1]};
    double* hv[1] = {const_cast<double*>(b)};
    CHECK(stage_copy(ctx, true, 1, dv, hv, bytes));
  }
  CHECK(aggmg_vcycle_dev(ctx, h, x0 ? h->io[0] : nullptr, h->io[1], nPre, nPost, alpha, h->io[2]));
  {
    double* dv[1] = {h->io[2]};
    double* hv[1] = {x_out};
    CHECK(stage_copy(ctx, false, 1, dv, hv, bytes));
  }
  return AGGMG_OK;
}

extern "C" int aggmg_hier_level_kind(aggmg_ctx* ctx, const aggmg_hier* h, int level, int* kind) {
  if (!ctx || !h || !kind) return AGGMG_ERR_ARGUMENT;
  if (level < 0 || level >= (int)h->lv.size()) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_level_kind: level out of range");
  switch (level_path(h, level)) {
    case LevelPath::Coarsest: *kind = AGGMG_LEVEL_COARSEST; break;
    case LevelPath::FusedChain: *kind = AGGMG_LEVEL_FUSED_CHAIN; break;
    case LevelPath::FusedBtd: *kind = AGGMG_LEVEL_FUSED_BTD; break;
    case LevelPath::Patch:   // (fused sweeps; the level counts as fused where its transfer launches are)
      *kind = h->lv[level].tb ? AGGMG_LEVEL_FUSED_BTD : AGGMG_LEVEL_GENERIC;
      break;
    case LevelPath::BtdTransfer:   // (several launches per half-cycle, as the generic kernels)
    case LevelPath::Generic: *kind = AGGMG_LEVEL_GENERIC; break;
  }
  return AGGMG_OK;
}

// ---- compulsory bytes of a launch: what its arrays hold, each read or written once -------------
// (the denominator-free side of the roofline fraction: no halo re-reads, no cache effects, no CSR
// model -- the arrays in the format the level stores them)
// ncols: columns of a K-column launch (btd_multi_kernel) -- the vectors' bytes once per column, the operator's once
static void btd_launch_bytes(const BtdDev& b, bool sweeps, bool u_in, bool residual, bool r_out, const TransferBtd* tin,
                             const TransferBtd* tout, bool preconditioned, int64_t* rd, int64_t* wr, int64_t ncols = 1) {
  const int64_t m = b.m, ne = b.ne, N = ne * m, D = sizeof(double), K = ncols;
  const bool need_g = sweeps || (tout && preconditioned);
  const bool grp = btd_sym_form(b.m, b.cmp);
  const bool sym = grp && b.bsym;
  int64_t r = K * N * D, w = 0;                                             // b
  if (u_in) r += K * N * D;
  if (need_g) {
    r += sym ? ne * (m * (m + 1) / 2) * D : N * m * D;                       // B^{-1}: packed or full rows
    if (b.cmp) r += sym ? 0 : N * D;                                         // pcol (rebuilt from qrow when packed)
    else r += sym ? N * m * D : 2 * N * m * D;                               // sup, or P and Q
  }
  if (b.cmp) r += N * D;                                                     // qrow
  const bool explicit_res = residual && (r_out || (tout && !preconditioned));
  if (explicit_res) {
    r += N * m * D;                                                          // diagonal blocks
    if (b.cmp) r += N * D;                                                   // scol
    else r += (sym && need_g ? 1 : 2) * N * m * D;                           // sub (+ sup unless the sweeps read it already)
  }
  if (tin) {
    r += tin->lf1 ? N * D : N * tin->mc * D;                                 // rows of L
    r += K * tin->nec * tin->mc * D;                                         // coarse iterate
    if (!tin->rho) r += ne * 4;                                              // parent map
  }
  if (sweeps || tin) w += K * N * D;                                         // iterate
  if (r_out) w += K * N * D;
  if (residual && tout) {
    if (preconditioned)
      r += N * tout->mc * D;                                                 // rows of (L'D)'
    else if (tout != tin)
      r += tout->lf1 ? N * D : N * tout->mc * D;                             // rows of L (once when the launch prolongs with them too)
    if (!tout->rho) r += ne * 4 + (tout->nec + 1) * 4;
    w += K * tout->nec * tout->mc * D;
  }
  *rd = r;
  *wr = w;
}

extern "C" int aggmg_hier_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, int kind, int has_x0,
                                       int64_t* read_bytes, int64_t* write_bytes) {
  if (!ctx || !h || !read_bytes || !write_bytes) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_launch_bytes: NULL argument");
  if (level < 0 || level + 1 >= (int)h->lv.size())
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_launch_bytes: level out of range (the coarsest level has no fused launch)");
  // the launches of a replayed cycle (AGGMG_OPT_REPLAY_PRESMOOTH): the descent without its iterate store; the ascent reads
  // the first iterate where the storing one reads the stored iterate -- a vector only where there is a first iterate
  const bool replay = kind == AGGMG_KIND_REPLAY_DOWN || kind == AGGMG_KIND_REPLAY_UP;
  if (replay) {
    if (level_path(h, level) != LevelPath::FusedBtd)
      return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_hier_launch_bytes: only a fused block-tridiagonal level replays its pre-smoothing");
    kind = kind == AGGMG_KIND_REPLAY_DOWN ? AGGMG_KIND_FUSED_DOWN : AGGMG_KIND_FUSED_UP;
  }
  if (kind != AGGMG_KIND_FUSED_DOWN && kind != AGGMG_KIND_FUSED_UP && kind != AGGMG_KIND_FUSED_MID)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_launch_bytes: kind must be AGGMG_KIND_FUSED_DOWN / _UP / _MID or AGGMG_KIND_REPLAY_DOWN / _UP");
  const Level& l = h->lv[level];
  const bool down = kind != AGGMG_KIND_FUSED_UP, up = kind != AGGMG_KIND_FUSED_DOWN;
  const LevelPath path = level_path(h, level);
  if (path == LevelPath::FusedChain) return cgt_launch_bytes(ctx, h, level, down, up, has_x0 != 0, read_bytes, write_bytes);
  if (path == LevelPath::Patch)   // (its sweep launch: aggmg_smoother_launch_bytes)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_hier_launch_bytes: an element-patch Schwarz level runs its sweeps and its transfer in several launches");
  if (path != LevelPath::FusedBtd)
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_hier_launch_bytes: the level runs the generic kernels (several launches)");
  const bool pre = l.tb->ld && h->restriction == AGGMG_RESTRICT_PRECONDITIONED;
  btd_launch_bytes(*l.S->btd, true, (up && !replay) || has_x0, down, false, up ? l.tb.get() : nullptr, down ? l.tb.get() : nullptr, pre,
                   read_bytes, write_bytes);
  if (replay && down) *write_bytes -= l.N * (int64_t)sizeof(double);   // the pre-smoothed iterate stays in the launch
  return AGGMG_OK;
}

extern "C" int aggmg_hier_multi_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, int kind, int has_x0,
                                             int64_t ncols, int64_t* read_bytes, int64_t* write_bytes) {
  if (!ctx || !h || !read_bytes || !write_bytes)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_multi_launch_bytes: NULL argument");
  if (level < 0 || level + 1 >= (int)h->lv.size())
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_multi_launch_bytes: level out of range (the coarsest level has no fused launch)");
  if (kind != AGGMG_KIND_FUSED_DOWN && kind != AGGMG_KIND_FUSED_UP)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_multi_launch_bytes: kind must be AGGMG_KIND_FUSED_DOWN / _UP");
  if (ncols < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_multi_launch_bytes: ncols must be >= 1");
  const Level& l = h->lv[level];
  const bool down = kind == AGGMG_KIND_FUSED_DOWN;
  switch (level_path(h, level)) {   // the families of vcycle_multi_group
    case LevelPath::FusedChain:     // (a launch of cgt_multi_kernel, AGGMG_OPT_CHAIN_MULTI)
      return cgt_multi_launch_bytes(ctx, h, level, down, has_x0 != 0, ncols, read_bytes, write_bytes);
    case LevelPath::FusedBtd:
      btd_launch_bytes(*l.S->btd, true, !down || has_x0, down, false, down ? nullptr : l.tb.get(), down ? l.tb.get() : nullptr,
                       restrict_with_ld(h, l), read_bytes, write_bytes, ncols);
      return AGGMG_OK;
    default: break;   // (a patch level: several launches a half -- its sweep launch: aggmg_smoother_launch_bytes)
  }
  return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_hier_multi_launch_bytes: the level has no fused block-tridiagonal launch");
}

extern "C" int aggmg_smoother_launch_bytes(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, int what, int64_t* read_bytes,
                                           int64_t* write_bytes) {
  if (!ctx || !A || !read_bytes || !write_bytes) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_launch_bytes: NULL argument");
  if (what != 0 && what != 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_launch_bytes: what must be 0 (sweeps) or 1 (residual)");
  if (what == 0 && !sm) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_launch_bytes: sweeps need the smoother");
  const int64_t N = A->m, D = sizeof(double);
  if (what == 0 && sm->cgt && sm->A == A) return cgt_op_launch_bytes(*sm->cgt, true, read_bytes, write_bytes);
  if (what == 1 && A->cgt) return cgt_op_launch_bytes(*A->cgt, false, read_bytes, write_bytes);
  if (what == 0 && sm->patch && sm->A == A) {
    // b, u and the new u; per row its 4m inverse-row words, its m entries of D_e and its couplings -- or, with the
    // smoother's dictionary, those of every class once and 2 bytes of class per element
    const int64_t m = sm->patch->m, ne = sm->patch->ne;
    const int64_t rec = m * 4 * m * D + m * m * D + (sm->patch->btd->cmp ? m * D + m * D : 2 * m * m * D);   // per element
    const PatchDictDev* d = sm->patch->dict.get();
    *read_bytes = 2 * N * D + (d ? ne * 2 + (int64_t)d->nclasses * rec : ne * rec);
    *write_bytes = N * D;
    return AGGMG_OK;
  }
  if (what == 0 && sm->btd && sm->A == A) {
    btd_launch_bytes(*sm->btd, true, true, false, false, nullptr, nullptr, false, read_bytes, write_bytes);
    return AGGMG_OK;
  }
  if (what == 1 && A->btd) {
    btd_launch_bytes(*A->btd, false, true, true, true, nullptr, nullptr, false, read_bytes, write_bytes);
    return AGGMG_OK;
  }
  // generic CSR: int32 column indices + fp64 entries + row pointers, the vectors once each
  int64_t r = A->nnz * (4 + D) + (N + 1) * 4 + 2 * N * D;   // entries, row pointers, u and b
  int64_t w = N * D;
  if (what == 0) {
    if (sm->kind == 0) {
      r += N * D;                                             // diagonal
    } else {
      r += sm->nb * sm->m * sm->m * D + sm->nb * sm->m * 4;   // block inverses and their index lists
      if (sm->kind == 2) r += N * D;                          // overlap counts
    }
  }
  *read_bytes = r;
  *write_bytes = w;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_coarse_probe(aggmg_ctx* ctx, const aggmg_hier* h, double* backward_error) {
  if (!ctx || !h || !backward_error) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_coarse_probe: NULL argument");
  *backward_error = h->cr_probe_backward_error;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_coarse_info(aggmg_ctx* ctx, const aggmg_hier* h, int* on_device, int* block_size,
                                      double* cond_est) {
  if (!ctx || !h) return AGGMG_ERR_ARGUMENT;
  if (on_device) *on_device = h->cr.valid ? 1 : 0;
  if (block_size) *block_size = h->cr.valid ? h->cr.m : 0;
  if (cond_est) *cond_est = h->cr.valid ? h->cr.cond_est : 0.0;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_coarse_chain(aggmg_ctx* ctx, const aggmg_hier* h, int* on, int* m, int64_t* blocks) {
  if (!ctx || !h) return AGGMG_ERR_ARGUMENT;
  const bool c = h->cr.valid && h->cr.chain;
  if (on) *on = c ? 1 : 0;
  if (m) *m = c ? h->cr.m : 0;
  if (blocks) *blocks = c ? h->cr.n0 : 0;
  return AGGMG_OK;
}

extern "C" int aggmg_hier_coarse_tail(aggmg_ctx* ctx, const aggmg_hier* h, int* kind, int64_t* blocks) {
  if (!ctx || !h) return AGGMG_ERR_ARGUMENT;
  if (kind) *kind = !h->cr.valid ? 0 : h->cr.pcr.valid ? 2 : 1;
  if (blocks) *blocks = h->cr.valid ? h->cr.tail.n_in : 0;
  return AGGMG_OK;
}

// ---- chunked coarsest solve, phase by phase (multi-GPU driver) --------------------------------
// can the stage-0 chunks of a block range be run alone?  (chain order: the blocks are not ranges of the operator's rows)
static bool cr_chunked_plan(const CrDev& cr) { return cr.valid && !cr.st.empty() && cr.n0 * cr.m == cr.N && !cr.chain; }

extern "C" int aggmg_coarse_plan(aggmg_ctx* ctx, const aggmg_hier* h, int* chunk_log2, int64_t* n_boundary,
                                 int* block_size, int64_t* n_blocks) {
  if (!ctx || !h) return AGGMG_ERR_ARGUMENT;
  const CrDev& cr = h->cr;
  const bool ok = cr_chunked_plan(cr);
  if (chunk_log2) *chunk_log2 = ok ? cr.st[0].q : -1;
  if (n_boundary) *n_boundary = ok ? cr.st[0].n_out : 0;
  if (block_size) *block_size = cr.valid ? cr.m : 0;
  if (n_blocks) *n_blocks = cr.valid ? cr.n0 : 0;
  return AGGMG_OK;
}

static int coarse_phase_check(aggmg_ctx* ctx, aggmg_hier* h, int64_t blk_lo, int64_t blk_hi) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_coarse_*: NULL hierarchy");
  const CrDev& cr = h->cr;
  if (!cr_chunked_plan(cr))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_coarse_*: this hierarchy has no chunked cyclic-reduction plan");
  const int64_t mask = ((int64_t)1 << cr.st[0].q) - 1;
  if (blk_lo < 0 || blk_hi > cr.n0 || blk_lo > blk_hi || (blk_lo & mask) || ((blk_hi & mask) && blk_hi != cr.n0))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_coarse_*: block range must be aligned to the chunk size");
  return AGGMG_OK;
}

extern "C" int aggmg_coarse_chunk_forward_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs_owned,
                                              int64_t blk_lo, int64_t blk_hi, double* partR, double* partL) {
  CHECK(coarse_phase_check(ctx, h, blk_lo, blk_hi));
  if (!rhs_owned || !partR || !partL) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_coarse_chunk_forward_dev: NULL");
  return cr_phase(ctx, h->cr, 0, rhs_owned, blk_lo, blk_hi, partR, partL, nullptr, nullptr);
}

extern "C" int aggmg_coarse_boundary_solve_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* partR,
                                               const double* partL, double* xq) {
  CHECK(coarse_phase_check(ctx, h, 0, 0));
  if (!partR || !partL || !xq) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_coarse_boundary_solve_dev: NULL");
  return cr_phase(ctx, h->cr, 1, nullptr, 0, 0, const_cast<double*>(partR), const_cast<double*>(partL), xq, nullptr);
}

// Element-partitioned driver (dist.hip): the chunk kernels write their boundary rows chunk-interleaved into Z --
// chunk c: Z[c][0..m) = its right-hand terms, Z[c][m..2m) = the terms for chunk c + 1's left end -- so that a rank's
// chunks are ONE contiguous slice and the all-gather of the boundary system runs in place, with no pack or unpack
// launch; the boundary solve reads Z as it lies (block stride 2 m).  Z points one pad block (2 m zeros) into its
// allocation: the left-end terms of chunk 0 do not exist.
int coarse_chunk_forward_interleaved(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs_owned, int64_t blk_lo, int64_t blk_hi,
                                     double* Z) {
  return cr_phase(ctx, h->cr, 0, rhs_owned, blk_lo, blk_hi, Z, Z - h->cr.m, nullptr, nullptr, 2 * h->cr.m);
}

int coarse_boundary_solve_interleaved(aggmg_ctx* ctx, aggmg_hier* h, const double* Z, double* xq) {
  return cr_phase(ctx, h->cr, 1, nullptr, 0, 0, const_cast<double*>(Z), const_cast<double*>(Z) - h->cr.m, xq, nullptr,
                  2 * h->cr.m);
}

extern "C" int aggmg_coarse_chunk_backward_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs_owned,
                                               int64_t blk_lo, int64_t blk_hi, const double* xq, double* x_owned) {
  CHECK(coarse_phase_check(ctx, h, blk_lo, blk_hi));
  if (!rhs_owned || !xq || !x_owned) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_coarse_chunk_backward_dev: NULL");
  return cr_phase(ctx, h->cr, 2, rhs_owned, blk_lo, blk_hi, nullptr, nullptr, xq, x_owned);
}

extern "C" int aggmg_hier_last_coarse_ms(aggmg_ctx* ctx, const aggmg_hier* h, double* ms) {
  if (!ctx || !h || !ms) return AGGMG_ERR_ARGUMENT;
  *ms = h->last_coarse_ms;
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// outer solver loops on the device: multigrid (src/solvers.jl:116-139) and
// iterative_smoother_solve (src/solvers.jl:189-213) without the per-iteration host round trips of
// the iterate, and ldiv! (src/solvers.jl:63-92) as the preconditioner of a conjugate-gradient loop
// ---------------------------------------------------------------------------------------------
static int solv_scalars(aggmg_ctx* ctx) {
  if (!ctx->solv_part) CHECK(ctx->solv_part.alloc(ctx, kDotBlocks));
  if (!ctx->solv_sc) CHECK(ctx->solv_sc.alloc(ctx, kSolvScalars));   // (the names: workspace.hpp)
  return AGGMG_OK;
}

// sc_out[0] = x . y  (or its square root); everything stays on the stream.  `first`: the pass over the vectors --
// diff2_partial_kernel makes it the sum of (x - y)^2
using PartialKernel = void (*)(int64_t, const double*, const double*, double*);
static int dev_dot(aggmg_ctx* ctx, int64_t n, const double* x, const double* y, double* sc_out, int take_sqrt,
                   PartialKernel first = dot_partial_kernel) {
  CHECK(solv_scalars(ctx));
  hipLaunchKernelGGL(first, dim3(kDotBlocks), dim3(kThreads), 0, ctx->stream, n, x, y, (double*)ctx->solv_part);
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, kDotBlocks,
                     (const double*)ctx->solv_part, sc_out, take_sqrt);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int read_scalar(aggmg_ctx* ctx, const double* sc, double* out) {
  HIPCHK(hipMemcpyAsync(out, sc, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

// reduce, then read back at once: *host_out = x . y (or its square root) when this returns.  Every such value passes
// through the one scalar kScReadBack; it is on the host before anything else can touch the slot.
static int reduce_read(aggmg_ctx* ctx, int64_t n, const double* x, const double* y, int take_sqrt, double* host_out,
                       PartialKernel first = dot_partial_kernel) {
  CHECK(solv_scalars(ctx));
  double* sc = ctx->solv_sc + kScReadBack.at;
  CHECK(dev_dot(ctx, n, x, y, sc, take_sqrt, first));
  return read_scalar(ctx, sc, host_out);
}

extern "C" int aggmg_dot_dev(aggmg_ctx* ctx, const double* x, const double* y, int64_t n, double* out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!x || !y || !out || n < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_dot_dev: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  return reduce_read(ctx, n, x, y, 0, out);
}

extern "C" int aggmg_norm2_dev(aggmg_ctx* ctx, const double* x, int64_t n, double* out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!x || !out || n < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_norm2_dev: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  return reduce_read(ctx, n, x, x, 1, out);
}

// EXTENSION (no reference counterpart): power iteration for the largest eigenvalue of S^-1 A of a level, what a
// Chebyshev sweep-weight schedule is scaled by.  One step: t = A v (the residual launch on a zero right-hand side: -A v,
// the sign changes no norm), w = S^-1 t (one sweep of the level's smoother with factor 1 from the zero iterate), then
// ||w|| and v = w / ||w|| on the stream.  The estimate is ||w|| / ||v|| of the last step: one host read, at the end.
extern "C" int aggmg_hier_estimate_lambda_max(aggmg_ctx* ctx, aggmg_hier* h, int level, const double* v0, int iters,
                                              double* lambda_max) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !lambda_max) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_estimate_lambda_max: NULL argument");
  if (level < 0 || level >= (int)h->lv.size() - 1)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_estimate_lambda_max: level out of range (the coarsest level has no smoother)");
  if (iters < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_hier_estimate_lambda_max: iters must be >= 1");
  HIPCHK(hipSetDevice(ctx->device));
  Level& l = h->lv[level];
  const int64_t N = l.N;
  if (N == 0) {
    *lambda_max = 0.0;
    return AGGMG_OK;
  }
  CHECK(solv_scalars(ctx));
  // work vectors of THIS call (allocated and freed per call: the estimate is made once per hierarchy, not per cycle): the
  // iterate, A v, S^-1 A v, and the zero right-hand side that turns the residual launch into -A v
  DevArray<double> v, t, w, zero;
  CHECK(v.alloc(ctx, N));
  CHECK(t.alloc(ctx, N));
  CHECK(w.alloc(ctx, N));
  CHECK(zero.alloc(ctx, N, true));
  const unsigned nb = (unsigned)((N + kThreads - 1) / kThreads);
  if (v0) {
    HIPCHK(hipMemcpyAsync(v, v0, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  } else {   // a fixed start, made on the device
    hipLaunchKernelGGL(seed_vector_kernel, dim3(nb), dim3(kThreads), 0, ctx->stream, N, (double*)v);
    HIPCHK(hipGetLastError());
  }
  double* sc = ctx->solv_sc + kScLambda.at;   // [0] ||w||, [1] ||v|| of the last step
  for (int it = 0; it < iters; ++it) {
    CHECK(aggmg_residual_dev(ctx, l.A, v, zero, t));
    CHECK(smooth_dev(ctx, l.A, l.S, nullptr, t, Damping(1.0), 1, w));
    if (it == iters - 1) CHECK(dev_dot(ctx, N, v, v, sc + 1, 1));
    CHECK(dev_dot(ctx, N, w, w, sc, 1));
    hipLaunchKernelGGL(div_scalar_kernel, dim3(nb), dim3(kThreads), 0, ctx->stream, N, (const double*)w, (const double*)sc,
                       (double*)v);
    HIPCHK(hipGetLastError());
  }
  double out[2] = {0.0, 0.0};
  HIPCHK(hipMemcpyAsync(out, sc, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *lambda_max = out[1] > 0.0 ? out[0] / out[1] : 0.0;
  return AGGMG_OK;
}

// ||b - A x||_2 on the device
static int residual_norm(aggmg_ctx* ctx, aggmg_op* A, const double* x, const double* b, double* out) {
  WorkLease r;
  CHECK(solv_lease(ctx, kSolvR, A->m, "residual_norm", &r));
  CHECK(aggmg_residual_dev(ctx, A, x, b, r));
  return reduce_read(ctx, A->m, r, r, 1, out);
}

// ||x - y||_2 on the device: one entry of the `err` history (src/solvers.jl:128, :202)
static int diff_norm(aggmg_ctx* ctx, int64_t n, const double* x, const double* y, double* out) {
  return reduce_read(ctx, n, x, y, 1, out, diff2_partial_kernel);
}

extern "C" int aggmg_residual_norm_dev(aggmg_ctx* ctx, aggmg_op* A, const double* x, const double* b, double* out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!A || !x || !b || !out) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual_norm_dev: NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  return residual_norm(ctx, A, x, b, out);
}

// norms of the checkpoints of a launch: part[nchk][ntiles][2] -> out[nchk][2] (chk_reduce1/2_kernel); `mid`: room for
// nchk * kChkReduceGroups * 2 doubles
static int chk_reduce(aggmg_ctx* ctx, int nchk, int64_t ntiles, const double* part, double* mid, double* out) {
  const int G = (int)std::min<int64_t>(kChkReduceGroups, std::max<int64_t>(1, (ntiles + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(chk_reduce1_kernel, dim3((unsigned)G, (unsigned)nchk), dim3(kThreads), 0, ctx->stream, ntiles, part, mid);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(chk_reduce2_kernel, dim3((unsigned)nchk), dim3(kThreads), 0, ctx->stream, G, (const double*)mid, out);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// room for launches of up to nchk_max checkpoints over at most `tiles` tiles; sc: where their norms go
static int chk_buffers(aggmg_ctx* ctx, int nchk_max, int64_t tiles, ScalarRange sc, ChkHist* H) {
  if (2 * nchk_max > sc.n) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: more checkpoints than their scalars hold");
  const int64_t npart = (int64_t)nchk_max * 2 * tiles;
  CHECK(solv_lease(ctx, kSolvP, npart + (int64_t)nchk_max * 2 * kChkReduceGroups, "chk_buffers", &H->hold));
  H->part = H->hold;
  H->mid = H->part + npart;
  H->cap = tiles;
  H->sc = ctx->solv_sc + sc.at;
  return AGGMG_OK;
}

// The nchk (<= kChkMax) checkpoints of a launch, in order, into the histories up to the first one that meets the
// tolerance: *met is its index, or -1.
static int chk_collect(aggmg_ctx* ctx, ChkHist& H, int nchk, int64_t ntiles, int* met) {
  CHECK(chk_reduce(ctx, nchk, ntiles, H.part, H.mid, H.sc));
  double host[2 * kChkMax];   // per checkpoint: ||A x - b||, ||x - u_exact||
  HIPCHK(hipMemcpyAsync(host, H.sc, (size_t)2 * nchk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *met = -1;
  for (int k = 0; k < nchk && *met < 0; ++k) {
    if (H.u_exact) H.err[H.checks] = host[2 * k + 1];   // err[i] = ||x - u_exact||, src/solvers.jl:128, :202
    H.res[H.checks++] = host[2 * k];                    // res[i] = ||A x - b||,      :127, :201
    if (host[2 * k] < H.tol_nb) *met = k;               // :131, :206
  }
  return AGGMG_OK;
}

// A run of multigrid() (src/solvers.jl:116-139) or iterative_smoother_solve (:189-213) on the device: `maxiter` steps
// from x0 into x_out, the residual test (and the error norm) after every check_every-th one.  What the two entry points
// share is written here once; their fused paths, which form the checks inside their launches, stay with them.
struct CheckedRun {
  aggmg_ctx* ctx;
  aggmg_op* A;
  const double *x0, *b;
  double* x_out;
  int maxiter;
  double tol;
  int check_every;
  const double* u_exact;
  double *res_hist, *err_hist;
  int *n_done, *n_checks;
  int64_t N = 0;
  double tol_nb = 0.0;   // tol ||b||
  WorkLease alt;         // the iterate ping-pongs between x_out and this vector (a step wants distinct input and output)

  // the arguments (who: the entry point, as its messages name it), ||b||, the alternate iterate; *returned: maxiter == 0,
  // the reference returns its initial `x = zeros(length(x0))` (src/solvers.jl:119, :192)
  int begin(const char* who, bool* returned) {
    const std::string w(who);
    if (!x_out || !res_hist || !n_done || !n_checks || maxiter < 0 || check_every < 1)
      return fail(ctx, AGGMG_ERR_ARGUMENT, w + ": bad argument");
    if (x_out == x0 || x_out == b) return fail(ctx, AGGMG_ERR_ARGUMENT, w + ": x_out must not alias x0 or b");
    if ((u_exact == nullptr) != (err_hist == nullptr))
      return fail(ctx, AGGMG_ERR_ARGUMENT, w + ": u_exact and err_hist come together (or both NULL)");
    HIPCHK(hipSetDevice(ctx->device));
    N = A->m;
    double nb = 0.0;
    CHECK(reduce_read(ctx, N, b, b, 1, &nb));
    tol_nb = tol * nb;
    CHECK(solv_lease(ctx, kSolvZ, N, who, &alt));
    *n_done = 0;
    *n_checks = 0;
    *returned = maxiter == 0;
    if (*returned) {
      HIPCHK(hipMemsetAsync(x_out, 0, N * sizeof(double), ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return AGGMG_OK;
  }
  // histories and stopping test of a fused path's checkpoints
  void fill(ChkHist* H) const {
    H->u_exact = u_exact;
    H->tol_nb = tol_nb;
    H->res = res_hist;
    H->err = err_hist;
  }
  // the result is in `cur`: into x_out, and the counts
  int end(const double* cur, int done, int checks) {
    if (cur != x_out) HIPCHK(hipMemcpyAsync(x_out, cur, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *n_done = done;
    *n_checks = checks;
    return AGGMG_OK;
  }
  // the unfused loop: step(src, k, dst) takes k steps; then the norms on the device, the histories, the test
  template <class Step>
  int loop(Step&& step) {
    const double* cur = x0;
    int done = 0, checks = 0;
    while (done < maxiter) {
      const int k = std::min(check_every, maxiter - done);
      double* dst = (cur == x_out) ? alt.get() : x_out;
      CHECK(step(cur, k, dst));
      cur = dst;
      done += k;
      double res = 0.0;
      if (u_exact) CHECK(diff_norm(ctx, N, cur, u_exact, &err_hist[checks]));  // err[i] = ||x - u_exact||, src/solvers.jl:128, :202
      CHECK(residual_norm(ctx, A, cur, b, &res));
      res_hist[checks++] = res;
      if (res < tol_nb) break;  // src/solvers.jl:131, :206
    }
    return end(cur, done, checks);
  }
};

extern "C" int aggmg_multigrid_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* x0, const double* b, int maxiter,
                                   double tol, int check_every, int nPre, int nPost, double alpha, double* x_out,
                                   double* res_hist, int* n_cycles, int* n_checks, const double* u_exact,
                                   double* err_hist) {
  CHECK(vcycle_args(ctx, h, x0, b, nPre, nPost));
  CheckedRun R{ctx, h->lv[0].A, x0, b, x_out, maxiter, tol, check_every, u_exact, res_hist, err_hist, n_cycles, n_checks};
  bool returned = false;
  CHECK(R.begin("aggmg_multigrid_dev", &returned));
  if (returned) return AGGMG_OK;
  // Fused block-tridiagonal fine level: the residual test (and the error norm) of a checked cycle are formed INSIDE the
  // fine-level launch that post-smooths it -- the launch that goes on to pre-smooth the next cycle (aggmg_vcycles_dev's
  // cross-cycle fusion) -- so a check after every cycle, the reference's semantics (src/solvers.jl:124-131), costs a
  // store of the iterate and a few reductions instead of a residual launch over the fine operator and a cycle without
  // the cross-cycle fusion (AGGMG_OPT_MG_CHECKPOINT = 0: the form below, for A/B runs and tests).
  // The CG chain fine level (point-Jacobi): the same loop with the chain kernel's checkpoint variant.
  if (ctx->mg_checkpoint && fine_mid_ok(h, nPre, nPost, MidFor::Checkpointed)) {
    const FineLevel f{ctx, h, b, nPre, nPost, alpha};
    ChkHist H;
    CHECK(chk_buffers(ctx, 1, f.chk_tiles(), kScMgChk, &H));
    R.fill(&H);
    int done = 0;
    CHECK(cycle_loop(f, x0, maxiter, x_out, check_every, &H, &done));
    return R.end(x_out, done, H.checks);
  }
  return R.loop([&](const double* src, int k, double* dst) { return aggmg_vcycles_dev(ctx, h, src, b, k, nPre, nPost, alpha, dst); });
}

extern "C" int aggmg_smoother_solve_dev(aggmg_ctx* ctx, aggmg_op* A, aggmg_smoother* sm, const double* x0,
                                        const double* b, int maxiter, double tol, double alpha, int check_every,
                                        double* x_out, double* res_hist, int* n_iters, int* n_checks,
                                        const double* u_exact, double* err_hist) {
  CHECK(check_pair(ctx, A, sm, "aggmg_smoother_solve_dev"));
  if (!x0 || !b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_smoother_solve_dev: bad argument");   // (a sweep has no zero guess)
  CheckedRun R{ctx, A, x0, b, x_out, maxiter, tol, check_every, u_exact, res_hist, err_hist, n_iters, n_checks};
  bool returned = false;
  CHECK(R.begin("aggmg_smoother_solve_dev", &returned));
  if (returned) return AGGMG_OK;
  const int64_t N = R.N;
  // Fused block-tridiagonal smoother on its own operator: launches of up to S sweeps with the residual test (and the error
  // norm) of every checked sweep formed INSIDE the launch (the checkpoint variant of the fused kernel, as
  // aggmg_multigrid_dev) -- the reference's test after every sweep (src/solvers.jl:198-206) at the multi-sweep smoother's
  // traffic instead of a sweep launch, a residual launch and a reduction per iteration.  A launch whose histories show
  // the tolerance met after j < S sweeps is run again for j sweeps from the same iterate (the same arithmetic: the
  // iterate the reference stops with, bit for bit).  AGGMG_OPT_MG_CHECKPOINT = 0: the form below.
  // Point-Jacobi on a CG chain: the same with the chain kernel.
  const bool fused = ctx->mg_checkpoint && sm->btd && sm->A == A && !sm->gs && btd_max_sweeps(*sm->btd, 1) >= 1 && maxiter > 0;
  const bool chain = !fused && ctx->mg_checkpoint && sm->cgt && sm->A == A && sm->cgt->sw == 0 && cgt_max_fused_sweeps(*sm->cgt) >= 2;
  if (fused || chain) {
    // (one less than a launch takes: the residual rows of the last sweep's iterate)
    const int smax = std::min(fused ? btd_max_sweeps(*sm->btd, 1) : cgt_max_fused_sweeps(*sm->cgt) - 1, kChkMax);
    ChkHist H;
    CHECK(chk_buffers(ctx, smax, fused ? btd_chk_tiles(*sm->btd, smax, nullptr) : cgt_chk_tiles(*sm->cgt, smax, 1), kScSmChk, &H));
    R.fill(&H);
    const double* cur = x0;
    int done = 0;
    // S sweeps src -> dst in one launch; chk: with its checkpoints
    auto sweeps = [&](const double* src, double* dst, int S, CgtChk* chk) -> int {
      return chain ? cgt_smooth_ext(ctx, *sm->cgt, src, b, alpha, S, dst, 0, chk)
                   : btd_smooth(ctx, *sm->btd, src, b, alpha, S, dst, 0, N, 0, chk);
    };
    while (done < maxiter) {
      const int S = std::min(smax, maxiter - done);
      double* dst = (cur == x_out) ? R.alt.get() : x_out;
      // checked iteration counts in (done, done + S]: multiples of check_every, and maxiter
      CgtChk chk;
      chk.sweep = check_every - done % check_every;   // sweeps of this launch before its first check
      chk.stride = check_every;
      chk.final = (done + S == maxiter && (done + S) % check_every != 0) ? 1 : 0;
      chk.exact = u_exact;
      chk.part = H.part;
      chk.cap = H.cap;
      const int nchk = (chk.sweep <= S ? 1 + (S - chk.sweep) / check_every : 0) + chk.final;
      CHECK(sweeps(cur, dst, S, nchk ? &chk : nullptr));
      int met = -1;
      if (nchk) CHECK(chk_collect(ctx, H, nchk, chk.ntiles, &met));
      // sweeps of this launch after which the tolerance was met
      const int stop = met < 0 ? -1 : ((chk.final && met == nchk - 1) ? S : chk.sweep + met * check_every);
      if (stop >= 0 && stop < S) {   // met before the launch's last sweep: that iterate again, without the rest
        CHECK(sweeps(cur, dst, stop, nullptr));
        done += stop;
      } else {
        done += S;
      }
      cur = dst;
      if (stop >= 0) break;
    }
    return R.end(cur, done, H.checks);
  }
  // k x (x += alpha S (b - A x)), src/solvers.jl:200
  return R.loop([&](const double* src, int k, double* dst) { return aggmg_smooth_dev(ctx, A, sm, src, b, alpha, k, dst); });
}

// Conjugate gradients on A x = b preconditioned by one V-cycle from a zero guess, i.e. by
// ldiv!(y, H, r) (src/solvers.jl:84-92).  Needs a symmetric positive definite A and a symmetric
// cycle (nPre == nPost, block-Jacobi / Jacobi smoothers, L' restriction): true for every hierarchy
// the reference builds.  Extension: the reference stops at ldiv!, it has no Krylov loop.
extern "C" int aggmg_pcg_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, double* x_inout, int maxiter, double tol,
                             int nPre, int nPost, double alpha, double* res_hist, int* n_iters) {
  CHECK(vcycle_args(ctx, h, x_inout, b, nPre, nPost));
  if (!res_hist || !n_iters || maxiter < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_pcg_dev: bad argument");
  if (x_inout == b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_pcg_dev: x must not alias b");
  if (h->coarse_mode == AGGMG_COARSE_EXTERNAL)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_pcg_dev: hierarchy was created with AGGMG_COARSE_EXTERNAL");
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(solv_scalars(ctx));
  aggmg_op* A = h->lv[0].A;
  const int64_t N = A->m;
  WorkLease vec[kSolvSlots];
  for (int s = 0; s < kSolvSlots; ++s) CHECK(solv_lease(ctx, (SolvSlot)s, N, "aggmg_pcg_dev", &vec[s]));
  double *r = vec[kSolvR], *z = vec[kSolvZ], *pv = vec[kSolvP], *q = vec[kSolvQ], *zero = vec[kSolvZero];
  HIPCHK(hipMemsetAsync(zero, 0, N * sizeof(double), ctx->stream));
  double* sc = ctx->solv_sc + kScPcg.at;  // [0] rz  [1] p.q  [2] rz_new
  const unsigned grid = (unsigned)((N + kThreads - 1) / kThreads);
  double nb = 0.0, res = 0.0;
  CHECK(reduce_read(ctx, N, b, b, 1, &nb));
  *n_iters = 0;
  CHECK(aggmg_residual_dev(ctx, A, x_inout, b, r));                       // r = b - A x
  CHECK(aggmg_vcycle_dev(ctx, h, nullptr, r, nPre, nPost, alpha, z));     // z = M^-1 r  (ldiv!: zero initial guess)
  HIPCHK(hipMemcpyAsync(pv, z, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  CHECK(dev_dot(ctx, N, r, z, sc + 0, 0));
  for (int it = 0; it < maxiter; ++it) {
    CHECK(aggmg_residual_dev(ctx, A, pv, zero, q));                       // q = -A p
    CHECK(dev_dot(ctx, N, pv, q, sc + 1, 0));
    hipLaunchKernelGGL(pcg_xr_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, N, x_inout, r, (const double*)pv,
                       (const double*)q, (const double*)(sc + 0), (const double*)(sc + 1));
    CHECK(reduce_read(ctx, N, r, r, 1, &res));
    res_hist[it] = res;
    *n_iters = it + 1;
    if (res < tol * nb) break;
    CHECK(aggmg_vcycle_dev(ctx, h, nullptr, r, nPre, nPost, alpha, z));
    CHECK(dev_dot(ctx, N, r, z, sc + 2, 0));
    hipLaunchKernelGGL(pcg_p_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, N, pv, (const double*)z,
                       (const double*)(sc + 2), (const double*)(sc + 0));
    HIPCHK(hipMemcpyAsync(sc + 0, sc + 2, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// K right-hand sides through the outer loops (EXTENSION: the reference's solvers take vectors,
// src/solvers.jl:116-139; every column keeps the single-vector entry point's arithmetic and bits)
// ---------------------------------------------------------------------------------------------
// launches with the columns in blockIdx.y: f(c0, kc) for every chunk [c0, c0 + kc) of K columns that a grid holds
template <class F>
static void for_col_chunks(int64_t K, F&& f) {
  constexpr int64_t kColsGridMax = 65535;
  for (int64_t c0 = 0; c0 < K; c0 += kColsGridMax) f(c0, (unsigned)std::min<int64_t>(kColsGridMax, K - c0));
}

static int cols_scalars(aggmg_ctx* ctx, int64_t K) {
  CHECK(solv_scalars(ctx));
  if (ctx->cols_cap >= K) return AGGMG_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->cols_cap = 0;
  CHECK(ctx->cols_part.alloc(ctx, K * kDotBlocks));
  CHECK(ctx->cols_sc.alloc(ctx, K * kColsScalars));
  CHECK(ctx->cols_map.alloc(ctx, K));
  ctx->cols_cap = K;
  return AGGMG_OK;
}
static double* cols_sc(aggmg_ctx* ctx, ColsScalar which) { return ctx->cols_sc + (int64_t)which * ctx->cols_cap; }

// out[c] = X[:, c] . Y[:, c] (or its square root), c < K <= cols_cap; everything stays on the stream
static int dev_dot_cols(aggmg_ctx* ctx, int64_t n, int64_t K, const double* x, int64_t ldx, const double* y, int64_t ldy,
                        double* out, int take_sqrt) {
  for_col_chunks(K, [&](int64_t c0, unsigned kc) {
    hipLaunchKernelGGL(dot_cols_partial_kernel, dim3(kDotBlocks, kc), dim3(kThreads), 0, ctx->stream, n, x + c0 * ldx, ldx,
                       y + c0 * ldy, ldy, ctx->cols_part + c0 * kDotBlocks);
    hipLaunchKernelGGL(dot_cols_final_kernel, dim3(kc), dim3(kThreads), 0, ctx->stream, kDotBlocks,
                       (const double*)(ctx->cols_part + c0 * kDotBlocks), out + c0, take_sqrt);
  });
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}
// out[c] = ||X[:, c] - Y[:, ycol ? ycol[c] : c]||_2
static int dev_diff_cols(aggmg_ctx* ctx, int64_t n, int64_t K, const double* x, int64_t ldx, const double* y, int64_t ldy,
                         const int* ycol, double* out) {
  for_col_chunks(K, [&](int64_t c0, unsigned kc) {
    hipLaunchKernelGGL(diff2_cols_partial_kernel, dim3(kDotBlocks, kc), dim3(kThreads), 0, ctx->stream, n, x + c0 * ldx, ldx,
                       ycol ? y : y + c0 * ldy, ldy, ycol ? ycol + c0 : nullptr, ctx->cols_part + c0 * kDotBlocks);
    hipLaunchKernelGGL(dot_cols_final_kernel, dim3(kc), dim3(kThreads), 0, ctx->stream, kDotBlocks,
                       (const double*)(ctx->cols_part + c0 * kDotBlocks), out + c0, 1);
  });
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int read_scalars(aggmg_ctx* ctx, const double* sc, int64_t K, double* out) {
  HIPCHK(hipMemcpyAsync(out, sc, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

static int dot_cols_entry(aggmg_ctx* ctx, const char* who, const double* X, const double* Y, int64_t n, int64_t ncols, int64_t ld,
                          double* out, int take_sqrt) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!X || !Y || !out) return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": NULL argument");
  if (n < 0 || ncols < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": needs n >= 0 and ncols >= 1");
  if (ld < n) return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": ld must be >= n");
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(cols_scalars(ctx, ncols));
  CHECK(dev_dot_cols(ctx, n, ncols, X, ld, Y, ld, cols_sc(ctx, kColRes), take_sqrt));
  return read_scalars(ctx, cols_sc(ctx, kColRes), ncols, out);
}
extern "C" int aggmg_dot_cols_dev(aggmg_ctx* ctx, const double* X, const double* Y, int64_t n, int64_t ncols, int64_t ld,
                                  double* out_host) {
  return dot_cols_entry(ctx, "aggmg_dot_cols_dev", X, Y, n, ncols, ld, out_host, 0);
}
extern "C" int aggmg_norm2_cols_dev(aggmg_ctx* ctx, const double* X, int64_t n, int64_t ncols, int64_t ld, double* out_host) {
  return dot_cols_entry(ctx, "aggmg_norm2_cols_dev", X, X, n, ncols, ld, out_host, 1);
}

// ---------------------------------------------------------------------------------------------
// Flexible GMRES around the cycle (EXTENSION: the reference has no Krylov loop).  Conjugate gradients above need a
// symmetric cycle; a minimal-residual method is valid for every cycle -- nPre != nPost, sweep-weight schedules whose
// post half is not the pre half reversed, hybrid Schwarz and Gauss-Seidel levels -- and for a preconditioner that
// changes from one application to the next.  The two streaming passes of its orthogonalisation are
// krylov_kernels.hpp, the small dense part is host_gmres.hpp.
// ---------------------------------------------------------------------------------------------
constexpr int64_t kKryMaxVec = AGGMG_FGMRES_MAX_RESTART + 1;
// device scalars of the Krylov passes: [0 .. 65] the dots of a pass and, behind them, the norm of the update;
// [kKryCoef .. + 64] coefficients that came from the host; [kKryBeta] ||r|| of a restart
constexpr int kKryCoef = 128, kKryBeta = 200, kKryScalars = 256;
static_assert(HostGmres::kMaxRestart == AGGMG_FGMRES_MAX_RESTART, "host_gmres.hpp and the header disagree");

static int kry_scalars(aggmg_ctx* ctx) {
  CHECK(solv_scalars(ctx));
  if (!ctx->kry_part) CHECK(ctx->kry_part.alloc(ctx, (kKryMaxVec + 1) * kDotBlocks));
  if (!ctx->kry_sc) CHECK(ctx->kry_sc.alloc(ctx, kKryScalars, true));
  return AGGMG_OK;
}

template <int G>
static void launch_multi_dot(aggmg_ctx* ctx, int64_t n, const double* V, int64_t ld, const double* w, double* part) {
  hipLaunchKernelGGL(multi_dot_partial_kernel<G>, dim3(kDotBlocks), dim3(kThreads), 0, ctx->stream, n, V, ld, w, part);
}
template <int G>
static void launch_multi_axpy(aggmg_ctx* ctx, int64_t n, const double* V, int64_t ld, const double* coef, double scale,
                              double* w, double* part) {
  if (part)
    hipLaunchKernelGGL((multi_axpy_kernel<G, true>), dim3(kDotBlocks), dim3(kThreads), 0, ctx->stream, n, V, ld, coef, scale, w,
                       part);
  else
    hipLaunchKernelGGL((multi_axpy_kernel<G, false>), dim3(kDotBlocks), dim3(kThreads), 0, ctx->stream, n, V, ld, coef, scale, w,
                       part);
}
#define KRY_GROUP_SWITCH(g, CALL) \
  switch (g) {                    \
    case 1: CALL(1); break;       \
    case 2: CALL(2); break;       \
    case 3: CALL(3); break;       \
    case 4: CALL(4); break;       \
    case 5: CALL(5); break;       \
    case 6: CALL(6); break;       \
    case 7: CALL(7); break;       \
    default: CALL(8); break;      \
  }

// out[i] = V_i . w, i < nvec <= kKryMaxVec (out on the device): one pass over w per group of 8 vectors, then one
// workgroup per dot; everything stays on the stream
static int dev_multi_dot(aggmg_ctx* ctx, int64_t n, int64_t nvec, const double* V, int64_t ld, const double* w, double* out) {
  for (int64_t i0 = 0; i0 < nvec; i0 += kKrylovGroup) {
    const int g = (int)std::min<int64_t>(kKrylovGroup, nvec - i0);
#define KRY_CALL(G) launch_multi_dot<G>(ctx, n, V + i0 * ld, ld, w, ctx->kry_part + i0 * kDotBlocks)
    KRY_GROUP_SWITCH(g, KRY_CALL)
#undef KRY_CALL
  }
  hipLaunchKernelGGL(dot_cols_final_kernel, dim3((unsigned)nvec), dim3(kThreads), 0, ctx->stream, kDotBlocks,
                     (const double*)ctx->kry_part, out, 0);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// w += V (scale coef), coef[0 .. nvec - 1] on the device, in groups of 8 (ascending); norm_out (device, or null)
// receives ||w||_2 of the stored vector, summed by the pass of the last group
static int dev_multi_axpy(aggmg_ctx* ctx, int64_t n, int64_t nvec, const double* V, int64_t ld, const double* coef, double scale,
                          double* w, double* norm_out) {
  double* part = ctx->kry_part + kKryMaxVec * kDotBlocks;
  for (int64_t i0 = 0; i0 < nvec; i0 += kKrylovGroup) {
    const int g = (int)std::min<int64_t>(kKrylovGroup, nvec - i0);
    double* p = (norm_out && i0 + g == nvec) ? part : nullptr;
#define KRY_CALL(G) launch_multi_axpy<G>(ctx, n, V + i0 * ld, ld, coef + i0, scale, w, p)
    KRY_GROUP_SWITCH(g, KRY_CALL)
#undef KRY_CALL
  }
  if (norm_out)
    hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, kDotBlocks, (const double*)part, norm_out, 1);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int kry_args(aggmg_ctx* ctx, const char* who, const double* V, int64_t n, int64_t nvec, int64_t ld, const double* w,
                    const void* host) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!V || !w || !host) return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": NULL argument");
  if (n < 0 || nvec < 1 || nvec > kKryMaxVec)
    return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": needs n >= 0 and 1 <= nvec <= " + std::to_string(kKryMaxVec));
  if (ld < n) return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": ld must be >= n");
  return AGGMG_OK;
}

extern "C" int aggmg_multi_dot_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ld, const double* w,
                                   double* out_host) {
  CHECK(kry_args(ctx, "aggmg_multi_dot_dev", V, n, nvec, ld, w, out_host));
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(kry_scalars(ctx));
  CHECK(dev_multi_dot(ctx, n, nvec, V, ld, w, ctx->kry_sc));
  return read_scalars(ctx, ctx->kry_sc, nvec, out_host);
}

extern "C" int aggmg_multi_axpy_norm_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ld,
                                         const double* coef_host, double* w_inout, double* norm_out_host) {
  CHECK(kry_args(ctx, "aggmg_multi_axpy_norm_dev", V, n, nvec, ld, w_inout, coef_host));
  if (ranges_overlap(V, (nvec - 1) * ld + n, w_inout, n))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_multi_axpy_norm_dev: w must not overlap V");
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(kry_scalars(ctx));
  double* coef = ctx->kry_sc + kKryCoef;
  HIPCHK(hipMemcpyAsync(coef, coef_host, (size_t)nvec * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  CHECK(dev_multi_axpy(ctx, n, nvec, V, ld, coef, 1.0, w_inout, norm_out_host ? ctx->kry_sc.get() : nullptr));
  if (norm_out_host) return read_scalar(ctx, ctx->kry_sc, norm_out_host);
  HIPCHK(hipStreamSynchronize(ctx->stream));   // (coef_host has been read when this returns)
  return AGGMG_OK;
}

// Right-preconditioned flexible GMRES(restart), classical Gram-Schmidt in one pass: per iteration one cycle
// z_j = M^-1 v_j, one operator product, the fused dots h = V' w, the fused update w -= V h that also yields
// h_{j+1,j} = ||w||, one read-back of the column, v_{j+1} = w / h_{j+1,j}.  The operator product is the residual launch
// on a zero right-hand side, w = -A z_j (as in aggmg_pcg_dev): the Arnoldi relation is therefore kept for -A,
// (-A) Z = V Hbar, the least-squares problem min || beta e_1 - Hbar y || is the usual one, and the correction enters
// with the other sign: x -= Z y gives r_new = r - (-A Z) y = V (beta e_1 - Hbar y).  Every sign change is exact, so
// the history is what the recurrence on +A gives.
extern "C" int aggmg_fgmres_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* b, double* x_inout, int restart, int maxiter,
                                double tol, int nPre, int nPost, double alpha, double* res_hist, int* n_iters) {
  CHECK(vcycle_args(ctx, h, x_inout, b, nPre, nPost));
  if (!res_hist || !n_iters || maxiter < 0) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_fgmres_dev: bad argument");
  if (restart < 1 || restart > AGGMG_FGMRES_MAX_RESTART)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_fgmres_dev: restart must be 1 .. " + std::to_string(AGGMG_FGMRES_MAX_RESTART));
  if (x_inout == b) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_fgmres_dev: x must not alias b");
  if (h->coarse_mode == AGGMG_COARSE_EXTERNAL)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_fgmres_dev: hierarchy was created with AGGMG_COARSE_EXTERNAL");
  CHECK(schedule_check(ctx, h, nPre, nPost));
  HIPCHK(hipSetDevice(ctx->device));
  *n_iters = 0;
  if (maxiter == 0) return AGGMG_OK;
  CHECK(kry_scalars(ctx));
  aggmg_op* A = h->lv[0].A;
  const int64_t N = A->m;
  // work space: V (restart + 1 vectors), Z (restart), and w, which holds r between the cycles; kept for the next call
  // of the same size, exchanged for another size
  const int64_t need = (2 * (int64_t)restart + 2) * N;
  if (ctx->kry_work.size() != need || !ctx->kry_work) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    (void)ctx->kry_work.reset(ctx);
    if (int st = ctx->kry_work.alloc(ctx, need))
      return fail(ctx, st, "aggmg_fgmres_dev: no device memory for the work space of " + std::to_string(need * 8) +
                               " bytes (restart " + std::to_string(restart) + ", " + std::to_string(2 * restart + 2) +
                               " vectors of " + std::to_string(N) + "): " + ctx->err);
  }
  double* V = ctx->kry_work;
  double* Z = V + ((int64_t)restart + 1) * N;
  double* w = Z + (int64_t)restart * N;
  WorkLease zero;
  CHECK(solv_lease(ctx, kSolvZero, N, "aggmg_fgmres_dev", &zero));
  HIPCHK(hipMemsetAsync(zero, 0, N * sizeof(double), ctx->stream));
  double* sc = ctx->kry_sc;
  const unsigned grid = (unsigned)((N + kThreads - 1) / kThreads);
  double nb = 0.0;
  CHECK(reduce_read(ctx, N, b, b, 1, &nb));
  HostGmres ls;
  double col[AGGMG_FGMRES_MAX_RESTART + 2], y[AGGMG_FGMRES_MAX_RESTART];
  int it = 0;
  bool done = false;
  while (!done && it < maxiter) {
    double beta = 0.0;
    CHECK(aggmg_residual_dev(ctx, A, x_inout, b, w));                      // every cycle starts from r = b - A x
    CHECK(dev_dot(ctx, N, w, w, sc + kKryBeta, 1));
    CHECK(read_scalar(ctx, sc + kKryBeta, &beta));
    if (beta == 0.0 || beta < tol * nb || !std::isfinite(beta)) break;     // (at entry: x untouched, n_iters = 0)
    hipLaunchKernelGGL(div_scalar_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, N, (const double*)w,
                       (const double*)(sc + kKryBeta), V);                // v_0 = r / beta
    ls.start(beta);
    const int len = std::min(restart, maxiter - it);
    bool finite = true;
    for (int j = 0; j < len; ++j) {
      double* zj = Z + (int64_t)j * N;
      CHECK(aggmg_vcycle_dev(ctx, h, nullptr, V + (int64_t)j * N, nPre, nPost, alpha, zj));   // z_j = M^-1 v_j
      CHECK(aggmg_residual_dev(ctx, A, zj, zero, w));                                          // w = -A z_j
      CHECK(dev_multi_dot(ctx, N, j + 1, V, N, w, sc));                                        // h = V' w
      CHECK(dev_multi_axpy(ctx, N, j + 1, V, N, sc, -1.0, w, sc + j + 1));                     // w -= V h; ||w||
      CHECK(read_scalars(ctx, sc, j + 2, col));
      const double res = ls.push(col);
      res_hist[it++] = res;
      *n_iters = it;
      if (!std::isfinite(res)) {
        finite = false;
        done = true;
        break;
      }
      if (res < tol * nb || col[j + 1] == 0.0) {   // converged, or the Krylov space is exhausted (no division by 0)
        done = true;
        break;
      }
      if (j + 1 < len)
        hipLaunchKernelGGL(div_scalar_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, N, (const double*)w,
                           (const double*)(sc + j + 1), V + (int64_t)(j + 1) * N);
    }
    if (!finite) break;   // (x keeps the value of the last finished cycle)
    ls.solve(y);
    HIPCHK(hipMemcpyAsync(sc + kKryCoef, y, (size_t)ls.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CHECK(dev_multi_axpy(ctx, N, ls.size(), Z, N, sc + kKryCoef, -1.0, x_inout, nullptr));     // x += Z y (for -A: -=)
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (y is read before it changes)
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

// ---- K-column residual -------------------------------------------------------------------------
// the operators btd_residual_multi_kernel covers: the K-column forms (multi_form, forms.hpp) with a tile
static bool res_multi_ok(const aggmg_op* A) {
  if (A->cgt || !A->btd) return false;
  const BtdDev& b = *A->btd;
  if (!multi_form(b.m, b.cmp)) return false;
  TileQuery q;
  q.launch = kTileMulti;
  q.te = kMultiNT / b.m;
  q.halo = 1;
  return launch_has_tile(q);
}

template <int M, bool CMP>
static int launch_res_multi_t(aggmg_ctx* ctx, ResMultiArgs m) {
  constexpr int TE = kMultiNT / M;
  m.owned = multi_tile_owned(TE, 1, 1);   // host_plan.hpp, the planner res_multi_ok asks
  if (m.owned <= 0) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "internal: K-column residual tile too small");
  const int64_t ntiles = (m.lv.ne + m.owned - 1) / m.owned;
  if (ntiles == 0) return AGGMG_OK;
  with_col_group(m.kc, kMultiKB, [&](auto g) {   // (never a group above the cycle's)
    constexpr int KB = decltype(g)::value;
    const size_t lds = (size_t)KB * (TE + 2) * M * sizeof(double);
    hipLaunchKernelGGL((btd_residual_multi_kernel<M, CMP, KB, kMultiNT>), dim3((unsigned)ntiles), dim3(kMultiNT), lds, ctx->stream, m);
  });
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// R = B - A X (B null: R = -A X) on ncols columns; X, B, R column-major with their own leading dimensions
static int residual_multi(aggmg_ctx* ctx, aggmg_op* A, const double* X, int64_t ldx, const double* B, int64_t ldb, int64_t ncols,
                          double* R, int64_t ldr) {
  if (!res_multi_ok(A)) {   // column by column: the single-vector residual on every column slice
    WorkLease zero;
    if (!B) {
      CHECK(solv_lease(ctx, kSolvZero, A->m, "residual_multi", &zero));
      HIPCHK(hipMemsetAsync(zero, 0, A->m * sizeof(double), ctx->stream));
    }
    for (int64_t j = 0; j < ncols; ++j) CHECK(aggmg_residual_dev(ctx, A, X + j * ldx, B ? B + j * ldb : zero.get(), R + j * ldr));
    return AGGMG_OK;
  }
  const BtdDev& b = *A->btd;
  const int64_t group = std::min<int64_t>(ncols, kMultiKB);
  for (int64_t c0 = 0; c0 < ncols; c0 += group) {
    ResMultiArgs m;
    std::memset(&m, 0, sizeof(m));
    m.lv = btd_args(b).lv;
    m.x = X + c0 * ldx;
    m.b = B ? B + c0 * ldb : nullptr;
    m.r = R + c0 * ldr;
    m.ld_x = ldx;
    m.ld_b = ldb;
    m.ld_r = ldr;
    m.kc = (int)std::min<int64_t>(group, ncols - c0);
    ProfScope ps(ctx, AGGMG_KIND_RESIDUAL, 0);
    int rc = AGGMG_OK;   // (res_multi_ok: the form is one of multi_form)
    with_form<multi_form>(b.m, b.cmp, [&](auto f) { rc = launch_res_multi_t<decltype(f)::kM, decltype(f)::kCmp>(ctx, m); });
    CHECK(rc);
  }
  return AGGMG_OK;
}

extern "C" int aggmg_residual_multi_dev(aggmg_ctx* ctx, aggmg_op* A, const double* X, const double* B, int64_t ncols, int64_t ld,
                                        double* R) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!A || !X || !R) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual_multi_dev: NULL argument");
  if (ncols < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual_multi_dev: ncols must be >= 1");
  if (A->m != A->n) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_residual_multi_dev: the operator is not square");
  const int64_t N = A->m;
  if (ld < N) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual_multi_dev: ld must be >= N (" + std::to_string(N) + ")");
  const int64_t span = (ncols - 1) * ld + N;
  if (ranges_overlap(R, span, X, span) || ranges_overlap(R, span, B, span))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual_multi_dev: R must not overlap X or B");
  HIPCHK(hipSetDevice(ctx->device));
  if (N == 0) return AGGMG_OK;
  return residual_multi(ctx, A, X, ld, B, ld, ncols, R, ld);
}

extern "C" int aggmg_residual_multi_launch_bytes(aggmg_ctx* ctx, aggmg_op* A, int64_t ncols, int has_b, int64_t* read_bytes,
                                                 int64_t* write_bytes) {
  if (!ctx || !A || !read_bytes || !write_bytes) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual_multi_launch_bytes: NULL argument");
  if (ncols < 1) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_residual_multi_launch_bytes: ncols must be >= 1");
  if (!res_multi_ok(A))
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, "aggmg_residual_multi_launch_bytes: the operator runs aggmg_residual_dev column by column");
  btd_launch_bytes(*A->btd, false, true, true, true, nullptr, nullptr, false, read_bytes, write_bytes, ncols);
  if (!has_b) *read_bytes -= ncols * A->m * (int64_t)sizeof(double);
  return AGGMG_OK;
}

// ---- the active set of a K-column loop: slot s of the work matrices holds column col[s]; a finished column leaves and
// the last active slot's state moves into its place, so the active columns stay contiguous ------------------------------
struct ActiveCols {
  std::vector<int> col;
  int n = 0;
  bool dirty = true;   // the device copy of col (ctx->cols_map) is out of date
  explicit ActiveCols(int64_t K) : col((size_t)K), n((int)K) {
    for (int64_t j = 0; j < K; ++j) col[(size_t)j] = (int)j;
  }
  int upload(aggmg_ctx* ctx) {
    if (!dirty || n == 0) return AGGMG_OK;
    // (the stream is idle here: the callers have just read the norms back)
    HIPCHK(hipMemcpyAsync(ctx->cols_map, col.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dirty = false;
    return AGGMG_OK;
  }
  // drops the slots flagged in `finished` (n entries); move(dst, src) carries slot src's state to slot dst
  template <class F>
  int drop(const std::vector<char>& finished, F&& move) {
    for (int s = n - 1; s >= 0; --s) {
      if (!finished[(size_t)s]) continue;
      const int last = n - 1;
      if (s != last) {
        CHECK(move(s, last));
        col[(size_t)s] = col[(size_t)last];
      }
      --n;
      dirty = true;
    }
    return AGGMG_OK;
  }
};

static int multi_solver_args(aggmg_ctx* ctx, const char* who, aggmg_hier* h, const double* B, const double* X, int64_t ncols,
                             int64_t ld, int maxiter, int nPre, int nPost) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!h || !B || !X) return fail(ctx, AGGMG_ERR_ARGUMENT, std::string(who) + ": NULL argument");
  const char* own = ncols > (1 << 20)          ? "more than 2^20 columns"
                    : (nPre < 0 || nPost < 0) ? "negative sweep count"
                    : maxiter < 0             ? "negative maxiter"
                                              : nullptr;
  return multi_entry_check(ctx, who, h->lv[0].N, ncols, ld, own, ColsOut(), {}, nullptr, h);   // (X holds the guesses: no overlap rule)
}

// K conjugate-gradient recurrences in lockstep (aggmg_pcg_dev per column): per-column scalars on the device, the
// preconditioner one K-column cycle from zero guesses, q = -A p from the K-column residual
extern "C" int aggmg_pcg_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* B, double* X, int64_t ncols, int64_t ld,
                                   int maxiter, double tol, int nPre, int nPost, double alpha, double* res_hist, int* n_iters,
                                   int64_t* work_cols) {
  CHECK(multi_solver_args(ctx, "aggmg_pcg_multi_dev", h, B, X, ncols, ld, maxiter, nPre, nPost));
  if (!res_hist || !n_iters) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_pcg_multi_dev: NULL argument");
  if (nPre != nPost) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_pcg_multi_dev: the preconditioner must be symmetric (nPre == nPost)");
  aggmg_op* A = h->lv[0].A;
  const int64_t N = A->m, K = ncols;
  const int64_t span = (K - 1) * ld + N;
  if (ranges_overlap(X, span, B, span)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_pcg_multi_dev: X must not overlap B");
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(cols_scalars(ctx, K));
  WorkLease vec[4];   // (kSolvZero stays free: residual_multi takes it)
  for (int s = 0; s < 4; ++s) CHECK(solv_lease(ctx, (SolvSlot)s, N * K, "aggmg_pcg_multi_dev", &vec[s]));
  double *R = vec[kSolvR], *Z = vec[kSolvZ], *P = vec[kSolvP], *Q = vec[kSolvQ];
  double *rz = cols_sc(ctx, kColRz), *pq = cols_sc(ctx, kColPq), *rzn = cols_sc(ctx, kColRzNew), *nr = cols_sc(ctx, kColRes),
         *nbd = cols_sc(ctx, kColNormB);
  const unsigned grid = (unsigned)((N + kThreads - 1) / kThreads);
  std::vector<double> nb((size_t)K), res((size_t)K);
  std::vector<char> fin((size_t)K);
  int64_t work = 0;
  for (int64_t j = 0; j < K; ++j) n_iters[j] = 0;
  CHECK(dev_dot_cols(ctx, N, K, B, ld, B, ld, nbd, 1));
  CHECK(read_scalars(ctx, nbd, K, nb.data()));
  CHECK(residual_multi(ctx, A, X, ld, B, ld, K, R, N));                                    // r = b - A x
  CHECK(aggmg_vcycle_multi_dev(ctx, h, nullptr, R, K, N, nPre, nPost, alpha, Z));           // z = M^-1 r
  work += K;
  HIPCHK(hipMemcpyAsync(P, Z, (size_t)N * K * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  CHECK(dev_dot_cols(ctx, N, K, R, N, Z, N, rz, 0));
  ActiveCols act(K);
  for (int it = 0; it < maxiter && act.n > 0; ++it) {
    const int na = act.n;
    CHECK(act.upload(ctx));
    CHECK(residual_multi(ctx, A, P, N, nullptr, 0, na, Q, N));                             // q = -A p
    CHECK(dev_dot_cols(ctx, N, na, P, N, Q, N, pq, 0));
    for_col_chunks(na, [&](int64_t c0, unsigned kc) {
      hipLaunchKernelGGL(pcg_xr_cols_kernel, dim3(grid, kc), dim3(kThreads), 0, ctx->stream, N, X, ld,
                         (const int*)(ctx->cols_map + c0), R + c0 * N, (const double*)(P + c0 * N), (const double*)(Q + c0 * N), N,
                         (const double*)(rz + c0), (const double*)(pq + c0));
    });
    HIPCHK(hipGetLastError());
    CHECK(dev_dot_cols(ctx, N, na, R, N, R, N, nr, 1));
    CHECK(read_scalars(ctx, nr, na, res.data()));
    bool any = false;
    for (int s = 0; s < na; ++s) {
      const int j = act.col[(size_t)s];
      res_hist[(int64_t)j * maxiter + it] = res[(size_t)s];
      n_iters[j] = it + 1;
      fin[(size_t)s] = res[(size_t)s] < tol * nb[(size_t)j];
      any = any || fin[(size_t)s];
    }
    if (it + 1 == maxiter) break;   // (the single-vector loop's last cycle feeds nothing either)
    if (any) {
      CHECK(act.drop(fin, [&](int dst, int src) {
        HIPCHK(hipMemcpyAsync(R + (int64_t)dst * N, R + (int64_t)src * N, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(P + (int64_t)dst * N, P + (int64_t)src * N, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(rz + dst, rz + src, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        return (int)AGGMG_OK;
      }));
      if (act.n == 0) break;
    }
    const int nn = act.n;
    CHECK(aggmg_vcycle_multi_dev(ctx, h, nullptr, R, nn, N, nPre, nPost, alpha, Z));
    work += nn;
    CHECK(dev_dot_cols(ctx, N, nn, R, N, Z, N, rzn, 0));
    for_col_chunks(nn, [&](int64_t c0, unsigned kc) {
      hipLaunchKernelGGL(pcg_p_cols_kernel, dim3(grid, kc), dim3(kThreads), 0, ctx->stream, N, P + c0 * N, (const double*)(Z + c0 * N), N,
                         (const double*)(rzn + c0), (const double*)(rz + c0));
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rz, rzn, (size_t)nn * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (work_cols) *work_cols = work;
  return AGGMG_OK;
}

// multigrid() per column: check_every K-column cycles, then the K-column residual and the column norms
extern "C" int aggmg_multigrid_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* X0, const double* B, int64_t ncols, int64_t ld,
                                         int maxiter, double tol, int check_every, int nPre, int nPost, double alpha, double* X,
                                         double* res_hist, int* n_cycles, int* n_checks, const double* U_exact, double* err_hist,
                                         int64_t* work_cols) {
  CHECK(multi_solver_args(ctx, "aggmg_multigrid_multi_dev", h, B, X, ncols, ld, maxiter, nPre, nPost));
  if (!X0 || !res_hist || !n_cycles || !n_checks || check_every < 1)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_multigrid_multi_dev: bad argument");
  if ((U_exact == nullptr) != (err_hist == nullptr))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_multigrid_multi_dev: U_exact and err_hist come together (or both NULL)");
  aggmg_op* A = h->lv[0].A;
  const int64_t N = A->m, K = ncols;
  const int64_t span = (K - 1) * ld + N;
  if (ranges_overlap(X, span, X0, span) || ranges_overlap(X, span, B, span) || ranges_overlap(X, span, U_exact, span))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_multigrid_multi_dev: X must not overlap X0, B or U_exact");
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(cols_scalars(ctx, K));
  for (int64_t j = 0; j < K; ++j) n_cycles[j] = n_checks[j] = 0;
  if (work_cols) *work_cols = 0;
  const size_t colb = (size_t)N * sizeof(double);
  if (maxiter == 0) {   // the reference returns its initial `x = zeros(length(x0))` (src/solvers.jl:119)
    if (N) HIPCHK(hipMemset2DAsync(X, (size_t)ld * sizeof(double), 0, colb, (size_t)K, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return AGGMG_OK;
  }
  WorkLease vec[4];
  for (int s = 0; s < 4; ++s) CHECK(solv_lease(ctx, (SolvSlot)s, N * K, "aggmg_multigrid_multi_dev", &vec[s]));
  double *R = vec[kSolvR], *Xa = vec[kSolvZ], *Xb = vec[kSolvP], *Bw = vec[kSolvQ];
  double *nr = cols_sc(ctx, kColRes), *ne = cols_sc(ctx, kColErr), *nbd = cols_sc(ctx, kColNormB);
  std::vector<double> nb((size_t)K), res((size_t)K), err((size_t)K);
  std::vector<char> fin((size_t)K);
  CHECK(dev_dot_cols(ctx, N, K, B, ld, B, ld, nbd, 1));
  CHECK(read_scalars(ctx, nbd, K, nb.data()));
  const int nchk_max = (maxiter + check_every - 1) / check_every;
  if (N) {
    HIPCHK(hipMemcpy2DAsync(Xa, colb, X0, (size_t)ld * sizeof(double), colb, (size_t)K, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpy2DAsync(Bw, colb, B, (size_t)ld * sizeof(double), colb, (size_t)K, hipMemcpyDeviceToDevice, ctx->stream));
  }
  double *cur = Xa, *alt = Xb;
  ActiveCols act(K);
  int64_t work = 0;
  int done = 0;
  auto keep = [&](int s) {   // slot s's iterate is column col[s]'s result
    if (N) HIPCHK(hipMemcpyAsync(X + (int64_t)act.col[(size_t)s] * ld, cur + (int64_t)s * N, colb, hipMemcpyDeviceToDevice, ctx->stream));
    return (int)AGGMG_OK;
  };
  while (done < maxiter && act.n > 0) {
    const int k = std::min(check_every, maxiter - done);
    const int na = act.n;
    for (int c = 0; c < k; ++c) {
      CHECK(aggmg_vcycle_multi_dev(ctx, h, cur, Bw, na, N, nPre, nPost, alpha, alt));
      std::swap(cur, alt);
      work += na;
    }
    done += k;
    if (U_exact) {   // err[i] = ||x - u_exact||, src/solvers.jl:128
      CHECK(act.upload(ctx));
      CHECK(dev_diff_cols(ctx, N, na, cur, N, U_exact, ld, ctx->cols_map, ne));
    }
    CHECK(residual_multi(ctx, A, cur, N, Bw, N, na, R, N));
    CHECK(dev_dot_cols(ctx, N, na, R, N, R, N, nr, 1));
    if (U_exact) CHECK(read_scalars(ctx, ne, na, err.data()));
    CHECK(read_scalars(ctx, nr, na, res.data()));
    bool any = false;
    for (int s = 0; s < na; ++s) {
      const int j = act.col[(size_t)s];
      const int64_t at = (int64_t)j * nchk_max + n_checks[j];
      if (U_exact) err_hist[at] = err[(size_t)s];
      res_hist[at] = res[(size_t)s];
      n_checks[j] += 1;
      n_cycles[j] = done;
      fin[(size_t)s] = res[(size_t)s] < tol * nb[(size_t)j];   // src/solvers.jl:131
      any = any || fin[(size_t)s];
    }
    if (any) {
      for (int s = 0; s < na; ++s)
        if (fin[(size_t)s]) CHECK(keep(s));
      CHECK(act.drop(fin, [&](int dst, int src) {
        HIPCHK(hipMemcpyAsync(cur + (int64_t)dst * N, cur + (int64_t)src * N, colb, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(Bw + (int64_t)dst * N, Bw + (int64_t)src * N, colb, hipMemcpyDeviceToDevice, ctx->stream));
        return (int)AGGMG_OK;
      }));
    }
  }
  for (int s = 0; s < act.n; ++s) CHECK(keep(s));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (work_cols) *work_cols = work;
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// Flexible GMRES on K right-hand sides in lockstep (EXTENSION): K recurrences of aggmg_fgmres_dev, one HostGmres per
// column, the cycle and the operator product on N x kact matrices, the orthogonalisation of all active columns in one
// launch sequence (krylov_kernels.hpp: the *_cols kernels), one read-back per iteration.
// ---------------------------------------------------------------------------------------------
// device scalars per column of capacity: 65 dots and the norm behind them (packed per pass: dot (c, i) of a pass over
// nvec vectors and na slots at [c * nvec + i], the norms at [na * nvec + c]), 65 coefficients from the host, beta
constexpr int64_t kKrycDots = kKryMaxVec + 1, kKrycCoef = kKryMaxVec, kKrycScalars = kKrycDots + kKrycCoef + 1;

static int kryc_scalars(aggmg_ctx* ctx, int64_t K) {
  CHECK(cols_scalars(ctx, K));
  CHECK(kry_scalars(ctx));
  if (ctx->kryc_cap >= K) return AGGMG_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->kryc_cap = 0;
  CHECK(ctx->kryc_part.alloc(ctx, K * kKrycDots * kDotBlocks));
  CHECK(ctx->kryc_sc.alloc(ctx, K * kKrycScalars, true));
  CHECK(ctx->kryc_map.alloc(ctx, K));
  ctx->kryc_cap = K;
  return AGGMG_OK;
}
static double* kryc_coef(aggmg_ctx* ctx) { return ctx->kryc_sc + ctx->kryc_cap * kKrycDots; }
static double* kryc_beta(aggmg_ctx* ctx) { return kryc_coef(ctx) + ctx->kryc_cap * kKrycCoef; }

template <int G>
static void launch_multi_dot_cols(aggmg_ctx* ctx, unsigned kc, int64_t n, const double* V, int64_t bs, int64_t cs, const double* W,
                                  int64_t ldw, int64_t pcol, double* part) {
  hipLaunchKernelGGL(multi_dot_cols_partial_kernel<G>, dim3(kDotBlocks, kc), dim3(kThreads), 0, ctx->stream, n, V, bs, cs, W, ldw,
                     pcol, part);
}
template <int G>
static void launch_multi_axpy_cols(aggmg_ctx* ctx, unsigned kc, int64_t n, const double* V, int64_t bs, int64_t cs,
                                   const double* coef, int64_t cld, double scale, double* W, int64_t ldw, const int* wcol,
                                   double* part) {
  if (part)
    hipLaunchKernelGGL((multi_axpy_cols_kernel<G, true>), dim3(kDotBlocks, kc), dim3(kThreads), 0, ctx->stream, n, V, bs, cs, coef,
                       cld, scale, W, ldw, wcol, part);
  else
    hipLaunchKernelGGL((multi_axpy_cols_kernel<G, false>), dim3(kDotBlocks, kc), dim3(kThreads), 0, ctx->stream, n, V, bs, cs, coef,
                       cld, scale, W, ldw, wcol, part);
}

// out[c * nvec + i] = V_i[:, c] . W[:, c], c < na <= kryc_cap, i < nvec <= kKryMaxVec (out on the device): per group of 8
// vectors one pass over W for all slots, then one workgroup per dot; everything stays on the stream
static int dev_multi_dot_cols(aggmg_ctx* ctx, int64_t n, int64_t nvec, int64_t na, const double* V, int64_t bs, int64_t cs,
                              const double* W, int64_t ldw, double* out) {
  for (int64_t i0 = 0; i0 < nvec; i0 += kKrylovGroup) {
    const int g = (int)std::min<int64_t>(kKrylovGroup, nvec - i0);
    for_col_chunks(na, [&](int64_t c0, unsigned kc) {
#define KRY_CALL(G) \
  launch_multi_dot_cols<G>(ctx, kc, n, V + i0 * bs + c0 * cs, bs, cs, W + c0 * ldw, ldw, nvec, ctx->kryc_part + (c0 * nvec + i0) * kDotBlocks)
      KRY_GROUP_SWITCH(g, KRY_CALL)
#undef KRY_CALL
    });
  }
  hipLaunchKernelGGL(dot_cols_final_kernel, dim3((unsigned)(na * nvec)), dim3(kThreads), 0, ctx->stream, kDotBlocks,
                     (const double*)ctx->kryc_part, out, 0);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

// W[:, d(c)] += V_c (scale coef_c), coef_c = coef + c * cld on the device, d(c) = wcol ? wcol[c] : c, in groups of 8
// (ascending); norm_out (device, na entries, or null) receives the norms of the stored columns, summed by the pass of
// the last group
static int dev_multi_axpy_cols(aggmg_ctx* ctx, int64_t n, int64_t nvec, int64_t na, const double* V, int64_t bs, int64_t cs,
                               const double* coef, int64_t cld, double scale, double* W, int64_t ldw, const int* wcol,
                               double* norm_out) {
  double* part = ctx->kryc_part + ctx->kryc_cap * kKryMaxVec * kDotBlocks;
  for (int64_t i0 = 0; i0 < nvec; i0 += kKrylovGroup) {
    const int g = (int)std::min<int64_t>(kKrylovGroup, nvec - i0);
    const bool last = norm_out && i0 + g == nvec;
    for_col_chunks(na, [&](int64_t c0, unsigned kc) {
#define KRY_CALL(G)                                                                                                      \
  launch_multi_axpy_cols<G>(ctx, kc, n, V + i0 * bs + c0 * cs, bs, cs, coef + c0 * cld + i0, cld, scale, wcol ? W : W + c0 * ldw, \
                            ldw, wcol ? wcol + c0 : nullptr, last ? part + c0 * kDotBlocks : nullptr)
      KRY_GROUP_SWITCH(g, KRY_CALL)
#undef KRY_CALL
    });
  }
  if (norm_out)
    hipLaunchKernelGGL(dot_cols_final_kernel, dim3((unsigned)na), dim3(kThreads), 0, ctx->stream, kDotBlocks, (const double*)part,
                       norm_out, 1);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}

static int kry_cols_args(aggmg_ctx* ctx, const char* who, const double* V, int64_t n, int64_t nvec, int64_t ncols, int64_t bstride,
                         int64_t cstride, const double* W, int64_t ldw, const void* host) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  const std::string w(who);
  if (!V || !W || !host) return fail(ctx, AGGMG_ERR_ARGUMENT, w + ": NULL argument");
  if (n < 0 || nvec < 1 || nvec > kKryMaxVec)
    return fail(ctx, AGGMG_ERR_ARGUMENT, w + ": needs n >= 0 and 1 <= nvec <= " + std::to_string(kKryMaxVec));
  if (ncols < 1 || ncols > (1 << 20)) return fail(ctx, AGGMG_ERR_ARGUMENT, w + ": needs 1 <= ncols <= 2^20");
  if (bstride < n || cstride < n || ldw < n)
    return fail(ctx, AGGMG_ERR_ARGUMENT, w + ": the basis stride, the column stride and ldw must be >= n");
  return AGGMG_OK;
}

extern "C" int aggmg_multi_dot_cols_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ncols, int64_t bstride,
                                        int64_t cstride, const double* W, int64_t ldw, double* out_host) {
  CHECK(kry_cols_args(ctx, "aggmg_multi_dot_cols_dev", V, n, nvec, ncols, bstride, cstride, W, ldw, out_host));
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(kryc_scalars(ctx, ncols));
  CHECK(dev_multi_dot_cols(ctx, n, nvec, ncols, V, bstride, cstride, W, ldw, ctx->kryc_sc));
  return read_scalars(ctx, ctx->kryc_sc, ncols * nvec, out_host);
}

extern "C" int aggmg_multi_axpy_norm_cols_dev(aggmg_ctx* ctx, const double* V, int64_t n, int64_t nvec, int64_t ncols,
                                              int64_t bstride, int64_t cstride, const double* coef_host, double* W_inout,
                                              int64_t ldw, double* norm_out_host) {
  CHECK(kry_cols_args(ctx, "aggmg_multi_axpy_norm_cols_dev", V, n, nvec, ncols, bstride, cstride, W_inout, ldw, coef_host));
  if (ranges_overlap(V, (nvec - 1) * bstride + (ncols - 1) * cstride + n, W_inout, (ncols - 1) * ldw + n))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_multi_axpy_norm_cols_dev: W must not overlap V");
  HIPCHK(hipSetDevice(ctx->device));
  CHECK(kryc_scalars(ctx, ncols));
  double* coef = kryc_coef(ctx);   // packed as the host array: nvec per column
  HIPCHK(hipMemcpyAsync(coef, coef_host, (size_t)(ncols * nvec) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  double* norms = norm_out_host ? ctx->kryc_sc.get() : nullptr;
  CHECK(dev_multi_axpy_cols(ctx, n, nvec, ncols, V, bstride, cstride, coef, nvec, 1.0, W_inout, ldw, nullptr, norms));
  if (norm_out_host) return read_scalars(ctx, norms, ncols, norm_out_host);
  HIPCHK(hipStreamSynchronize(ctx->stream));   // (coef_host has been read when this returns)
  return AGGMG_OK;
}

// K recurrences of aggmg_fgmres_dev in lockstep.  Work space (ctx->kry_work): V[j][slot][N], Z[j][slot][N], W[slot][N]
// with ncols slots per basis index, so that V_j and Z_j of the active slots are contiguous N x kact matrices with
// leading dimension N.  All active columns share the position j in the restart cycle and the iteration counter: a
// column that stops leaves, and the others go on exactly as they would alone.
extern "C" int aggmg_fgmres_multi_dev(aggmg_ctx* ctx, aggmg_hier* h, const double* B, double* X, int64_t ncols, int64_t ld,
                                      int restart, int maxiter, double tol, int nPre, int nPost, double alpha, double* res_hist,
                                      int* n_iters, int64_t* work_cols) {
  CHECK(multi_solver_args(ctx, "aggmg_fgmres_multi_dev", h, B, X, ncols, ld, maxiter, nPre, nPost));
  if (!res_hist || !n_iters) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_fgmres_multi_dev: NULL argument");
  if (restart < 1 || restart > AGGMG_FGMRES_MAX_RESTART)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_fgmres_multi_dev: restart must be 1 .. " + std::to_string(AGGMG_FGMRES_MAX_RESTART));
  aggmg_op* A = h->lv[0].A;
  const int64_t N = A->m, K = ncols;
  const int64_t span = (K - 1) * ld + N;
  if (ranges_overlap(X, span, B, span)) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_fgmres_multi_dev: X must not overlap B");
  CHECK(schedule_check(ctx, h, nPre, nPost));
  HIPCHK(hipSetDevice(ctx->device));
  for (int64_t j = 0; j < K; ++j) n_iters[j] = 0;
  if (work_cols) *work_cols = 0;
  if (maxiter == 0 || N == 0) return AGGMG_OK;
  CHECK(kryc_scalars(ctx, K));
  const int64_t bs = N * K;   // from basis vector j of a slot to its vector j + 1
  const int64_t need = (2 * (int64_t)restart + 2) * bs;
  if (ctx->kry_work.size() != need || !ctx->kry_work) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    (void)ctx->kry_work.reset(ctx);
    if (int st = ctx->kry_work.alloc(ctx, need))
      return fail(ctx, st, "aggmg_fgmres_multi_dev: no device memory for the work space of " + std::to_string(need * 8) +
                               " bytes (restart " + std::to_string(restart) + ", ncols " + std::to_string(K) + ", " +
                               std::to_string(2 * restart + 2) + " matrices of " + std::to_string(N) + " x " + std::to_string(K) +
                               "): " + ctx->err);
  }
  double* V = ctx->kry_work;
  double* Z = V + ((int64_t)restart + 1) * bs;
  double* W = Z + (int64_t)restart * bs;
  double* sc = ctx->kryc_sc;
  double* coefd = kryc_coef(ctx);
  double* betad = kryc_beta(ctx);
  const size_t colb = (size_t)N * sizeof(double);
  const unsigned grid = (unsigned)((N + kThreads - 1) / kThreads);
  auto divide = [&](int64_t na, const double* s, double* Vj) {   // Vj[:, c] = W[:, c] / s[c]
    for_col_chunks(na, [&](int64_t c0, unsigned kc) {
      hipLaunchKernelGGL(div_scalar_cols_kernel, dim3(grid, kc), dim3(kThreads), 0, ctx->stream, N, (const double*)(W + c0 * N), N,
                         s + c0, Vj + c0 * N, N);
    });
  };
  std::vector<double> nb((size_t)K), beta((size_t)K), got((size_t)(K * kKrycDots));
  std::vector<double> yfin((size_t)(K * kKrycCoef)), ycyc((size_t)(K * kKrycCoef));
  std::vector<char> fin((size_t)K), upd((size_t)K);
  std::vector<HostGmres> ls((size_t)K);   // by column: a move carries none
  double col[AGGMG_FGMRES_MAX_RESTART + 2];
  CHECK(dev_dot_cols(ctx, N, K, B, ld, B, ld, cols_sc(ctx, kColNormB), 1));
  CHECK(read_scalars(ctx, cols_sc(ctx, kColNormB), K, nb.data()));
  GmresSlots slots((int)K);
  int it = 0;
  while (slots.active() > 0 && it < maxiter) {
    int na = slots.active();
    // every cycle starts from r = b - A x: the K-column residual on every run of slots whose columns are neighbours
    for (int s = 0; s < na;) {
      int e = s + 1;
      while (e < na && slots.column(e) == slots.column(e - 1) + 1) ++e;
      const int64_t c = slots.column(s);
      CHECK(residual_multi(ctx, A, X + c * ld, ld, B + c * ld, ld, e - s, W + (int64_t)s * N, N));
      s = e;
    }
    CHECK(dev_dot_cols(ctx, N, na, W, N, W, N, betad, 1));
    CHECK(read_scalars(ctx, betad, na, beta.data()));
    bool any = false;
    for (int s = 0; s < na; ++s) {   // (at entry: x untouched, n_iters = 0)
      const double b = beta[(size_t)s];
      fin[(size_t)s] = b == 0.0 || b < tol * nb[(size_t)slots.column(s)] || !std::isfinite(b);
      any = any || fin[(size_t)s];
    }
    if (any) {
      CHECK(slots.finish(fin, [&](int dst, int src) {
        HIPCHK(hipMemcpyAsync(W + (int64_t)dst * N, W + (int64_t)src * N, colb, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(betad + dst, betad + src, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        beta[(size_t)dst] = beta[(size_t)src];
        return (int)AGGMG_OK;
      }));
      na = slots.active();
      if (na == 0) break;
    }
    divide(na, betad, V);   // v_0 = r / beta
    HIPCHK(hipGetLastError());
    for (int s = 0; s < na; ++s) ls[(size_t)slots.column(s)].start(beta[(size_t)s]);
    const int len = std::min(restart, maxiter - it);
    for (int j = 0; j < len; ++j) {
      na = slots.active();
      const int64_t nvec = j + 1;
      double* Zj = Z + (int64_t)j * bs;
      CHECK(aggmg_vcycle_multi_dev(ctx, h, nullptr, V + (int64_t)j * bs, na, N, nPre, nPost, alpha, Zj));   // Z_j = M^-1 V_j
      slots.count_cycle();
      CHECK(residual_multi(ctx, A, Zj, N, nullptr, 0, na, W, N));                                           // W = -A Z_j
      double* norms = sc + (int64_t)na * nvec;
      CHECK(dev_multi_dot_cols(ctx, N, nvec, na, V, bs, N, W, N, sc));                                      // h_c = V_c' w_c
      CHECK(dev_multi_axpy_cols(ctx, N, nvec, na, V, bs, N, sc, nvec, -1.0, W, N, nullptr, norms));         // w_c -= V_c h_c; ||w_c||
      CHECK(read_scalars(ctx, sc, (int64_t)na * (nvec + 1), got.data()));
      ++it;
      any = false;
      for (int s = 0; s < na; ++s) {
        const int c = slots.column(s);
        for (int i = 0; i <= j; ++i) col[i] = got[(size_t)(s * nvec + i)];
        col[j + 1] = got[(size_t)(na * nvec + s)];
        const double res = ls[(size_t)c].push(col);
        res_hist[(int64_t)c * maxiter + it - 1] = res;
        n_iters[c] = it;
        if (!std::isfinite(res)) {   // (x keeps the value of the last finished cycle)
          fin[(size_t)s] = 1;
          upd[(size_t)s] = 0;
        } else {                     // converged, or the Krylov space is exhausted (no division by 0)
          fin[(size_t)s] = upd[(size_t)s] = res < tol * nb[(size_t)c] || col[j + 1] == 0.0;
        }
        any = any || fin[(size_t)s];
      }
      if (any) {
        for (int s = 0; s < na; ++s) {   // a finished column is final: x += Z y (for -A: -=) at once
          if (!fin[(size_t)s] || !upd[(size_t)s]) continue;
          const int64_t c = slots.column(s);
          double* y = yfin.data() + c * kKrycCoef;
          ls[(size_t)c].solve(y);
          HIPCHK(hipMemcpyAsync(coefd + c * kKrycCoef, y, (size_t)nvec * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
          CHECK(dev_multi_axpy(ctx, N, nvec, Z + (int64_t)s * N, bs, coefd + c * kKrycCoef, -1.0, X + c * ld, nullptr));
        }
        CHECK(slots.finish(fin, [&](int dst, int src) {   // V_0..j, Z_0..j, W and ||w|| of the last slot
          for (int64_t i = 0; i <= j; ++i) {
            HIPCHK(hipMemcpyAsync(V + i * bs + (int64_t)dst * N, V + i * bs + (int64_t)src * N, colb, hipMemcpyDeviceToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(Z + i * bs + (int64_t)dst * N, Z + i * bs + (int64_t)src * N, colb, hipMemcpyDeviceToDevice, ctx->stream));
          }
          HIPCHK(hipMemcpyAsync(W + (int64_t)dst * N, W + (int64_t)src * N, colb, hipMemcpyDeviceToDevice, ctx->stream));
          HIPCHK(hipMemcpyAsync(norms + dst, norms + src, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
          return (int)AGGMG_OK;
        }));
        if (slots.active() == 0) break;
      }
      if (j + 1 < len) {
        divide(slots.active(), norms, V + (int64_t)(j + 1) * bs);
        HIPCHK(hipGetLastError());
      }
    }
    na = slots.active();
    if (na == 0) break;
    // the restart cycle is over for the columns still active: x_c += Z_c y_c, all in one launch sequence
    for (int s = 0; s < na; ++s) ls[(size_t)slots.column(s)].solve(ycyc.data() + (int64_t)s * kKrycCoef);
    HIPCHK(hipMemcpyAsync(coefd, ycyc.data(), (size_t)(na * kKrycCoef) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->kryc_map, slots.map(), (size_t)na * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    CHECK(dev_multi_axpy_cols(ctx, N, len, na, Z, bs, N, coefd, kKrycCoef, -1.0, X, ld, ctx->kryc_map, nullptr));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (y and the map are read before they change)
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (work_cols) *work_cols = slots.work_cols();
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// interface packing for element-partitioned runs
// ---------------------------------------------------------------------------------------------
extern "C" int aggmg_copy_segments_dev(aggmg_ctx* ctx, int nseg, const double* const* src, double* const* dst,
                                       const int64_t* rows, const int64_t* cols, const int64_t* src_ld,
                                       const int64_t* dst_ld) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (nseg < 0 || nseg > 4 || (nseg && (!src || !dst || !rows || !cols || !src_ld || !dst_ld)))
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_copy_segments_dev: 0..4 segments, no NULL arrays");
  CopySegs S{};
  int64_t most = 0;
  for (int g = 0; g < nseg; ++g) {
    if (rows[g] < 0 || cols[g] < 0 || (rows[g] * cols[g] > 0 && (!src[g] || !dst[g])) ||
        (rows[g] > 1 && (src_ld[g] < cols[g] || dst_ld[g] < cols[g])))
      return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_copy_segments_dev: bad segment");
    S.src[g] = src[g];
    S.dst[g] = dst[g];
    S.rows[g] = rows[g];
    S.cols[g] = cols[g];
    S.src_ld[g] = src_ld[g];
    S.dst_ld[g] = dst_ld[g];
    most = std::max(most, rows[g] * cols[g]);
  }
  if (nseg == 0 || most == 0) return AGGMG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const unsigned gx = (unsigned)std::min<int64_t>((most + kThreads - 1) / kThreads, 4096);
  hipLaunchKernelGGL(copy_segments_kernel, dim3(gx, (unsigned)nseg), dim3(kThreads), 0, ctx->stream, S);
  HIPCHK(hipGetLastError());
  return AGGMG_OK;
}


// ---------------------------------------------------------------------------------------------
// Measurement aid (tools/exp_coarse.py --calibrate): what a plain streaming kernel reaches on a given grid,
// as the ceiling the coarsest solve's streaming steps are held against.  mode 0: 16-byte copy src -> dst
// (nbytes read + nbytes written), mode 1: read only (nbytes read, one 16-byte store per thread that the
// compiler cannot prove dead).  Grid-stride over `workgroups` workgroups of 256 threads, four independent
// loads in flight per thread and pass.  Timed here with HIP events on the context stream (synchronous).
// ---------------------------------------------------------------------------------------------
template <int MODE>
static __global__ __launch_bounds__(kThreads) void stream_copy_kernel(const double2* __restrict__ src, double2* __restrict__ dst,
                                                                     int64_t n16) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double2 acc = make_double2(0.0, 0.0);
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const double2 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    if (MODE == 0) {
      dst[i] = a, dst[i + stride] = b, dst[i + 2 * stride] = c, dst[i + 3 * stride] = d;
    } else {
      acc.x += (a.x + b.x) + (c.x + d.x);
      acc.y += (a.y + b.y) + (c.y + d.y);
    }
  }
  for (; i < n16; i += stride) {
    const double2 a = src[i];
    if (MODE == 0) dst[i] = a;
    else acc.x += a.x, acc.y += a.y;
  }
  if (MODE == 1 && acc.x == 0.12345 && acc.y == 0.54321) dst[threadIdx.x] = acc;   // (never: keeps the loads alive)
}

extern "C" int aggmg_debug_stream_copy(aggmg_ctx* ctx, void* dst, const void* src, int64_t nbytes, int workgroups, int mode,
                                       double* ms_out) {
  if (!ctx) return AGGMG_ERR_ARGUMENT;
  if (!dst || !src || nbytes < 16 || workgroups < 1 || (mode != 0 && mode != 1) || !ms_out)
    return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_debug_stream_copy: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, ctx->stream));
  if (mode == 0)
    hipLaunchKernelGGL(stream_copy_kernel<0>, dim3((unsigned)workgroups), dim3(kThreads), 0, ctx->stream, (const double2*)src,
                       (double2*)dst, nbytes / 16);
  else
    hipLaunchKernelGGL(stream_copy_kernel<1>, dim3((unsigned)workgroups), dim3(kThreads), 0, ctx->stream, (const double2*)src,
                       (double2*)dst, nbytes / 16);
  hipError_t le = hipGetLastError();
  (void)hipEventRecord(e1, ctx->stream);
  hipError_t se = hipEventSynchronize(e1);
  float ms = 0.f;
  if (le == hipSuccess && se == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (le != hipSuccess) return fail(ctx, AGGMG_ERR_HIP, std::string("stream_copy_kernel: ") + hipGetErrorString(le));
  if (se != hipSuccess) return fail(ctx, AGGMG_ERR_HIP, std::string("stream_copy_kernel: ") + hipGetErrorString(se));
  *ms_out = ms;
  return AGGMG_OK;
}
