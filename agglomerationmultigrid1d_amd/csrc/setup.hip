// Device-side set-up of libaggmg_hip: host code here only allocates, launches the
// kernels of setup_kernels.hpp and reads back a handful of flags -- no O(n) host loop touches an
// operator any more.  Compiled with -ffp-contract=off (see setup_kernels.hpp).
#include <functional>

#include <hipcub/hipcub.hpp>

#include "internal.hpp"
#include "setup_kernels.hpp"
#include "pair_elem_kernels.hpp"

namespace {

inline unsigned grid_for(int64_t n) { return (unsigned)((n + kSetupThreads - 1) / kSetupThreads); }

// a few ints of flags on the device, read back synchronously
struct Flags {
  DevArray<int> d;
  int n = 0;
  int init(aggmg_ctx* ctx, int count) {
    n = count;
    return d.alloc(ctx, count, true);
  }
  int read(aggmg_ctx* ctx, int* host) {
    HIPCHK(hipMemcpyAsync(host, d, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return AGGMG_OK;
  }
  int clear(aggmg_ctx* ctx) {
    HIPCHK(hipMemsetAsync(d, 0, n * sizeof(int), ctx->stream));
    return AGGMG_OK;
  }
};

#define LAUNCH(kern, n, ...)                                                                      \
  do {                                                                                            \
    if ((n) > 0) hipLaunchKernelGGL(kern, dim3(grid_for(n)), dim3(kSetupThreads), 0, ctx->stream, __VA_ARGS__); \
    HIPCHK(hipGetLastError());                                                                    \
  } while (0)

}  // namespace

// ---------------------------------------------------------------------------------------------
// upload
// ---------------------------------------------------------------------------------------------
int setup_csc_upload(aggmg_ctx* ctx, int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval,
                     const double* nzval, int one_based, CsrDev* out) {
  const int64_t base = one_based ? 1 : 0;
  const int64_t nnz = colptr[n] - base;
  out->nrows = n;  // rows of the transposed orientation = columns of the matrix
  out->ncols = m;
  out->nnz = nnz;
  CHECK(out->rowptr.alloc(ctx, n + 1));
  CHECK(out->colind.alloc(ctx, nnz));
  CHECK(out->vals.alloc(ctx, nnz));
  DevArray<int64_t> cp64, rv64;
  CHECK(cp64.alloc(ctx, n + 1));
  CHECK(rv64.alloc(ctx, nnz));
  HIPCHK(hipMemcpyAsync(cp64, colptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (nnz) {
    HIPCHK(hipMemcpyAsync(rv64, rowval, (size_t)nnz * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(out->vals, nzval, (size_t)nnz * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  Flags f;
  CHECK(f.init(ctx, 4));
  LAUNCH(csc_convert_colptr_kernel, n + 1, n, cp64.get(), base, nnz, out->rowptr, f.d);
  int h[4];
  CHECK(f.read(ctx, h));  // the row pass below walks colptr: it must be sane first
  if (h[0]) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: colptr not monotone");
  if (h[3]) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: colptr does not start at the index base");
  LAUNCH(csc_convert_rows_kernel, n, n, m, (const int32_t*)out->rowptr, rv64.get(), base, out->colind, f.d);
  CHECK(f.read(ctx, h));
  if (h[1]) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_csc_upload: row index out of range");
  if (h[2]) return fail(ctx, AGGMG_ERR_ARGUMENT, "aggmg_csc_upload: row indices not strictly ascending in a column");
  return AGGMG_OK;
}

// CSR-stream row blocks of a device CSR (rows cut into runs of <= kStreamNnz entries and <= 4 * kThreads
// rows); only the generic kernels need them
int setup_stream_blocks(aggmg_ctx* ctx, CsrDev* d) {
  if (d->rowblk || d->nrows == 0) return AGGMG_OK;
  d->lpr = 1;
  {
    const double avg = (double)d->nnz / (double)d->nrows;
    while (d->lpr < 64 && (double)d->lpr * 1.5 < avg) d->lpr *= 2;
  }
  if ((double)d->nnz / (double)d->nrows > 48.0) return AGGMG_OK;  // long rows: lanes-per-row kernel
  std::vector<int32_t> rowptr(d->nrows + 1);
  HIPCHK(hipMemcpyAsync(rowptr.data(), d->rowptr, rowptr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  {
    int32_t mx = 0;
    for (int64_t i = 0; i < d->nrows; ++i) mx = std::max(mx, rowptr[i + 1] - rowptr[i]);
    d->maxrow = mx;
  }
  const int64_t nrows = d->nrows;
  const std::vector<int32_t> blk = stream_row_blocks(rowptr.data(), nrows, kStreamNnz, kStreamRows);   // host_plan.hpp
  d->nblk = (int64_t)blk.size() - 1;
  CHECK(d->rowblk.upload(ctx, blk));
  // square and banded: row blocks for csr_band_kernel (x window in LDS, several point-Jacobi sweeps per launch) --
  // a tile -- a block's rows plus (S - 1) * bw halo rows on either side -- has at most kThreads rows and kBandNnz entries;
  // S, the most sweeps per launch, is chosen per operator so that the halo stays near a quarter of the tile
  static const bool band_on = [] {
    const char* e = std::getenv("AGGMG_CSR_BAND");
    return !(e && e[0] == '0');
  }();
  if (band_on && d->nrows == d->ncols && nrows > 1) {
    Flags f;
    CHECK(f.init(ctx, 1));
    LAUNCH(csr_bandwidth_kernel, nrows, d->view(), f.d);
    int bwv = 0;
    CHECK(f.read(ctx, &bwv));
    if (bwv <= kBandMaxBw) {
      const int bw = std::max(bwv, 1);
      std::vector<int32_t> bb;
      const int S = std::max(2, std::min(kBandSweeps, 1 + 32 / bw));
      // (band_row_blocks: block rows + 2 * S * bw <= window  <=>  tile rows = block rows + 2 (S - 1) bw <= kThreads)
      const bool ok = band_row_blocks(rowptr.data(), nrows, bw, S, kBandNnz, kThreads + 2 * bw, kThreads, &bb);   // host_plan.hpp
      if (ok) {
        d->band_sweeps = S;
        d->bw = bw;
        d->nbandblk = (int64_t)bb.size() - 1;
        CHECK(d->bandblk.upload(ctx, bb));
      }
    }
  }
  return AGGMG_OK;
}

// row-gather CSR of the matrix from its CSC arrays: stable radix sort of the entries by row
int setup_transpose(aggmg_ctx* ctx, const CsrDev& csc, int64_t m, CsrDev* out) {
  const int64_t n = csc.nrows, nnz = csc.nnz;
  out->nrows = m;
  out->ncols = n;
  out->nnz = nnz;
  CHECK(out->rowptr.alloc(ctx, m + 1, true));
  CHECK(out->colind.alloc(ctx, nnz));
  CHECK(out->vals.alloc(ctx, nnz));
  if (nnz == 0) return AGGMG_OK;
  // rowptr: histogram of the row indices, exclusive scan
  DevArray<int32_t> counts;
  CHECK(counts.alloc(ctx, m + 1, true));
  LAUNCH(row_count_kernel, nnz, nnz, (const int32_t*)csc.colind, counts.get());
  size_t sbytes = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, sbytes, counts.get(), out->rowptr.get(), (int)(m + 1), ctx->stream));
  DevArray<char> stmp;
  CHECK(stmp.alloc(ctx, (int64_t)sbytes));
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(stmp.get(), sbytes, counts.get(), out->rowptr.get(), (int)(m + 1), ctx->stream));
  // entries sorted by row; the sort is stable, so columns stay ascending inside a row
  DevArray<int32_t> ecol;
  DevArray<uint32_t> iota, perm, keys;
  CHECK(ecol.alloc(ctx, nnz));
  CHECK(iota.alloc(ctx, nnz));
  CHECK(perm.alloc(ctx, nnz));
  CHECK(keys.alloc(ctx, nnz));
  LAUNCH(csc_entry_cols_kernel, n, n, (const int32_t*)csc.rowptr, ecol.get());
  LAUNCH(iota_kernel, nnz, nnz, iota.get());
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < m) ++bits;
  size_t rbytes = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, rbytes, (const uint32_t*)csc.colind.get(), keys.get(), iota.get(),
                                            perm.get(), (int)nnz, 0, bits, ctx->stream));
  DevArray<char> rtmp;
  CHECK(rtmp.alloc(ctx, (int64_t)rbytes));
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(rtmp.get(), rbytes, (const uint32_t*)csc.colind.get(), keys.get(), iota.get(),
                                            perm.get(), (int)nnz, 0, bits, ctx->stream));
  LAUNCH(csr_gather_kernel, nnz, nnz, (const uint32_t*)perm, (const int32_t*)ecol,
         (const double*)csc.vals, out->colind, out->vals);
  HIPCHK(hipStreamSynchronize(ctx->stream));  // the temporaries go out of scope
  return AGGMG_OK;
}

int op_ensure_csr(aggmg_ctx* ctx, aggmg_op* op) {
  if (!op->csr.rowptr) CHECK(setup_transpose(ctx, op->csc, op->m, &op->csr));
  return setup_stream_blocks(ctx, &op->csr);
}

int op_ensure_csc_blocks(aggmg_ctx* ctx, aggmg_op* op) { return setup_stream_blocks(ctx, &op->csc); }

// host copy of the row-gather CSR (the host banded LU fallback of the coarsest solve wants one)
int op_host_csr(aggmg_ctx* ctx, aggmg_op* op, HostCsr* h) {
  CHECK(op_ensure_csr(ctx, op));
  h->rowptr.resize(op->m + 1);
  h->colind.resize(op->nnz);
  h->vals.resize(op->nnz);
  HIPCHK(hipMemcpyAsync(h->rowptr.data(), op->csr.rowptr, (op->m + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (op->nnz) {
    HIPCHK(hipMemcpyAsync(h->colind.data(), op->csr.colind, op->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h->vals.data(), op->csr.vals, op->nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// smoothers
// ---------------------------------------------------------------------------------------------
int setup_jacobi_diag(aggmg_ctx* ctx, const aggmg_op* A, DevArray<double>* diag) {
  CHECK(diag->alloc(ctx, A->m));
  LAUNCH(diag_extract_kernel, A->m, A->m, (const int32_t*)A->csc.rowptr, (const int32_t*)A->csc.colind,
         (const double*)A->csc.vals, diag->get());
  return AGGMG_OK;
}

// row -> covering entries of the index lists (flat index block * m + i), rows by histogram + scan, the entries by a
// stable sort on the row: ascending flat index inside a row, the same order every time
int setup_block_order(aggmg_ctx* ctx, aggmg_smoother* sm) {
  if (sm->ordered) return AGGMG_OK;
  const int64_t N = sm->N, total = sm->nb * sm->m;
  // The one-pass sweep reads the operator rows of a block where they lie: blocks listed in an order unrelated to
  // their indices would turn that into scattered 100-byte reads (measured: 498 us per sweep against 289 us for the
  // four-launch form on 2^20 element blocks listed in random order).  The order of the blocks means nothing to an
  // additive / hybrid smoother, so they are put in ascending order of their smallest index, once, in place.
  if (sm->nb > 1) {
    Flags uns;
    CHECK(uns.init(ctx, 1));
    DevArray<uint32_t> keys, keys2, iota, order;
    CHECK(keys.alloc(ctx, sm->nb));
    LAUNCH(block_minkey_kernel, sm->nb, sm->nb, (int)sm->m, (const int32_t*)sm->inds, keys.get(), uns.d);
    int u1 = 0;
    CHECK(uns.read(ctx, &u1));
    if (u1) {
      CHECK(keys2.alloc(ctx, sm->nb));
      CHECK(iota.alloc(ctx, sm->nb));
      CHECK(order.alloc(ctx, sm->nb));
      LAUNCH(iota_kernel, sm->nb, sm->nb, iota.get());
      int kb = 1;
      while (kb < 32 && ((int64_t)1 << kb) < N) ++kb;
      size_t rb = 0;
      HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, rb, keys.get(), keys2.get(), iota.get(),
                                                order.get(), (int)sm->nb, 0, kb, ctx->stream));
      DevArray<char> rt;
      CHECK(rt.alloc(ctx, (int64_t)rb));
      HIPCHK(hipcub::DeviceRadixSort::SortPairs(rt.get(), rb, keys.get(), keys2.get(), iota.get(),
                                                order.get(), (int)sm->nb, 0, kb, ctx->stream));
      DevArray<int32_t> inds2;
      DevArray<double> binv2;
      CHECK(inds2.alloc(ctx, total));
      CHECK(binv2.alloc(ctx, total * sm->m));
      LAUNCH(block_permute_kernel, total, total, (int)sm->m, (const uint32_t*)order, (const int32_t*)sm->inds,
             (const double*)sm->binv, inds2, binv2);
      HIPCHK(hipStreamSynchronize(ctx->stream));
      std::swap(sm->inds, inds2);   // the old arrays are released with the temporaries
      std::swap(sm->binv, binv2);
    }
  }
  sm->ordered = true;
  return AGGMG_OK;
}

int setup_block_cover(aggmg_ctx* ctx, aggmg_smoother* sm) {
  if (sm->cover_ptr) return AGGMG_OK;
  CHECK(setup_block_order(ctx, sm));
  const int64_t N = sm->N, total = sm->nb * sm->m;
  DevArray<int32_t> cptr;   // (the two are released on an early return)
  DevArray<uint32_t> cidx;
  CHECK(cptr.alloc(ctx, N + 1, true));
  if (total > 0) {
    CHECK(cidx.alloc(ctx, total));
    DevArray<int32_t> counts;
    DevArray<uint32_t> iota, keys;
    CHECK(counts.alloc(ctx, N + 1, true));
    LAUNCH(row_count_kernel, total, total, (const int32_t*)sm->inds, counts.get());
    size_t sbytes = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, sbytes, counts.get(), cptr.get(), (int)(N + 1), ctx->stream));
    DevArray<char> stmp;
    CHECK(stmp.alloc(ctx, (int64_t)sbytes));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(stmp.get(), sbytes, counts.get(), cptr.get(), (int)(N + 1), ctx->stream));
    CHECK(iota.alloc(ctx, total));
    CHECK(keys.alloc(ctx, total));
    LAUNCH(iota_kernel, total, total, iota.get());
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < N) ++bits;
    size_t rbytes = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, rbytes, (const uint32_t*)sm->inds.get(), keys.get(), iota.get(), cidx.get(),
                                              (int)total, 0, bits, ctx->stream));
    DevArray<char> rtmp;
    CHECK(rtmp.alloc(ctx, (int64_t)rbytes));
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(rtmp.get(), rbytes, (const uint32_t*)sm->inds.get(), keys.get(), iota.get(), cidx.get(),
                                              (int)total, 0, bits, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the temporaries go out of scope
  }
  sm->cover_ptr = std::move(cptr);
  sm->cover_idx = std::move(cidx);
  return AGGMG_OK;
}

// blocks [nb][m][m] (row-major, or one column-major Julia Matrix per block) -> inverses on the device;
// *first_singular = index of the first singular block or -1
int setup_invert_blocks(aggmg_ctx* ctx, int64_t nb, int m, const double* blocks_dev, int colmajor, double* inv_dev,
                        int64_t* first_singular) {
  DevArray<unsigned long long> sing;
  CHECK(sing.alloc(ctx, 1));
  const unsigned long long none = (unsigned long long)nb;
  HIPCHK(hipMemcpyAsync(sing, &none, sizeof(none), hipMemcpyHostToDevice, ctx->stream));
  DevArray<double> work;
  const bool sized = with_block_size<invert_form>(m, [&](auto n) {
    if (nb > 0)
      hipLaunchKernelGGL((block_invert_kernel<decltype(n)::value>), dim3(grid_for(nb)), dim3(kSetupThreads), 0, ctx->stream, nb, blocks_dev,
                         colmajor, inv_dev, sing.get());
  });
  HIPCHK(hipGetLastError());
  if (!sized) {   // (no form of invert_form, forms.hpp: the kernel for any size)
    CHECK(work.alloc(ctx, nb * ((int64_t)m * m + 2 * m)));
    LAUNCH(block_invert_any_kernel, nb, nb, m, blocks_dev, colmajor, work.get(), inv_dev, sing.get());
  }
  unsigned long long got = none;
  HIPCHK(hipMemcpyAsync(&got, sing, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *first_singular = got >= none ? -1 : (int64_t)got;
  return AGGMG_OK;
}

// dg_smoother(mesh, A, :blockJac) / cg_smoother(..., :addSchwarz | :hybridSchwarz) on the device: index lists
// -> dense blocks A[inds, inds] -> pivoted LU -> inverses; contiguous aligned lists on a block-tridiagonal
// operator additionally get the index-free fused form (patterns and symmetry detected on the device)
int setup_block_smoother(aggmg_ctx* ctx, aggmg_smoother* sm, const int64_t* blockinds, int one_based, int want_btd) {
  aggmg_op* A = sm->A;
  const int64_t N = sm->N, nb = sm->nb;
  const int m = (int)sm->m;
  const int64_t total = nb * m;
  const int64_t base = one_based ? 1 : 0;
  DevArray<int64_t> inds64;
  CHECK(inds64.alloc(ctx, total));
  if (total) HIPCHK(hipMemcpyAsync(inds64, blockinds, (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
  CHECK(sm->inds.alloc(ctx, total));
  CHECK(sm->counts.alloc(ctx, N, true));
  Flags f;
  CHECK(f.init(ctx, 4));
  LAUNCH(inds_convert_kernel, total, total, N, inds64.get(), base, sm->inds, sm->counts, f.d);
  int h[4];
  CHECK(f.read(ctx, h));
  if (h[0]) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_blockjacobi_setup: block index out of range");
  sm->contiguous = (total == N) && !h[1];
  sm->overlapping = h[2] != 0;
  CHECK(sm->binv.alloc(ctx, total * m));
  int64_t sing = -1;
  auto b = std::make_shared<BtdDev>();
  bool btd_ok = false;
  if (sm->contiguous && !sm->overlapping && m <= 9) {
    // scatter the entries into the three block diagonals: the diagonal blocks ARE A[inds, inds]
    b->m = m;
    b->ne = nb;
    CHECK(b->dblk.alloc(ctx, N * m, true));
    CHECK(b->sub.alloc(ctx, N * m, true));
    CHECK(b->sup.alloc(ctx, N * m, true));
    Flags f2;
    CHECK(f2.init(ctx, 4));
    unsigned* masks = reinterpret_cast<unsigned*>(f2.d + 2);
    LAUNCH(btd_scatter_kernel, N, N, m, (const int32_t*)A->csc.rowptr, (const int32_t*)A->csc.colind,
           (const double*)A->csc.vals, b->dblk, b->sub, b->sup, f2.d, masks);
    int g[4];
    CHECK(f2.read(ctx, g));
    btd_ok = !g[0];
    CHECK(setup_invert_blocks(ctx, nb, m, b->dblk, 0, sm->binv, &sing));
    if (btd_ok && want_btd && sing < 0) {
      const unsigned submask = (unsigned)g[2], supmask = (unsigned)g[3];
      bool cmp = m >= 2 && __builtin_popcount(submask) <= 1 && __builtin_popcount(supmask) <= 1;
      int c_sub = submask ? __builtin_ctz(submask) : 0, r_sup = supmask ? __builtin_ctz(supmask) : 0;
      if (cmp && !btd_form(m, true)) cmp = false;
      if (!cmp) c_sub = r_sup = 0;
      if (cmp || btd_form(m, false)) {
        b->cmp = cmp;
        b->c_sub = c_sub;
        b->r_sup = r_sup;
        // the fused kernel's copy of the inverses
        CHECK(b->binv.alloc(ctx, N * m));
        HIPCHK(hipMemcpyAsync(b->binv, sm->binv, (size_t)N * m * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        Flags asym;
        CHECK(asym.init(ctx, 1));
        const bool try_sym = btd_sym_form(m, cmp) && ctx->sym_packing && (!cmp || c_sub == r_sup);
        if (cmp) {
          CHECK(b->scol.alloc(ctx, N));
          CHECK(b->pcol.alloc(ctx, N));
          CHECK(b->qrow.alloc(ctx, N));
          LAUNCH(btd_cmp_finish_kernel, nb, nb, m, c_sub, r_sup, (const double*)b->binv, (const double*)b->sub,
                 (const double*)b->sup, b->scol, b->pcol, b->qrow);
        } else {
          CHECK(b->P.alloc(ctx, N * m));
          CHECK(b->Q.alloc(ctx, N * m));
          LAUNCH(btd_dense_finish_kernel, N, nb, m, (const double*)b->binv, (const double*)b->sub, (const double*)b->sup,
                 b->P, b->Q);
        }
        if (try_sym) {
          LAUNCH(btd_sym_check_kernel, nb, nb, m, cmp ? 1 : 0, c_sub, r_sup, 1e-13, (const double*)b->binv,
                 (const double*)b->sub, (const double*)b->sup, asym.d);
          int a1 = 0;
          CHECK(asym.read(ctx, &a1));
          if (!a1) {
            CHECK(b->bsym.alloc(ctx, nb * (int64_t)(m * (m + 1) / 2)));
            LAUNCH(btd_sym_pack_kernel, nb, nb, m, (const double*)b->binv, b->bsym);
            if (cmp && m <= 4 && ctx->sym_residual) {
              // the explicit residual's entries as half + exact int8 corrections (AGGMG_OPT_SYMMETRIC_RESIDUAL); a level
              // where more than 1 / 1024 of the corrections overflow keeps the full arrays only
              const int T = m * (m + 1) / 2;
              Flags over;
              CHECK(over.init(ctx, 1));
              CHECK(b->dup.alloc(ctx, nb * (int64_t)T));
              CHECK(b->corr.alloc(ctx, N));
              LAUNCH(btd_sym_residual_kernel, N, nb, m, (const double*)b->dblk, (const double*)b->scol,
                     (const double*)b->qrow, b->dup, b->corr, over.d);
              int nover = 0;
              CHECK(over.read(ctx, &nover));
              const int64_t entries = nb * (int64_t)(m * (m - 1) / 2 + m);   // lower entries of D + couplings
              if ((int64_t)nover * 1024 > entries) {
                b->dup.reset();
                b->corr.reset();
              }
            }
          }
        }
        if (cmp) {  // the dense off-diagonal blocks are not read by the compressed kernels
          (void)hipStreamSynchronize(ctx->stream);
          b->sub.reset();
          b->sup.reset();
        }
        sm->btd = b;
        A->btd = b;
      }
    }
  } else {
    DevArray<double> blocks;
    CHECK(blocks.alloc(ctx, total * m));
    LAUNCH(block_extract_generic_kernel, total * m, nb, m, (const int32_t*)sm->inds, (const int32_t*)A->csc.rowptr,
           (const int32_t*)A->csc.colind, (const double*)A->csc.vals, blocks.get());
    CHECK(setup_invert_blocks(ctx, nb, m, blocks, 0, sm->binv, &sing));
  }
  if (sing >= 0)
    return fail(ctx, AGGMG_ERR_SINGULAR,
                "aggmg_blockjacobi_setup: singular block " + std::to_string(sing + 1) + " (SingularException)");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// structured transfer of a block-tridiagonal level
// ---------------------------------------------------------------------------------------------
// two-mode transfers whose first column is exactly 1.0 in every row (the constant mode of an agglomerate's modal basis
// at the fine nodes): keep the second column on its own, the fused kernels then read 8 instead of 16 bytes per row
static int setup_unit_column(aggmg_ctx* ctx, TransferBtd* t, int64_t Nf) {
  static const bool on = [] {
    const char* e = std::getenv("AGGMG_UNIT_COLUMN");
    return !(e && e[0] == '0');
  }();
  if (!on || t->mc != 2 || Nf == 0) return AGGMG_OK;
  Flags f;
  CHECK(f.init(ctx, 1));
  LAUNCH(transfer_unit_check_kernel, Nf, Nf, (const double*)t->lf, f.d);
  int notone = 0;
  CHECK(f.read(ctx, &notone));
  if (notone) return AGGMG_OK;
  CHECK(t->lf1.alloc(ctx, Nf));
  LAUNCH(transfer_second_column_kernel, Nf, Nf, (const double*)t->lf, t->lf1);
  return AGGMG_OK;
}

int setup_transfer_btd(aggmg_ctx* ctx, const aggmg_op* L, const BtdDev* Abtd, int mf, int64_t nef, int hint_mc,
                       TransferBtd* out, bool* ok) {
  *ok = false;
  const int64_t Nf = L->m, Nc = L->n;
  if (Nf != nef * mf) return AGGMG_OK;
  Flags bad;
  CHECK(bad.init(ctx, 2));  // [0]: pattern does not fit, [1]: largest agglomerate (transfer_vr_kernel)
  for (int mc = 1; mc <= 16; ++mc) {
    if (hint_mc > 0 && mc != hint_mc) continue;
    if (Nc % mc) continue;
    const int64_t nec = Nc / mc;
    if (nec == 0 || nef % nec) continue;
    const int64_t rho = nef / nec;
    if (rho > 64) continue;
    DevArray<double> lf;
    CHECK(lf.alloc(ctx, Nf * mc, true));
    CHECK(bad.clear(ctx));
    LAUNCH(transfer_scatter_kernel, Nc, Nc, mf, mc, rho, (const int32_t*)L->csc.rowptr, (const int32_t*)L->csc.colind,
           (const double*)L->csc.vals, lf, bad.d);
    int bf[2] = {0, 0};
    CHECK(bad.read(ctx, bf));
    const int b1 = bf[0];
    if (b1) continue;
    out->lf = std::move(lf);
    if (Abtd && Abtd->dblk) {
      CHECK(out->ld.alloc(ctx, Nf * mc));
      LAUNCH(transfer_ld_kernel, Nf, nef, mf, mc, (const double*)out->lf, (const double*)Abtd->dblk, out->ld);
    }
    out->mc = mc;
    out->rho = (int)rho;
    out->nec = nec;
    CHECK(setup_unit_column(ctx, out, Nf));
    *ok = true;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return AGGMG_OK;
  }
  // agglomerates of different sizes (contiguous runs of fine elements, at most 64 each)
  if (nef >= ((int64_t)1 << 31)) return AGGMG_OK;
  for (int mc = 1; mc <= 16; ++mc) {
    if (hint_mc > 0 && mc != hint_mc) continue;
    if (Nc % mc) continue;
    const int64_t nec = Nc / mc;
    if (nec == 0 || nec > nef) continue;
    DevArray<double> lf;
    DevArray<int32_t> first, parent;
    CHECK(lf.alloc(ctx, Nf * mc, true));
    CHECK(first.alloc(ctx, nec + 1, true));
    CHECK(parent.alloc(ctx, nef, true));
    CHECK(bad.clear(ctx));
    LAUNCH(transfer_vr_kernel, nec, nec, nef, mf, mc, 64, (const int32_t*)L->csc.rowptr, (const int32_t*)L->csc.colind,
           (const double*)L->csc.vals, first, parent, lf, bad.d);
    int bf[2] = {0, 0};
    CHECK(bad.read(ctx, bf));
    const int b1 = bf[0];
    if (b1) continue;
    out->lf = std::move(lf);
    out->first = std::move(first);
    out->parent = std::move(parent);
    if (Abtd && Abtd->dblk) {
      CHECK(out->ld.alloc(ctx, Nf * mc));
      LAUNCH(transfer_ld_kernel, Nf, nef, mf, mc, (const double*)out->lf, (const double*)Abtd->dblk, out->ld);
    }
    out->mc = mc;
    out->rho = 0;
    out->maxagg = bf[1];
    out->nec = nec;
    CHECK(setup_unit_column(ctx, out, Nf));
    *ok = true;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return AGGMG_OK;
  }
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// operator dictionary of a fused level
// ---------------------------------------------------------------------------------------------
namespace {
// the arrays of a level's record, in the record's order; `dict` of every field is filled in by dict_build
struct DictFields {
  DictView v;
  std::function<int(aggmg_ctx*, int64_t)> make[kDictMaxFields];   // allocates the owner's dictionary copy of field k
  DictFields(int64_t ne) {
    std::memset(&v, 0, sizeof(v));
    v.ne = ne;
  }
  template <typename T>
  void add(const DevArray<T>& full, DevArray<T>* dict, int n, bool back = false) {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "records are made of 64- and 32-bit words");
    const int k = v.nf++;
    make[k] = [this, k, dict](aggmg_ctx* ctx, int64_t count) {
      CHECK(dict->alloc(ctx, count));
      v.f[k].dict = dict->get();
      return (int)AGGMG_OK;
    };
    v.f[k] = DictField{full.get(), nullptr, n, (int)sizeof(T), back ? 1 : 0};
  }
  // (an array that is a view: the levels of the cyclic reduction)
  template <typename T>
  void add_view(const T* full, DevArray<T>* dict, int n) {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "records are made of 64- and 32-bit words");
    const int k = v.nf++;
    make[k] = [this, k, dict](aggmg_ctx* ctx, int64_t count) {
      CHECK(dict->alloc(ctx, count));
      v.f[k].dict = dict->get();
      return (int)AGGMG_OK;
    };
    v.f[k] = DictField{full, nullptr, n, (int)sizeof(T), 0};
  }
};

// The classes of identical records of a level: *nclasses > 0, cls[ne] and the dictionary's arrays (through F.make: they
// belong to the caller's object whatever happens) when the level takes the form; *nclasses = 0 when it has more than
// kDictMaxClasses distinct records or two records share a hash.
int dict_build(aggmg_ctx* ctx, DictFields& F, DevArray<uint16_t>* cls, int* nclasses) {
  *nclasses = 0;
  DictView& v = F.v;
  const int64_t ne = v.ne;
  // the distinct record hashes; more than kDictMaxClasses: the level keeps the plain path
  DevArray<unsigned long long> table;
  CHECK(table.alloc(ctx, kDictSlots, true));
  Flags stat;
  CHECK(stat.init(ctx, 2));
  LAUNCH(dict_collect_kernel, ne, v, table.get(), stat.d);
  int st[2] = {0, 0};
  CHECK(stat.read(ctx, st));
  if (st[1] || st[0] > kDictMaxClasses || st[0] < 1) return AGGMG_OK;
  std::vector<unsigned long long> slots(kDictSlots), hashes;
  HIPCHK(hipMemcpyAsync(slots.data(), table, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (unsigned long long s : slots)
    if (s) hashes.push_back(s);
  std::sort(hashes.begin(), hashes.end());
  const int nc = (int)hashes.size();
  if (nc != st[0]) return AGGMG_OK;
  // classes in ascending order of the hash, each one's record from its first element: the same dictionary every time
  DevArray<unsigned long long> sorted, rep;
  CHECK(sorted.alloc(ctx, nc));
  CHECK(rep.alloc(ctx, nc));
  HIPCHK(hipMemcpyAsync(sorted, hashes.data(), (size_t)nc * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
  const std::vector<unsigned long long> none((size_t)nc, (unsigned long long)ne);
  HIPCHK(hipMemcpyAsync(rep, none.data(), (size_t)nc * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // (the two host vectors are done with before anything below can return)
  CHECK(cls->alloc(ctx, ne));
  for (int k = 0; k < v.nf; ++k) CHECK(F.make[k](ctx, (int64_t)nc * v.f[k].n));
  Flags bad;
  CHECK(bad.init(ctx, 1));
  LAUNCH(dict_assign_kernel, ne, v, nc, (const unsigned long long*)sorted, cls->get(),
         rep.get(), bad.d);
  LAUNCH(dict_gather_kernel, nc, v, nc, (const unsigned long long*)rep);
  // every element's record against its class's, bit for bit: two records of one hash leave the level on the plain path
  LAUNCH(dict_verify_kernel, ne, v, (const uint16_t*)*cls, bad.d);
  int b1 = 0;
  CHECK(bad.read(ctx, &b1));
  if (!b1) *nclasses = nc;
  return AGGMG_OK;
}
}  // namespace

int setup_op_dictionary(aggmg_ctx* ctx, const BtdDev& b, const TransferBtd& t, std::unique_ptr<DictDev>* out) {
  out->reset();
  const int m = b.m;
  // the levels of btd_fused_kernel<M, CMP, ., SYM, ...> on a form of btd_sres_form whose transfer has two modes on equal agglomerates
  if (!(btd_sres_form(m, b.cmp) && b.bsym && b.scol && b.dblk && b.qrow)) return AGGMG_OK;
  if (!(t.rho > 0 && t.mc == 2 && t.lf) || b.ne < 1) return AGGMG_OK;
  const int T = m * (m + 1) / 2;
  auto d = std::make_unique<DictDev>();
  d->lf_unit = t.lf1 != nullptr;
  // the record: bsym[e] (T), qrow[e] (m), the mirror qrow[e-1] (m; zeros at e = 0), dup[e] (T) and corr (m words) where
  // the level has the symmetric residual form, the escape sources scol[e] (m) and dblk[e] (m*m), and the element's rows
  // of the transfer (lf1, or the two-entry rows of lf); the dictionary keeps the mirror in an array of its own (qmir)
  DictFields F(b.ne);
  F.add(b.bsym, &d->bsym, T);
  F.add(b.qrow, &d->qrow, m);
  F.add(b.qrow, &d->qmir, m, true);
  if (b.dup) {
    F.add(b.dup, &d->dup, T);
    F.add(b.corr, &d->corr, m);
  }
  F.add(b.scol, &d->scol, m);
  F.add(b.dblk, &d->dblk, m * m);
  F.add(t.lf1 ? t.lf1 : t.lf, &d->lf, m * (t.lf1 ? 1 : 2));
  CHECK(dict_build(ctx, F, &d->cls, &d->nclasses));
  if (m == 4 && d->nclasses > 0 && d->nclasses <= kElemRecMaxClasses) {
    // the record of every class once more in the layout the element-thread kernels copy into LDS (host_plan.hpp,
    // elem_record_pack), pcol = B^{-1} q_{e-1} with it: a few KB, repacked on the host
    const int nc = d->nclasses, nl = d->lf_unit ? m : 2 * m;
    std::vector<double> hb((size_t)T * nc), hq((size_t)m * nc), hm((size_t)m * nc), hd(b.dup ? (size_t)T * nc : 0), hl((size_t)nl * nc);
    std::vector<uint32_t> hc(b.dup ? (size_t)m * nc : 0);
    std::vector<double> rec((size_t)nc * kElemRecWords);
    auto down = [&](auto& v, const auto* src) {
      return hipMemcpyAsync(v.data(), src, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost, ctx->stream);
    };
    HIPCHK(down(hb, d->bsym.get()));
    HIPCHK(down(hq, d->qrow.get()));
    HIPCHK(down(hm, d->qmir.get()));
    if (b.dup) {
      HIPCHK(down(hd, d->dup.get()));
      HIPCHK(down(hc, d->corr.get()));
    }
    HIPCHK(down(hl, d->lf.get()));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    elem_record_pack(nc, hb.data(), hq.data(), hm.data(), b.dup ? hd.data() : nullptr, b.dup ? hc.data() : nullptr, hl.data(),
                     d->lf_unit, rec.data());
    CHECK(d->rec.alloc(ctx, (int64_t)rec.size()));
    HIPCHK(hipMemcpyAsync(d->rec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (the host vector is done with)
  }
  if (d->nclasses > 0) *out = std::move(d);
  return AGGMG_OK;
}

int setup_pair_dictionary(aggmg_ctx* ctx, const BtdDev& b, const TransferBtd& t, std::unique_ptr<PairDictDev>* out) {
  out->reset();
  const int m = b.m;
  // the levels of btd_pair_down_kernel / btd_pair_up_kernel: dense blocks of 2 rows, packed inverses, two modes on equal
  // agglomerates
  if (!(!b.cmp && m == 2 && b.bsym && b.sup && b.sub && b.dblk) || b.ne < 1) return AGGMG_OK;
  if (!(t.rho > 0 && t.mc == 2 && t.lf)) return AGGMG_OK;
  auto d = std::make_unique<PairDictDev>();
  d->lf_unit = t.lf1 != nullptr;
  // the record: bsym[e] (3), the rows of sup[e] (m*m), those of sup[e-1] (m*m; zeros at e = 0) in an array of its own
  // (sback), the rows of sub[e] and dblk[e] (m*m each) and the element's rows of the transfer (lf1, or the rows of lf)
  DictFields F(b.ne);
  F.add(b.bsym, &d->bsym, m * (m + 1) / 2);
  F.add(b.sup, &d->sup, m * m);
  F.add(b.sup, &d->sback, m * m, true);
  F.add(b.sub, &d->sub, m * m);
  F.add(b.dblk, &d->dblk, m * m);
  F.add(t.lf1 ? t.lf1 : t.lf, &d->lf, m * (t.lf1 ? 1 : 2));
  CHECK(dict_build(ctx, F, &d->cls, &d->nclasses));
  if (d->nclasses > 0 && d->nclasses <= kPairElemMaxClasses) {
    // the record of every class once more in the element-thread pair kernels' layout (pair_elem_kernels.hpp): a few KB,
    // repacked on the host
    const int nc = d->nclasses, nl = d->lf_unit ? m : 2 * m;
    std::vector<double> hb(3 * nc), hsb(4 * nc), hsp(4 * nc), hsu(4 * nc), hd(4 * nc), hl((size_t)nl * nc);
    std::vector<double> rec((size_t)nc * kPairRecWords, 0.0);
    auto down = [&](std::vector<double>& v, const double* src) {
      return hipMemcpyAsync(v.data(), src, v.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    };
    HIPCHK(down(hb, d->bsym));
    HIPCHK(down(hsb, d->sback));
    HIPCHK(down(hsp, d->sup));
    HIPCHK(down(hsu, d->sub));
    HIPCHK(down(hd, d->dblk));
    HIPCHK(down(hl, d->lf));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < nc; ++c) {
      double* r = rec.data() + (size_t)c * kPairRecWords;
      for (int j = 0; j < 3; ++j) r[kPairRecBsym + j] = hb[c * 3 + j];
      for (int j = 0; j < 4; ++j) {
        r[kPairRecSback + j] = hsb[c * 4 + j];
        r[kPairRecSup + j] = hsp[c * 4 + j];
        r[kPairRecSub + j] = hsu[c * 4 + j];
        r[kPairRecDblk + j] = hd[c * 4 + j];
      }
      for (int i = 0; i < 2; ++i) {   // (a unit first column: the 1.0 it stands for)
        r[kPairRecLf + 2 * i] = d->lf_unit ? 1.0 : hl[(c * 2 + i) * 2];
        r[kPairRecLf + 2 * i + 1] = d->lf_unit ? hl[c * 2 + i] : hl[(c * 2 + i) * 2 + 1];
      }
    }
    CHECK(d->rec.alloc(ctx, (int64_t)rec.size()));
    HIPCHK(hipMemcpyAsync(d->rec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (the host vector is done with)
  }
  if (d->nclasses > 0) *out = std::move(d);
  return AGGMG_OK;
}

int setup_cgt_dictionary(aggmg_ctx* ctx, const CgtDev& g, const TransferCgt& t, std::unique_ptr<CgtDictDev>* out) {
  out->reset();
  const int m = g.m;
  // the levels of cgt_fused_kernel<M, ., ., 0, false, DICT = true>: a block size of chain_dict_form, point-Jacobi sweeps
  if (!(chain_dict_form(m) && g.sw == 0 && g.dblk && g.subrow && g.supcol) || g.ne < 1) return AGGMG_OK;
  if (!((t.type == kTrChain && t.l) || (t.type == kTrAgg && t.l && t.lp && t.rho >= 1)) || t.mc < 1) return AGGMG_OK;
  auto d = std::make_unique<CgtDictDev>();
  // the record of block e (the trailing identity-padded one is a block like any other): its rows of dblk (m*m), subrow
  // (m) and supcol (m), and its rows of the transfer -- l[e m + i][mc + 1] (chain), or l[e m + i][mc] and lp[e][mc]
  DictFields F(g.ne);
  F.add(g.dblk, &d->dblk, m * m);
  F.add(g.subrow, &d->subrow, m);
  F.add(g.supcol, &d->supcol, m);
  if (t.type == kTrChain) {
    F.add(t.l, &d->l, m * (t.mc + 1));
  } else {
    F.add(t.l, &d->l, m * t.mc);
    F.add(t.lp, &d->lp, t.mc);
  }
  CHECK(dict_build(ctx, F, &d->cls, &d->nclasses));
  if (d->nclasses > 0) *out = std::move(d);
  return AGGMG_OK;
}

int setup_patch_dictionary(aggmg_ctx* ctx, PatchDev& P) {
  P.dict.reset();
  if (!P.btd || !P.zrows || P.ne < 1) return AGGMG_OK;
  const BtdDev& b = *P.btd;
  const int m = P.m;
  if (!(b.dblk && (b.cmp ? (b.scol && b.qrow) : (b.sub && b.sup)))) return AGGMG_OK;
  auto d = std::make_unique<PatchDictDev>();
  // the record of element e: its rows of zrows (4 m*m: the rows of Z_{e-1} and of Z_e they apply), of dblk (m*m) and of
  // the couplings -- scol[e] (m) and qrow[e] (m), or the rows of sub[e] and sup[e] (m*m each); all at index e
  DictFields F(P.ne);
  F.add(P.zrows, &d->zrows, 4 * m * m);
  F.add(b.dblk, &d->dblk, m * m);
  if (b.cmp) {
    F.add(b.scol, &d->scol, m);
    F.add(b.qrow, &d->qrow, m);
  } else {
    F.add(b.sub, &d->sub, m * m);
    F.add(b.sup, &d->sup, m * m);
  }
  CHECK(dict_build(ctx, F, &d->cls, &d->nclasses));
  if (d->nclasses > 0) P.dict = std::move(d);
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// cyclic-reduction factorisation of the coarsest operator
// ---------------------------------------------------------------------------------------------
template <int M>
static int cr_levels_t(aggmg_ctx* ctx, CrDev* cr, DevArray<double> a, DevArray<double> b, DevArray<double> c, int64_t n,
                       double* cond_dev, int* bad_dev) {
  const int mm2 = M * M;
  while (n > 1) {
    if (M <= 2 && n <= 1024) {  // a candidate for the tail's first level (parallel cyclic reduction, setup_pcr)
      CrDev::Raw R{(int)cr->lv.size(), n, {}, {}, {}};
      for (DevArray<double>* p : {&R.a, &R.b, &R.c}) CHECK(p->alloc(ctx, n * mm2));
      HIPCHK(hipMemcpyAsync(R.a, a, n * mm2 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(R.b, b, n * mm2 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(R.c, c, n * mm2 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      cr->raw.push_back(std::move(R));
    }
    const int64_t ne = (n + 1) / 2, no = n / 2;
    CrDev::Factors F;   // the level's: fe, fo, lu, perm below
    DevArray<double> Za, Zc, a2, b2, c2;
    CHECK(F.lu.alloc(ctx, no * mm2));
    CHECK(F.perm.alloc(ctx, no * M));
    CHECK(Za.alloc(ctx, std::max<int64_t>(no, 1) * mm2));
    CHECK(Zc.alloc(ctx, std::max<int64_t>(no, 1) * mm2));
    CHECK(a2.alloc(ctx, ne * mm2));
    CHECK(b2.alloc(ctx, ne * mm2));
    CHECK(c2.alloc(ctx, ne * mm2));
    double *lu = F.lu, *fe = nullptr, *fo = nullptr;
    int32_t* perm = F.perm;
    LAUNCH((cr_factor_odd_kernel<M>), no, no, (const double*)a, (const double*)b, (const double*)c, lu, perm, Za.get(), Zc.get(),
           cond_dev, bad_dev);
    LAUNCH((cr_schur_even_kernel<M>), ne, n, ne, (const double*)a, (const double*)b, (const double*)c, (const double*)Za,
           (const double*)Zc, a2, b2, c2);
    HIPCHK(hipStreamSynchronize(ctx->stream));  // Za / Zc leave scope
    // the solve reads the off-diagonal blocks parity-split (forward: even rows, backward: odd rows)
    CHECK(F.fe.alloc(ctx, ne * 2 * mm2));
    CHECK(F.fo.alloc(ctx, std::max<int64_t>(no, 1) * 2 * mm2));
    fe = F.fe, fo = F.fo;
    LAUNCH(cr_split_kernel, n * 2 * mm2, n, mm2, (const double*)a, (const double*)c, fe, fo);
    LAUNCH((cr_even_multipliers_kernel<M>), no, no, ne, (const double*)lu, (const int32_t*)perm, fe);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    CrLevel L;
    L.n = n;
    L.n_even = ne;
    L.n_odd = no;
    L.fe = fe;
    L.fo = fo;
    L.lu = lu;
    L.perm = perm;
    cr->lv.push_back(L);
    cr->owned.push_back(std::move(F));
    a = std::move(a2);  // (the diagonal blocks of this level live on in the odd factors and the next level)
    b = std::move(b2);
    c = std::move(c2);
    n = ne;
    if ((int)cr->lv.size() > kCrMaxLevels) return AGGMG_ERR_UNSUPPORTED;
  }
  CrDev::Factors F;
  CHECK(F.lu.alloc(ctx, mm2));
  CHECK(F.perm.alloc(ctx, M));
  hipLaunchKernelGGL((cr_factor_last_kernel<M>), dim3(1), dim3(64), 0, ctx->stream, (const double*)b, F.lu.get(), F.perm.get(),
                     cond_dev, bad_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  cr->lu_last = F.lu;
  cr->perm_last = F.perm;
  cr->owned.push_back(std::move(F));
  return AGGMG_OK;
}

// parallel cyclic reduction of the tail's system (internal.hpp CrDev::Pcr): log2(n) levels of multipliers from the blocks
// kept in `raw`; leaves pcr.valid false when a diagonal block of some level is singular (the register-blocked tail stays)
template <int M>
static int setup_pcr_t(aggmg_ctx* ctx, CrDev* cr, const CrDev::Raw& R) {
  const int64_t n = R.n;
  constexpr int MM = M * M;
  int L = 0;
  while (((int64_t)1 << L) < n) ++L;
  if (L < 1 || L > kPcrMaxLevels) return AGGMG_OK;
  DevArray<double> mult, lu, ta, tb, tc;
  DevArray<int32_t> perm;
  CHECK(mult.alloc(ctx, (int64_t)L * n * 2 * MM, true));
  CHECK(lu.alloc(ctx, n * MM));
  CHECK(perm.alloc(ctx, n * M));
  CHECK(ta.alloc(ctx, n * MM));
  CHECK(tb.alloc(ctx, n * MM));
  CHECK(tc.alloc(ctx, n * MM));
  double *a2 = ta, *b2 = tb, *c2 = tc;
  Flags bad;
  CHECK(bad.init(ctx, 1));
  double *a = R.a, *b = R.b, *c = R.c;  // (the copies are scratch from here on: ping-pong with a2, b2, c2)
  for (int k = 0; k < L; ++k) {
    LAUNCH((pcr_factor_kernel<M>), n, n, (const double*)b, lu.get(), perm.get(), bad.d);
    LAUNCH((pcr_reduce_kernel<M>), n, n, (int64_t)1 << k, (const double*)a, (const double*)b, (const double*)c,
           (const double*)lu, (const int32_t*)perm, mult.get() + (int64_t)k * n * 2 * MM, a2, b2, c2);
    std::swap(a, a2), std::swap(b, b2), std::swap(c, c2);
  }
  LAUNCH((pcr_factor_kernel<M>), n, n, (const double*)b, lu.get(), perm.get(), bad.d);
  int b1 = 0;
  CHECK(bad.read(ctx, &b1));
  if (b1) return AGGMG_OK;
  cr->pcr.n = (int)n;
  cr->pcr.L = L;
  cr->pcr.mult = std::move(mult);
  cr->pcr.lu = std::move(lu);
  cr->pcr.perm = std::move(perm);
  cr->pcr.valid = true;
  return AGGMG_OK;
}

void cr_discard(CrDev* c) { *c = CrDev(); }

// AGGMG_OPT_COARSE_DICTIONARY: the chunk stages whose levels hold at most ctx->coarse_dict_cap distinct factor records
// get their table and class indices (cr_kernels.hpp: CrDictArgs), all or nothing per stage -- cr_dict_plan decides.  Only
// the stages' levels are classed, and a stage stops at its first level over the cap: a system of unlike rows costs one
// search.  The levels' full arrays stay: the other path and the tail read them.
static int setup_cr_dictionary(aggmg_ctx* ctx, CrDev* cr) {
  const int m = cr->m, cap = ctx->coarse_dict_cap, mm = m * m;
  cr->dict_even.assign(cr->lv.size(), -1);
  cr->dict_odd.assign(cr->lv.size(), -1);
  if (!cr_dict_form(m) || cap < 1) return AGGMG_OK;
  for (CrStage& S : cr->st) {
    int ne[kCrMaxStageLevels] = {0}, no[kCrMaxStageLevels] = {0};
    std::vector<DevArray<uint16_t>> ce(S.q), co(S.q);
    std::vector<DevArray<double>> fe(S.q), fo(S.q), lu(S.q);
    std::vector<DevArray<int32_t>> pm(S.q);
    bool ok = true;
    for (int l = 0; l < S.q && ok; ++l) {
      const CrLevel& L = cr->lv[S.l0 + l];
      ok = L.n_odd >= 1;
      if (!ok) break;
      DictFields E(L.n_even);
      E.add_view(L.fe, &fe[l], 2 * mm);
      CHECK(dict_build(ctx, E, &ce[l], &ne[l]));
      cr->dict_even[S.l0 + l] = ne[l];
      ok = ne[l] >= 1 && ne[l] <= cap;
      if (!ok) break;
      DictFields O(L.n_odd);
      O.add_view(L.fo, &fo[l], 2 * mm);
      O.add_view(L.lu, &lu[l], mm);
      O.add_view(L.perm, &pm[l], m);
      CHECK(dict_build(ctx, O, &co[l], &no[l]));
      cr->dict_odd[S.l0 + l] = no[l];
      ok = no[l] >= 1 && no[l] <= cap;
    }
    if (!ok) continue;
    const CrDictPlan P = cr_dict_plan(m, S.q, S.lds_total, ne, no, cap);
    if (!P.take) continue;
    // the table: the levels' dictionaries in the stage's layout, a few KB repacked on the host
    std::vector<double> tab((size_t)P.tab_words, 0.0);
    std::vector<std::vector<double>> hfo(S.q), hlu(S.q);
    std::vector<std::vector<int32_t>> hpm(S.q);
    auto down = [&](void* dst, const void* src, size_t bytes) {
      return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    };
    for (int l = 0; l < S.q; ++l) {
      hfo[l].resize((size_t)no[l] * 2 * mm);
      hlu[l].resize((size_t)no[l] * mm);
      hpm[l].resize((size_t)no[l] * m);
      HIPCHK(down(tab.data() + P.tab_e[l], fe[l].get(), (size_t)ne[l] * 2 * mm * sizeof(double)));
      HIPCHK(down(hfo[l].data(), fo[l].get(), hfo[l].size() * sizeof(double)));
      HIPCHK(down(hlu[l].data(), lu[l].get(), hlu[l].size() * sizeof(double)));
      HIPCHK(down(hpm[l].data(), pm[l].get(), hpm[l].size() * sizeof(int32_t)));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int l = 0; l < S.q; ++l) cr_dict_pack_odd(m, no[l], hfo[l].data(), hlu[l].data(), hpm[l].data(), tab.data() + P.tab_o[l]);
    CHECK(S.dict_tab.alloc(ctx, P.tab_words));
    HIPCHK(hipMemcpyAsync(S.dict_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    // the class indices of every chunk (chunk c = block c of the stage's output level), in the order of the launch's LDS
    const int64_t chunks = std::max<int64_t>(S.n_out, 1);
    CHECK(S.dict_idx.alloc(ctx, chunks * P.idx_count, true));
    for (int l = 0; l < S.q; ++l) {
      const CrLevel& L = cr->lv[S.l0 + l];
      const int shift = S.q - l - 1, cnt = 1 << shift;
      LAUNCH(cr_dict_chunk_index_kernel, chunks * (cnt + 1), chunks, cnt + 1, shift, L.n_even, (const uint16_t*)ce[l],
             S.dict_idx.get(), P.idx_count, P.idx_e[l]);
      LAUNCH(cr_dict_chunk_index_kernel, chunks * cnt, chunks, cnt, shift, L.n_odd, (const uint16_t*)co[l], S.dict_idx.get(),
             P.idx_count, P.idx_o[l]);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (the host table and the levels' class arrays are done with)
    S.dict = P;
  }
  return AGGMG_OK;
}

// probe vector of the factorisation check: entries in [-1, 1) from a hash of the index (no structure a
// tridiagonal stencil could annihilate)
__global__ __launch_bounds__(kSetupThreads) void probe_vector_kernel(int64_t n, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * kSetupThreads + threadIdx.x;
  if (i >= n) return;
  uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  w[i] = (double)(int64_t)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

// y += sign * A x from the uploaded CSC arrays, set-up checks only.  DETERMINISTIC: the acceptance decisions taken on
// its result (probe backward error, parallel tail kept or not) must come out the same run to run and on every rank
// of a partitioned job that holds a replica of the operator -- no atomics.  The operator is block-tridiagonal with
// block size m (what the cyclic reduction it checks has established), so row i has its entries in the columns of
// blocks i/m - 1 .. i/m + 1: one thread per row walks those <= 3m columns in ascending order and looks its row up in
// each (rows ascend inside a column: validated at upload).
__global__ __launch_bounds__(kSetupThreads) void csc_band_gather_kernel(int64_t n, int m, const int32_t* __restrict__ cp,
                                                                        const int32_t* __restrict__ rv,
                                                                        const double* __restrict__ vv,
                                                                        const double* __restrict__ x, double sign,
                                                                        double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * kSetupThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t bi = i / m;
  const int64_t j0 = bi > 0 ? (bi - 1) * m : 0;
  const int64_t j1 = (bi + 2) * m < n ? (bi + 2) * m : n;
  double acc = 0.0;
  for (int64_t j = j0; j < j1; ++j) {
    int32_t lo = cp[j], hi = cp[j + 1];
    while (lo < hi) {  // first entry of column j with row >= i
      const int32_t mid = lo + (hi - lo) / 2;
      if (rv[mid] < (int32_t)i) lo = mid + 1; else hi = mid;
    }
    if (lo < cp[j + 1] && rv[lo] == (int32_t)i) acc += vv[lo] * x[j];
  }
  y[i] += sign * acc;
}

int setup_probe_vector(aggmg_ctx* ctx, int64_t n, double* w) {
  LAUNCH(probe_vector_kernel, n, n, w);
  return AGGMG_OK;
}

// a smooth positive vector, 1 + cos(pi i / n) / 2: as a RIGHT-HAND SIDE of an elliptic coarse operator it asks for a large
// smooth solution -- where a reduction that accumulates like an inverse loses most against one that substitutes back
__global__ __launch_bounds__(kSetupThreads) void smooth_vector_kernel(int64_t n, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * kSetupThreads + threadIdx.x;
  if (i >= n) return;
  w[i] = 1.0 + 0.5 * cos(3.141592653589793 * (double)i / (double)n);
}

int setup_smooth_vector(aggmg_ctx* ctx, int64_t n, double* w) {
  LAUNCH(smooth_vector_kernel, n, n, w);
  return AGGMG_OK;
}

int setup_band_matvec_add(aggmg_ctx* ctx, const aggmg_op* A, int m, const double* x, double sign, double* y) {
  LAUNCH(csc_band_gather_kernel, A->m, A->m, m, (const int32_t*)A->csc.rowptr, (const int32_t*)A->csc.colind,
         (const double*)A->csc.vals, x, sign, y);
  return AGGMG_OK;
}

static int cr_factor_blocks(aggmg_ctx* ctx, CrDev* cr, DevArray<double> a, DevArray<double> b, DevArray<double> c);

// Sets cr->valid when the operator is block-tridiagonal for some block size m <= 8 and every pivot block is
// comfortably invertible; leaves it false otherwise (the caller then keeps the host banded solver).
int setup_cr(aggmg_ctx* ctx, const aggmg_op* Ac, int hint_m, CrDev* cr, int* band_out) {
  cr->valid = false;
  if (band_out) band_out[0] = band_out[1] = 0;
  const int64_t N = Ac->m;
  if (N == 0) return AGGMG_OK;
  const int32_t* cp = Ac->csc.rowptr;
  const int32_t* rv = Ac->csc.colind;
  const double* vv = Ac->csc.vals;
  Flags f;
  CHECK(f.init(ctx, 4));
  LAUNCH(band_kernel, N, N, cp, rv, f.d);
  int band[4];
  CHECK(f.read(ctx, band));
  const int kl = band[0], ku = band[1];
  if (band_out) band_out[0] = kl, band_out[1] = ku;
  Flags bad;
  CHECK(bad.init(ctx, 1));
  auto fits = [&](int mm_, bool* out) -> int {
    CHECK(bad.clear(ctx));
    LAUNCH(block_fit_kernel, N, N, mm_, cp, rv, bad.d);
    int b1 = 0;
    CHECK(bad.read(ctx, &b1));
    *out = !b1;
    return AGGMG_OK;
  };
  int m = 0;
  bool okm = false;
  if (hint_m >= 1 && hint_m <= 8) {
    CHECK(fits(hint_m, &okm));
    if (okm) m = hint_m;
  }
  // otherwise the smallest block size for which the operator is block-tridiagonal
  for (int cand = 1; !m && cand <= 8; ++cand)
    if (std::max(kl, ku) <= 2 * cand - 1) {
      CHECK(fits(cand, &okm));
      if (okm) m = cand;
    }
  if (!m) return AGGMG_OK;
  const int mm2 = m * m;
  const int64_t n = (N + m - 1) / m;
  cr->m = m;
  cr->n0 = n;
  cr->N = N;
  DevArray<double> a, b, c;
  CHECK(a.alloc(ctx, n * mm2, true));
  CHECK(b.alloc(ctx, n * mm2, true));
  CHECK(c.alloc(ctx, n * mm2, true));
  LAUNCH(cr_pack_kernel, n * m, N, m, cp, rv, vv, a, b, c);
  return cr_factor_blocks(ctx, cr, std::move(a), std::move(b), std::move(c));
}

// the element-chain entrance: the blocks come from the chain form of a CG operator (CgtDev, internal.hpp) -- block e =
// [left vertex of element e, its interior nodes], one trailing identity-padded block for the last vertex -- instead of
// from the CSC arrays in the operator's own numbering.  cr->N is the length of the block-ordered vectors; the solve
// permutes in and out through g.perm / g.inv (cr_solve, aggmg_hip.hip).
int setup_cr_chain(aggmg_ctx* ctx, const CgtDev& g, CrDev* cr) {
  cr->valid = false;
  const int m = g.m;
  const int64_t n = g.ne;
  if (m < 1 || m > 8 || n < 1) return fail(ctx, AGGMG_ERR_UNSUPPORTED, "setup_cr_chain: blocks of 1 .. 8 rows only");   // (the caller checks)
  cr->m = m;
  cr->n0 = n;
  cr->N = n * m;
  DevArray<double> a, b, c;
  CHECK(a.alloc(ctx, n * m * m, true));
  CHECK(b.alloc(ctx, n * m * m, true));
  CHECK(c.alloc(ctx, n * m * m, true));
  LAUNCH(cr_pack_chain_kernel, n * m, n, m, (const double*)g.dblk, (const double*)g.subrow, (const double*)g.supcol,
         (const int32_t*)g.perm, a.get(), b.get(), c.get());
  CHECK(cr_factor_blocks(ctx, cr, std::move(a), std::move(b), std::move(c)));
  if (cr->valid) {  // the block-ordered right-hand side and solution of a solve
    CHECK(cr->d0.alloc(ctx, n * m, true));
    CHECK(cr->x0.alloc(ctx, n * m, true));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return AGGMG_OK;
}

// levels, plan, arena and parallel tail of the n0 blocks (a, b, c) [n0][m][m] of cr->m rows; sets cr->valid, or leaves
// it false where a pivot block is close to singular or the plan does not fit
static int cr_factor_blocks(aggmg_ctx* ctx, CrDev* cr, DevArray<double> a, DevArray<double> b, DevArray<double> c) {
  const int m = cr->m;
  const int64_t n = cr->n0, N = cr->N;
  Flags bad;
  CHECK(bad.init(ctx, 1));
  DevArray<double> condt;
  CHECK(condt.alloc(ctx, 1, true));
  int st = AGGMG_OK;
  with_block_size<cr_form>(m, [&](auto mm) {
    st = cr_levels_t<decltype(mm)::value>(ctx, cr, std::move(a), std::move(b), std::move(c), n, condt, bad.d);
  });
  if (st == AGGMG_ERR_UNSUPPORTED) {  // too many levels
    cr_discard(cr);
    return AGGMG_OK;
  }
  if (st != AGGMG_OK) {
    cr_discard(cr);
    return st;
  }
  int b1 = 0;
  CHECK(bad.read(ctx, &b1));
  double cond = 0.0;
  HIPCHK(hipMemcpyAsync(&cond, condt, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  cr->cond_est = cond;
  if (b1 || !(cond < 1e13)) {  // a pivot block is singular or close to it: keep the pivoted banded LU
    cr_discard(cr);
    return AGGMG_OK;
  }
  // plan: chunk stages (one workgroup per 2^q-block chunk) until what is left fits the
  // single-workgroup tail (cr_kernels.hpp)
  const int nl = (int)cr->lv.size();
  auto level_n = [&](int l) -> int64_t { return l < nl ? cr->lv[l].n : 1; };
  auto dz = [&](int64_t len, DevArray<double>* out) -> int { return out->alloc(ctx, len, true); };
  // (AGGMG_CR_TAIL_ROWS / AGGMG_CR_MAX_Q shrink the tail and the chunks: the tests use them to run the
  // several-stage plan of systems beyond 2^24 rows at sizes a CPU reference solves in seconds)
  auto env_int = [](const char* name, int dflt, int lo, int hi) {
    const char* e = std::getenv(name);
    const int v = e && *e ? std::atoi(e) : dflt;
    return std::min(std::max(v, lo), hi);
  };
  const int tail_rows = env_int("AGGMG_CR_TAIL_ROWS", kCrTailRows, 8, kCrTailRows);
  const int max_q = env_int("AGGMG_CR_MAX_Q", ctx->cr_max_q, 1, kCrMaxStageLevels);
  CrSolvePlan plan;
  {
    const char* e = std::getenv("AGGMG_CR_FILL");
    const int fmax = e && *e ? std::atoi(e) : 12;
    const char* w = std::getenv("AGGMG_CR_MINWG");
    const int minwg = w && *w ? std::atoi(w) : 256;
    std::vector<int64_t> ln(nl);
    for (int l = 0; l < nl; ++l) ln[l] = cr->lv[l].n;
    // (large chunks -- every thread at least one sub-chunk of the streaming first step -- as long as a few hundred
    // workgroups remain; host_plan.hpp)
    if (!cr_plan_solve(ln, m, tail_rows, max_q, fmax, minwg, &plan)) {
      cr_discard(cr);
      return AGGMG_OK;
    }
  }
  for (const CrStagePlan& P : plan.stages) {
    CrStage S;
    static_cast<CrStagePlan&>(S) = P;
    const CrStageBuffers b = cr_stage_buffers(P, m);
    CHECK(dz(3 * b.part, &S.partR));  // the three boundary vectors in one allocation
    S.partL = S.partR + b.part;       // partL[0] is never written: stays zero
    S.xq = S.partL + b.part;
    if (b.stack > 0) CHECK(dz(b.stack, &S.stack));
    if (b.mid > 0) CHECK(dz(b.mid, &S.mid));
    cr->st.push_back(std::move(S));
  }
  static_cast<CrStagePlan&>(cr->tail) = plan.tail;
  if (const int64_t mid = cr_stage_buffers(plan.tail, m).mid; mid > 0) CHECK(dz(mid, &cr->tail.mid));
  // The small levels (the tail and the last steps of the stage before it) are worked through by a
  // few threads, one dependent step after the other: their factors go into ONE allocation, so that a
  // step touches a couple of pages instead of four arrays per level each on a page of its own -- an
  // address-translation miss per array is what such a step would otherwise wait for.
  {
    int pf = cr->tail.l0;
    while (pf > 0 && level_n(pf - 1) * m <= 8 * kCrTailRows) --pf;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t mm = (size_t)m * m;
    size_t total = al(mm * sizeof(double)) + al(m * sizeof(int32_t));
    for (int l = pf; l < nl; ++l) {
      const CrLevel& L = cr->lv[l];
      const size_t no = (size_t)std::max<int64_t>(L.n_odd, 1);
      total += al(L.n_even * 2 * mm * sizeof(double)) + al(no * 2 * mm * sizeof(double)) + al(no * mm * sizeof(double)) +
               al(no * m * sizeof(int32_t));
    }
    DevArray<char>& arena = cr->arena;
    CHECK(arena.alloc(ctx, (int64_t)total));
    size_t off = 0;
    auto move = [&](const void* src, size_t bytes) -> void* {
      void* dst = arena + off;
      (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream);
      off += al(bytes);
      return dst;
    };
    for (int l = pf; l < nl; ++l) {
      CrLevel& L = cr->lv[l];
      const size_t no = (size_t)std::max<int64_t>(L.n_odd, 1);
      L.fe = (const double*)move(L.fe, L.n_even * 2 * mm * sizeof(double));
      L.fo = (const double*)move(L.fo, no * 2 * mm * sizeof(double));
      L.lu = (const double*)move(L.lu, no * mm * sizeof(double));
      L.perm = (const int32_t*)move(L.perm, no * m * sizeof(int32_t));
    }
    cr->lu_last = (const double*)move(cr->lu_last, mm * sizeof(double));
    cr->perm_last = (const int32_t*)move(cr->perm_last, m * sizeof(int32_t));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int l = pf; l <= nl; ++l) cr->owned[l] = CrDev::Factors();   // (entry nl: the last block's)
  }
  // the tail's system by parallel cyclic reduction where it applies (AGGMG_CR_PCR=0: off)
  if (m <= 2 && cr->tail.nsteps >= 1 && env_int("AGGMG_CR_PCR", 1, 0, 1)) {
    // up to 512 rows: all of them in the parallel part; 513 .. 1024: its even rows (the next level's system)
    const bool pre = cr->tail.n_in > 512;
    const int want_level = cr->tail.l0 + (pre ? 1 : 0);
    const int64_t want_n = pre ? (cr->tail.n_in + 1) / 2 : cr->tail.n_in;
    if (cr->tail.n_in <= 1024 && (!pre || cr->tail.q >= 2))
      for (const auto& R : cr->raw)
        if (R.level == want_level && R.n == want_n) {
          if (m == 1) CHECK(setup_pcr_t<1>(ctx, cr, R));
          if (m == 2) CHECK(setup_pcr_t<2>(ctx, cr, R));
          cr->pcr.pre = pre;
        }
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  cr->raw.clear();
  if (n * m != N) {
    CHECK(dz(n * m, &cr->d0));
    CHECK(dz(n * m, &cr->x0));
  }
  CHECK(cr->ticket.alloc(ctx, 1, true));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  CHECK(setup_cr_dictionary(ctx, cr));
  cr->run = CrRun();
  for (const CrStage& S : cr->st) cr->run.st.push_back(cr_run_stage(S));
  cr->run.tail = cr_run_stage(cr->tail);
  cr->valid = true;
  return AGGMG_OK;
}

// ---------------------------------------------------------------------------------------------
// CG chain form
// ---------------------------------------------------------------------------------------------
static int cgt_build_impl(aggmg_ctx* ctx, aggmg_smoother* sm, const int64_t* elems, int64_t m1, int64_t nel, int one_based,
                          bool generate);

int cgt_build(aggmg_ctx* ctx, aggmg_smoother* sm, const int64_t* elems, int64_t m1, int64_t nel, int one_based) {
  return cgt_build_impl(ctx, sm, elems, m1, nel, one_based, false);
}

// AGGMG_OPT_DETECT_CHAIN: no element lists came with the operator -- try the lists of a CgMesh of degree p on
// (N - 1) / p elements in the reference's vertices-first numbering, generated on the device, for every p that divides
// N - 1 and whose entry count is plausible; cgt_build's own checks (a chain, every coupling inside the pattern) decide
int cgt_detect(aggmg_ctx* ctx, aggmg_smoother* sm) {
  const aggmg_op* A = sm->A;
  const int64_t N = A->m;
  if (N < 3 || A->m != A->n) return AGGMG_OK;
  for (int64_t p = 8; p >= 1 && !sm->cgt; --p) {
    if ((N - 1) % p) continue;
    const int64_t nel = (N - 1) / p;
    // a CG operator of degree p holds at most nel (p + 1)^2 entries, and not much fewer (Dirichlet rows are emptied)
    const double full = (double)nel * (double)((p + 1) * (p + 1));
    if ((double)A->nnz > full || (double)A->nnz < 0.5 * full) continue;
    CHECK(cgt_build_impl(ctx, sm, nullptr, p + 1, nel, 0, true));
  }
  return AGGMG_OK;
}

static int cgt_build_impl(aggmg_ctx* ctx, aggmg_smoother* sm, const int64_t* elems, int64_t m1, int64_t nel, int one_based,
                          bool generate) {
  aggmg_op* A = sm->A;
  const int64_t N = A->m;
  const int64_t p = m1 - 1;
  if (p < 1 || p > 8 || nel < 1) return AGGMG_OK;  // generic path
  if (N != nel * p + 1) return AGGMG_OK;
  const int64_t base = one_based ? 1 : 0;
  const int m = (int)p;
  const int64_t ne = nel + 1, Np = ne * m;
  if (Np >= ((int64_t)1 << 31)) return AGGMG_OK;
  auto g = std::make_shared<CgtDev>();
  g->m = m;
  g->ne = ne;
  g->N = N;
  DevArray<int64_t> el64;
  CHECK(el64.alloc(ctx, nel * m1));
  if (generate) {
    LAUNCH(chain_generate_elements_kernel, nel, nel, m, el64.get());
  } else {
    HIPCHK(hipMemcpyAsync(el64, elems, (size_t)nel * m1 * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  CHECK(g->perm.alloc(ctx, Np));
  CHECK(g->inv.alloc(ctx, N));
  HIPCHK(hipMemsetAsync(g->perm, 0xFF, (size_t)Np * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(g->inv, 0xFF, (size_t)N * 4, ctx->stream));
  Flags f;
  CHECK(f.init(ctx, 4));
  LAUNCH(chain_perm_kernel, nel, nel, m, N, el64.get(), base, g->perm, f.d);
  LAUNCH(perm_invert_kernel, Np, Np, (const int32_t*)g->perm, g->inv, f.d);
  LAUNCH(perm_cover_kernel, N, N, (const int32_t*)g->inv, f.d);
  LAUNCH(chain_affine_check_kernel, Np, ne, m, (const int32_t*)g->perm, f.d);
  int h[4];
  CHECK(f.read(ctx, h));
  if (h[0]) return fail(ctx, AGGMG_ERR_DIMENSION, "aggmg_jacobi_setup_elements: node index out of range");
  if (h[1]) return AGGMG_OK;  // not a chain: generic path
  g->affine = !h[3];
  CHECK(g->dblk.alloc(ctx, Np * m, true));
  CHECK(g->subrow.alloc(ctx, Np, true));
  CHECK(g->supcol.alloc(ctx, Np, true));
  LAUNCH(chain_scatter_kernel, N, N, m, (const int32_t*)g->inv, (const int32_t*)A->csc.rowptr, (const int32_t*)A->csc.colind,
         (const double*)A->csc.vals, g->dblk, g->subrow, g->supcol, f.d);
  LAUNCH(chain_pad_kernel, Np, Np, m, (const int32_t*)g->perm, g->dblk);
  CHECK(f.read(ctx, h));
  if (h[2]) return AGGMG_OK;  // couplings beyond the chain pattern: generic path
  sm->cgt = g;
  A->cgt = g;
  return AGGMG_OK;
}

// Element Schwarz smoothers on a chain (cg_smoother(cgMesh, A, :addSchwarz / :hybridSchwarz), src/smoother.jl:104-134):
// after cgt_build recognised the element chain, the inverses of the element blocks (already computed for the
// generic apply, K6) are re-ordered into the rows the fused kernel keeps in registers.  sw: 1 additive, 2 hybrid.
int cgt_attach_schwarz(aggmg_ctx* ctx, aggmg_smoother* sm, int sw) {
  if (!sm->cgt || !sm->binv) return AGGMG_OK;
  CgtDev& g = *sm->cgt;
  const int M = g.m;
  const int64_t nel = g.ne - 1;
  if (sm->m != M + 1 || sm->nb != nel) return AGGMG_OK;
  CHECK(g.zrows.alloc(ctx, g.ne * M * (M + 1), true));
  CHECK(g.zlast.alloc(ctx, g.ne * (M + 1), true));
  LAUNCH(chain_schwarz_rows_kernel, nel * (M + 1), nel, M, (const double*)sm->binv, g.zrows, g.zlast);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  g.sw = sw;
  return AGGMG_OK;
}

int cgt_build_transfer(aggmg_ctx* ctx, const aggmg_op* L, const CgtDev& f, const CgtDev* coarse, int hint_mc,
                       TransferCgt* out, bool* ok) {
  const int tile_blocks = cgt_tile_blocks(f.m);
  *ok = false;
  const int64_t Nf = L->m, Nc = L->n;
  if (Nf != f.N) return AGGMG_OK;
  const int M = f.m;
  const int64_t nel = f.ne - 1, Np = f.ne * M;
  const int32_t* cp = L->csc.rowptr;
  const int32_t* rv = L->csc.colind;
  const double* vv = L->csc.vals;
  Flags fl;
  CHECK(fl.init(ctx, 4));
  int h[4];

  // ---- chain: the coarse level is a CG level on the same elements ------------------------------
  if (nel > 0 && Nc > 1 && (Nc - 1) % nel == 0 && (Nc - 1) / nel <= 8 && M >= 2) {
    const int mc = (int)((Nc - 1) / nel);
    int32_t *cperm = nullptr, *cinv = nullptr;
    DevArray<int32_t> own_perm, own_inv;
    bool have = false;
    if (coarse && coarse->N == Nc && coarse->m == mc && coarse->ne == f.ne) {
      cperm = coarse->perm;
      cinv = coarse->inv;
      have = true;
    } else if (!coarse) {
      // the coarse level carries no element lists (the coarsest level has no smoother): read its chain
      // off L -- a coarse column holding a fine vertex row is that block's vertex, the others are the
      // interior nodes of the one element whose fine rows they touch, in ascending order
      CHECK(own_perm.alloc(ctx, f.ne * mc));
      CHECK(own_inv.alloc(ctx, Nc));
      cperm = own_perm;
      cinv = own_inv;
      HIPCHK(hipMemsetAsync(cperm, 0xFF, (size_t)f.ne * mc * 4, ctx->stream));
      HIPCHK(hipMemsetAsync(cinv, 0xFF, (size_t)Nc * 4, ctx->stream));
      DevArray<int32_t> slots;
      CHECK(slots.alloc(ctx, f.ne, true));
      LAUNCH(chain_coarse_vertices_kernel, Nc, Nc, M, mc, (const int32_t*)f.inv, cp, rv, cperm, cinv, fl.d);
      LAUNCH(chain_coarse_interiors_kernel, Nc, Nc, M, mc, (const int32_t*)f.inv, cp, rv, cperm, cinv, slots.get(), fl.d);
      LAUNCH(chain_coarse_sort_kernel, f.ne, f.ne, mc, cperm, cinv, (const int32_t*)slots, nel, fl.d);
      CHECK(fl.read(ctx, h));
      have = !h[1];
      CHECK(fl.clear(ctx));
    }
    if (have) {
      const int w = mc + 1;
      DevArray<double> l;
      CHECK(l.alloc(ctx, Np * w, true));
      LAUNCH(chain_transfer_scatter_kernel, Nc, Nc, M, mc, (const int32_t*)f.inv, (const int32_t*)cinv, cp, rv, vv, l, fl.d);
      CHECK(fl.read(ctx, h));
      if (!h[0]) {
        out->l = std::move(l);
        CHECK(out->cperm.alloc(ctx, f.ne * mc));
        HIPCHK(hipMemcpyAsync(out->cperm, cperm, (size_t)f.ne * mc * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        out->type = kTrChain;
        out->mc = mc;
        out->rho = 1;
        out->nec = f.ne;
        *ok = true;
        return AGGMG_OK;
      }
      l.reset();
      CHECK(fl.clear(ctx));
    }
  }

  // ---- agglomerating: the coarse level has contiguous blocks of mc DoFs per rho fine elements ---
  for (int mc = 1; mc <= 16; ++mc) {
    if (hint_mc > 0 && mc != hint_mc) continue;
    if (Nc % mc) continue;
    const int64_t nec = Nc / mc;
    if (nec == 0 || nel % nec) continue;
    const int64_t rho = nel / nec;
    if (rho > 64 || rho * 4 > tile_blocks) continue;
    DevArray<double> l, lp;
    CHECK(l.alloc(ctx, Np * mc, true));
    CHECK(lp.alloc(ctx, f.ne * mc, true));
    CHECK(fl.clear(ctx));
    LAUNCH(agg_transfer_scatter_kernel, Nc, Nc, M, mc, rho, (const int32_t*)f.inv, cp, rv, vv, l, lp, fl.d);
    CHECK(fl.read(ctx, h));
    if (h[0]) continue;
    out->l = std::move(l);
    out->lp = std::move(lp);
    out->type = kTrAgg;
    out->mc = mc;
    out->rho = (int)rho;
    out->nec = nec;
    *ok = true;
    return AGGMG_OK;
  }
  return AGGMG_OK;
}
