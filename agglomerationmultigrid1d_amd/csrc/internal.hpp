// Shared internals of libaggmg_hip: the objects behind the opaque handles of include/aggmg_hip.h
// and the small host helpers every translation unit of the library uses (error reporting, the
// owner of device memory, the leased work vectors, the HIP-event profiler, the set-up thread pool).
#pragma once
#include "../../include/aggmg_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.hpp"
#include "cr_kernels.hpp"
#include "cgt_kernels.hpp"

using namespace aggmg;

// ---------------------------------------------------------------------------------------------
// error helpers
// ---------------------------------------------------------------------------------------------
struct aggmg_ctx;
inline int fail(aggmg_ctx* ctx, int code, const std::string& msg);   // (defined below the context)

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return fail(ctx, AGGMG_ERR_HIP,                                                       \
                  std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + \
                      std::to_string(__LINE__) + ")");                                      \
  } while (0)

#define CHECK(expr)             \
  do {                          \
    int _s = (expr);            \
    if (_s != AGGMG_OK) return _s; \
  } while (0)

#include "devmem.hpp"
#include "workspace.hpp"

// ---------------------------------------------------------------------------------------------
// objects behind the opaque handles
// ---------------------------------------------------------------------------------------------
inline thread_local std::string g_create_error;

struct ProfEvent {
  hipEvent_t a, b;
  int tag;
};

struct aggmg_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  bool sym_packing = true;  // AGGMG_OPT_SYMMETRIC_PACKING
  int cr_max_q = 12;        // AGGMG_OPT_COARSE_CHUNK_LOG2
  bool detect_chain = true; // AGGMG_OPT_DETECT_CHAIN
  bool mg_checkpoint = [] { const char* e = std::getenv("AGGMG_MG_CHECKPOINT"); return !(e && e[0] == '0'); }();  // AGGMG_OPT_MG_CHECKPOINT
  bool pair_levels = [] { const char* e = std::getenv("AGGMG_PAIR"); return !(e && e[0] == '0'); }();  // AGGMG_OPT_PAIR_LEVELS
  bool sym_residual = [] { const char* e = std::getenv("AGGMG_SYM_RESIDUAL"); return !(e && e[0] == '0'); }();  // AGGMG_OPT_SYMMETRIC_RESIDUAL
  bool op_dict = [] { const char* e = std::getenv("AGGMG_OP_DICT"); return !(e && e[0] == '0'); }();  // AGGMG_OPT_OPERATOR_DICTIONARY
  bool elem_threads = [] { const char* e = std::getenv("AGGMG_ELEM_THREADS"); return !(e && e[0] == '0'); }();  // AGGMG_OPT_ELEMENT_THREADS
  int64_t elem_launches = 0;   // launches of the element-thread kernel so far (aggmg_element_thread_launches)
  bool pair_elem_threads = [] { const char* e = std::getenv("AGGMG_PAIR_ELEM_THREADS"); return !(e && e[0] == '0'); }();  // AGGMG_OPT_PAIR_ELEMENT_THREADS
  int64_t pair_elem_launches = 0;   // launches of the element-thread pair kernels so far (aggmg_pair_element_thread_launches)
  // AGGMG_OPT_ELEMENT_RECORDS_LDS: most classes of a level whose element-thread launches keep the class records in LDS
  // (0: off; at most kElemRecMaxClasses, host_plan.hpp)
  int elem_rec_cap = [] { const char* e = std::getenv("AGGMG_ELEM_RECORDS_LDS"); return (e && e[0] == '0') ? 0 : kElemRecMaxClasses; }();
  int64_t elem_rec_launches = 0;   // launches of those kernels so far (aggmg_element_record_lds_launches)
  // AGGMG_OPT_COARSE_DICTIONARY: most classes per level and parity of a chunk stage of the coarsest solve that keeps its
  // factor records in LDS (0: off; at most kCrDictMaxClasses, host_plan.hpp); read when a hierarchy is created
  int coarse_dict_cap = [] { const char* e = std::getenv("AGGMG_COARSE_DICT"); return (e && e[0] == '0') ? 0 : kCrDictMaxClasses; }();
  int64_t coarse_dict_launches = 0;   // stage launches served (aggmg_coarse_dictionary_launches)
  bool replay_presmooth = [] { const char* e = std::getenv("AGGMG_REPLAY_PRESMOOTH"); return !(e && e[0] == '0'); }();  // AGGMG_OPT_REPLAY_PRESMOOTH
  int64_t replay_launches = 0;   // replayed cycles so far (aggmg_replay_launches)
  bool patch_multi = [] { const char* e = std::getenv("AGGMG_PATCH_MULTI"); return e && e[0] == '1'; }();  // AGGMG_OPT_PATCH_MULTI (default 0)
  int64_t patch_multi_launches = 0;   // launches of patch_gs_multi_kernel so far (aggmg_patch_multi_launches)
  bool chain_multi = [] { const char* e = std::getenv("AGGMG_CHAIN_MULTI"); return e && e[0] == '1'; }();  // AGGMG_OPT_CHAIN_MULTI (default 0)
  int64_t chain_multi_launches = 0;   // launches of cgt_multi_kernel so far (aggmg_chain_multi_launches)
  bool patch_schwarz_multi = [] { const char* e = std::getenv("AGGMG_PATCH_SCHWARZ_MULTI"); return e && e[0] == '1'; }();  // AGGMG_OPT_PATCH_SCHWARZ_MULTI (default 0)
  int64_t patch_schwarz_multi_launches = 0;   // launches of patch_sweep_multi_kernel so far (aggmg_patch_schwarz_multi_launches)
  bool multi_elem_threads = [] { const char* e = std::getenv("AGGMG_MULTI_ELEM_THREADS"); return e && e[0] == '1'; }();  // AGGMG_OPT_MULTI_ELEMENT_THREADS (default 0)
  int64_t multi_elem_launches = 0;   // launches of btd_elem_rec_multi_kernel so far (aggmg_multi_element_thread_launches)
  // columns one launch of patch_sweep_multi_kernel takes of a group: kPatchSchwarzMultiCols, or what the measurement knob
  // AGGMG_PATCH_SCHWARZ_MULTI_COLS=4 | 8 says (tools/exp_patch_multi.py --group-width; profiles/r34_patch_schwarz_multi.md)
  int patch_schwarz_multi_cols = [] {
    const char* e = std::getenv("AGGMG_PATCH_SCHWARZ_MULTI_COLS");
    return e && e[0] == '4' && !e[1] ? 4 : e && e[0] == '8' && !e[1] ? 8 : kPatchSchwarzMultiCols;
  }();
  int profiling = 0;  // 0 off, 1 every launch, 2 only the fine-level fused-down launch (dominant kernel)
  std::vector<ProfEvent> prof;
  std::vector<hipEvent_t> ev_pool;
  // scratch vectors for ping-pong / temporaries, grown on demand, leased slot by slot (workspace.hpp: ScratchSlot)
  WorkVectors<kScratchSlots> scratch;
  // outer-solver work space (aggmg_multigrid_dev, aggmg_pcg_dev, ...): leased vectors (SolvSlot), dot-product
  // partials and the device-resident scalars (kSc*)
  WorkVectors<kSolvSlots> solv;
  DevArray<double> solv_part, solv_sc;
  // K-column solver loops (aggmg_pcg_multi_dev, aggmg_multigrid_multi_dev, aggmg_dot_cols_dev): for cols_cap columns,
  // kDotBlocks partials and kColsScalars scalars per column, and the slot -> column maps of the active set; lazy, grown
  // for more columns, freed with the context
  DevArray<double> cols_part, cols_sc;
  DevArray<int> cols_map;
  int64_t cols_cap = 0;
  // flexible GMRES (aggmg_fgmres_dev, aggmg_multi_dot_dev, aggmg_multi_axpy_norm_dev): the partial sums of up to 65 dots
  // and one norm, the device scalars, and the solver's (2 restart + 2) N work space -- kept between calls of the same
  // size, exchanged when another size is asked for, freed with the context
  DevArray<double> kry_part, kry_sc, kry_work;
  // its K-column forms (aggmg_fgmres_multi_dev, aggmg_multi_dot_cols_dev, aggmg_multi_axpy_norm_cols_dev): for
  // kryc_cap columns the partial sums of 65 dots and one norm, the scalars and coefficients, and the slot -> column
  // map; lazy, grown for more columns, freed with the context.  The solver's work space is kry_work,
  // (2 restart + 2) N ncols doubles, under the same rule as the single-vector solver's.
  DevArray<double> kryc_part, kryc_sc;
  DevArray<int> kryc_map;
  int64_t kryc_cap = 0;
  // owned-range reductions of the partitioned conjugate-gradient loop (aggmg_owned_dot_dev, aggmg_pcg_xr_owned_dev):
  // kOwnedBlocks partial sums per range, then the scalar; lazy, freed with the context
  DevArray<double> own_part;
  // the same for the partitioned flexible GMRES loop (aggmg_owned_multi_dot_dev, aggmg_owned_multi_axpy_norm_dev): the
  // partial sums of up to 65 dots (kOwnedBlocks per range each), 65 dots and one sum of squares; a buffer of its own, so
  // that own_part stays as the conjugate-gradient entry points read it; lazy (2.1 MB), freed with the context
  DevArray<double> own_multi_part;
  // host <-> device staging of the host-pointer entry points (aggmg_vcycle): per worker thread a stream and two
  // pinned chunks (HostStager in aggmg_hip.hip); allocated on first use
  struct StageLane {
    hipStream_t stream = nullptr;
    void* pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
  };
  std::vector<StageLane> stage;
  bool stage_failed = false;
  // host ranges the caller page-locked for good (aggmg_host_register / aggmg_host_alloc): copies from / to them go
  // straight over PCIe on the compute stream, no staging
  struct Pinned {
    char* base;
    size_t bytes;
    bool owned;   // allocated by aggmg_host_alloc (hipHostMalloc) rather than registered
  };
  std::vector<Pinned> pinned;  // the lanes could not be allocated once: aggmg_vcycle keeps to plain hipMemcpy
};

inline int fail(aggmg_ctx* ctx, int code, const std::string& msg) {
  if (ctx)
    ctx->err = msg;
  else
    g_create_error = msg;
  return code;
}

inline hipStream_t HipMem::stream_of(aggmg_ctx* ctx) { return ctx->stream; }

struct CsrDev {
  int64_t nrows = 0, ncols = 0, nnz = 0;
  DevArray<int32_t> rowptr, colind;
  DevArray<double> vals;
  int lpr = 1;
  DevArray<int32_t> rowblk;   // CSR-stream row blocks (short-row matrices), nblk + 1 entries
  int64_t nblk = 0;
  DevArray<int32_t> bandblk;  // CSR-band row blocks (square, entries within bw of the diagonal), nbandblk + 1 entries
  int64_t nbandblk = 0;
  int band_sweeps = 1;        // most point-Jacobi sweeps a csr_band_kernel launch takes on this operator (the blocks' halo is cut for it)
  int bw = -1;                // band half-width, -1: not banded / not examined
  int maxrow = -1;            // entries of the longest row (-1: not examined); <= kRowThreadMax: csr_rowthread_kernel
  CsrView view() const { return CsrView{rowptr, colind, vals, nrows}; }
};

// host copy of a CSR (only the host banded LU fallback of the coarsest solve reads an operator back)
struct HostCsr {
  std::vector<int32_t> rowptr, colind;
  std::vector<double> vals;
};

// index-free block-tridiagonal form of an operator + its block-Jacobi smoother; shared by the
// smoother that built it and the operator it describes (so aggmg_residual can use it too)
struct BtdDev {
  int m = 0;
  int64_t ne = 0;
  bool cmp = false;
  int c_sub = 0, r_sup = 0;
  DevArray<double> binv, dblk, scol, pcol, qrow;
  DevArray<double> bsym;   // packed symmetric inverses (replaces binv + pcol in the kernels) or null
  // lossless symmetric form of the explicit residual's entries (compressed couplings, m <= 4, with bsym): the upper
  // triangle of D_e row-owned, one word of int8 corrections per row (setup_kernels.hpp, btd_sym_residual_kernel); or null
  DevArray<double> dup;
  DevArray<uint32_t> corr;
  DevArray<double> sub, sup, P, Q;
};

// element-contiguous ("chain") form of a CG operator + its point-Jacobi smoother (cgt_kernels.hpp);
// shared by the smoother that built it and the operator it describes
struct CgtDev {
  int m = 0;        // rows per block = p
  int64_t ne = 0;   // blocks = elements + 1 (the trailing one holds the last vertex, identity-padded)
  int64_t N = 0;    // DoFs of the operator; the block-ordered vectors have ne * m entries
  DevArray<double> dblk, subrow, supcol;
  DevArray<int32_t> perm;   // [ne*m] block order -> reference numbering, -1 = padding
  DevArray<int32_t> inv;    // [N]    reference numbering -> block order
  bool affine = false;      // perm is the reference's vertices-first numbering: the kernel computes it
  // element Schwarz smoothers on the chain (cg_smoother :addSchwarz / :hybridSchwarz): rows of the inverses of
  // the element blocks A[nodes_e, nodes_e] in chain-local order [block e, first row of block e + 1]
  int sw = 0;               // 0 point Jacobi, 1 additive Schwarz, 2 hybrid Schwarz
  DevArray<double> zrows;   // [ne*m][m+1]  row i of element e's inverse at (e*m + i)
  DevArray<double> zlast;   // [ne][m+1]    its last row (the right vertex) at e + 1: with the block that owns the vertex
};

// operator dictionary of a fused element-patch Schwarz smoother (patch_sweep_dict_kernel in patch_kernels.hpp; the same
// search as DictDev's below): one copy of every distinct record -- every operator word patch_sweep_kernel reads on behalf
// of the element: its rows of zrows, of the diagonal block and of the couplings in the form the level has (scol + qrow, or
// sub + sup), [nclasses][...] in the layouts of the full arrays -- and the class of every element.  Belongs to the
// smoother: the record spans its arrays only, and every entry point that sweeps takes it.  The full arrays stay.
struct PatchDictDev {
  int nclasses = 0;
  DevArray<uint16_t> cls;    // [ne]
  DevArray<double> zrows, dblk, scol, qrow, sub, sup;
};

// fused form of an element-patch Schwarz smoother (aggmg_patch_schwarz_setup, patch_kernels.hpp): overlapping patches of two
// consecutive elements on a block-tridiagonal operator
struct PatchDev {
  int m = 0;         // rows per element
  int64_t ne = 0;
  bool hybrid = true;
  bool multiplicative = false;   // aggmg_patch_gs_setup: two-colour sweeps over the same patches (patch_gs_kernel)
  std::shared_ptr<BtdDev> btd;   // the element blocks of A: the sweeps' residual rows and the level's transfer launches
  DevArray<double> zrows;        // [N][2][2m] per row the two inverse rows it applies (zeros where a patch does not exist)
  std::unique_ptr<PatchDictDev> dict;   // operator dictionary of the sweep launches (AGGMG_OPT_OPERATOR_DICTIONARY), or null
};

struct aggmg_op {
  int64_t m = 0, n = 0, nnz = 0;
  int kind = AGGMG_OP_STIFFNESS;
  CsrDev csc;  // the uploaded CSC arrays (int32, 0-based) == row-gather CSR of the TRANSPOSE; always present
  CsrDev csr;  // row-gather CSR of the matrix: transposed on the device on first use (generic kernels only)
  std::shared_ptr<BtdDev> btd;  // set when a block-Jacobi smoother recognised the structure
  std::shared_ptr<CgtDev> cgt;  // set when a point-Jacobi smoother was given the CG element chain
};

struct aggmg_smoother {
  int kind = 0;  // 0 point Jacobi, 1 block (Jacobi / additive Schwarz), 2 hybrid Schwarz
  aggmg_op* A = nullptr;
  int64_t N = 0, m = 0, nb = 0;
  DevArray<double> diag;       // point Jacobi
  DevArray<double> binv;       // [nb][m][m] row-major
  DevArray<int32_t> inds;      // [nb][m]
  DevArray<double> counts;     // hybrid Schwarz
  bool overlapping = false;
  bool contiguous = false;
  // which (block, local row) entries cover each row, flat index block * m + i ascending inside a row: built on first use
  // by the generic one-pass sweep (block_sweep_kernel + block_combine_kernel)
  DevArray<int32_t> cover_ptr;    // [N + 1]
  DevArray<uint32_t> cover_idx;   // [nb * m]
  bool ordered = false;           // the blocks have been put in ascending order of their smallest index (one-pass sweep)
  bool gs = false;  // red-black block Gauss-Seidel (extension): needs the structured form
  std::shared_ptr<BtdDev> btd;  // structured fused form, or null
  std::shared_ptr<CgtDev> cgt;  // CG chain form (point Jacobi with the element lists), or null
  // element-patch Schwarz (aggmg_patch_schwarz_setup): elements per patch (0: another smoother) and, for the fused form
  // (width 2), its arrays -- btd above stays null then (a non-null btd is a block-Jacobi level), binv / inds are not kept
  int patch_width = 0;
  std::shared_ptr<PatchDev> patch;
};

struct TransferBtd {
  int mc = 0, rho = 0;   // rho: fine elements per coarse element; 0 = agglomerates of different sizes (parent / first)
  int64_t nec = 0;
  DevArray<double> lf;   // [N_f][mc]  rows of L
  DevArray<double> lf1;  // [N_f]      their second entries when mc == 2 and every first entry is exactly 1.0, else null
  DevArray<double> ld;   // [N_f][mc]  rows of (L_e' D_e)': restriction of the preconditioned residual
  DevArray<int32_t> parent;   // [ne_f]      coarse element of every fine element      (rho == 0)
  DevArray<int32_t> first;    // [ne_c + 1]  first fine element of every coarse element (rho == 0)
  int maxagg = 0;             // fine elements of the largest agglomerate                 (rho == 0)
};

// operator dictionary of a fused level (AGGMG_OPT_OPERATOR_DICTIONARY; BtdLevel::cls in kernels.hpp, the dict_* kernels of
// setup_kernels.hpp): one copy of every distinct per-element operator record -- the level's BtdDev arrays and its
// transfer's rows, [nclasses][...] in the layouts of the full arrays -- and the class of every element.  Belongs to the
// hierarchy's level: the record spans the smoother's form and the transfer.  The full arrays stay; every other kernel
// reads them.
struct DictDev {
  int nclasses = 0;
  DevArray<uint16_t> cls;    // [ne]
  DevArray<double> bsym, qrow, qmir, dup, scol, dblk;
  DevArray<uint32_t> corr;
  DevArray<double> lf;       // [nclasses][m] second entries (the transfer has lf1), else [nclasses][m][2] rows of L
  bool lf_unit = false;      // lf holds the lf1 form
  // blocks of 4 rows: the same words once more, one record of kElemRecWords per class (host_plan.hpp, elem_record_pack:
  // what the element-thread launches copy into LDS under AGGMG_OPT_ELEMENT_RECORDS_LDS); only for a level of at most
  // kElemRecMaxClasses classes, else null
  DevArray<double> rec;
};

// operator dictionary of a level the two-level launches take (PairLevel::cls in pair_kernels.hpp; the same search as
// DictDev's): one copy of every distinct record -- every operator word a pair kernel reads on behalf of the element,
// [nclasses][...] in the layouts of the full arrays -- and the class of every element.  sback holds the sup rows of the
// element before (zeros at the first one): what the kernels read as sup[e - 1].  The full arrays stay; the level's
// launches on its own, the K-column, Gauss-Seidel and element-partitioned ones read them.
struct PairDictDev {
  int nclasses = 0;
  DevArray<uint16_t> cls;    // [ne]
  DevArray<double> bsym, sup, sback, sub, dblk;
  DevArray<double> lf;       // [nclasses][2] second entries (the transfer has lf1), else [nclasses][2][2] rows of L
  bool lf_unit = false;      // lf holds the lf1 form
  // the same words once more, one record of kPairRecWords per class (pair_elem_kernels.hpp: what the element-thread
  // launches copy into LDS); only for a level of at most kPairElemMaxClasses classes, else null
  DevArray<double> rec;
};

// structured transfer of a CG chain level (CgtXfer in cgt_kernels.hpp)
struct TransferCgt {
  int type = 0, mc = 0, rho = 1;
  int64_t nec = 0;
  DevArray<double> l, lp;
  DevArray<int32_t> cperm;   // chain: coarse block order -> coarse reference numbering
};

// operator dictionary of a fused chain level (CgtArgs::cls in cgt_kernels.hpp; the same search as DictDev's): one copy of
// every distinct per-block record -- the block's rows of the CgtDev arrays and of the level's transfer, [nclasses][...]
// in the layouts of the full arrays -- and the class of every block.  The full arrays stay; every other kernel reads them.
struct CgtDictDev {
  int nclasses = 0;
  DevArray<uint16_t> cls;    // [ne]
  DevArray<double> dblk, subrow, supcol;
  DevArray<double> l;        // chain: [nclasses][m][mc + 1], agglomerating: [nclasses][m][mc]
  DevArray<double> lp;       // agglomerating: [nclasses][mc]
};

// The damping of a run of sweeps on the host: one factor for all of them (w null -- the reference's alpha,
// src/solvers.jl:19), or w[i] for sweep i of the run (a level's sweep-weight schedule, aggmg_hier_set_sweep_weights;
// aggmg_smooth_weighted_dev).  Whatever cuts the run into launches hands each launch its slice: from(s).launch(n).
struct Damping {
  double alpha;
  const double* w;
  Damping(double a, const double* w_ = nullptr) : alpha(a), w(w_) {}
  double at(int s) const { return w ? w[s] : alpha; }
  Damping from(int s) const { return Damping(alpha, w ? w + s : nullptr); }
  // the kernel argument of a launch of the run's first n sweeps (without a schedule every slot holds alpha)
  SweepWeights launch(int n) const {
    SweepWeights r;
    for (int i = 0; i < kSweepWeights; ++i) r.w[i] = w ? (i < n ? w[i] : 0.0) : alpha;
    return r;
  }
};
static_assert(kSweepWeights == AGGMG_MAX_SWEEP_WEIGHTS, "the documented limit is the kernels' array");

struct Level {
  aggmg_op* A = nullptr;
  aggmg_smoother* S = nullptr;
  aggmg_op* L = nullptr;  // level k+1 -> k
  int64_t N = 0;
  DevArray<double> u[2], rhs, tmp;
  std::unique_ptr<TransferBtd> tb;  // structured transfer to level k+1, or null
  std::unique_ptr<TransferCgt> tc;  // CG chain level: structured transfer to level k+1, or null
  std::unique_ptr<DictDev> dict;    // operator dictionary of the level's fused launches, or null
  std::unique_ptr<CgtDictDev> cdict;  // the same of a fused chain level's point-Jacobi launches, or null
  std::unique_ptr<PairDictDev> pdict; // the same of the two-level launches that take the level, or null
  bool cgt_fused = false;           // the level runs cgt_fused_kernel (chain form + structured transfer)
  bool native_io = false;           // rhs and u[1] are kept in block order (the finer level is a fused chain level)
  int64_t Nalloc = 0;               // length of the level's vectors (ne * m for chain levels)
  // sweep-weight schedule (aggmg_hier_set_sweep_weights), or scheduled == false: the entry point's alpha.  w_mid = w_post
  // ++ w_pre, the launch between two cycles (post-smoothing of one, pre-smoothing of the next); w_replay = w_pre ++ w_post,
  // the ascent that replays the pre-smoothing (AGGMG_OPT_REPLAY_PRESMOOTH)
  bool scheduled = false;
  std::vector<double> w_pre, w_post, w_mid, w_replay;
  Damping damp_pre(double alpha) const { return scheduled ? Damping(alpha, w_pre.data()) : Damping(alpha); }
  Damping damp_post(double alpha) const { return scheduled ? Damping(alpha, w_post.data()) : Damping(alpha); }
  Damping damp_mid(double alpha) const { return scheduled ? Damping(alpha, w_mid.data()) : Damping(alpha); }
  Damping damp_replay(double alpha) const { return scheduled ? Damping(alpha, w_replay.data()) : Damping(alpha); }
};

struct BandedLU {
  int64_t n = 0;
  int kl = 0, ku = 0, ldab = 0;
  std::vector<double> ab;
  std::vector<int32_t> ipiv;
};

// block cyclic reduction of the coarsest operator, factored once (device-resident)
// one launch of the cyclic reduction: levels [l0, l0 + q) in steps of up to three thread-local levels
// (cr_kernels.hpp); chunk stages reduce 2^q-block chunks to their end blocks, the tail takes the rest
struct CrStage : CrStagePlan {    // the host-side plan (host_plan.hpp) + the stage's device buffers
  DevArray<double> partR;                     // the stage's boundary system (n_out blocks): one allocation, ...
  double *partL = nullptr, *xq = nullptr;     // ... these two are views into it
  DevArray<double> stack;       // per chunk: summed inputs of the steps after the first
  DevArray<double> mid;         // per step and sub-chunk: reduced right-hand sides of the inner sub-levels' odd rows
  // AGGMG_OPT_COARSE_DICTIONARY (dict.take): the table of the levels' class records and, per chunk, the class indices of
  // its rows on all q levels (host_plan.hpp: cr_dict_plan; cr_kernels.hpp: CrDictArgs)
  CrDictPlan dict;
  DevArray<double> dict_tab;
  DevArray<uint16_t> dict_idx;
};

// Where one solve's launches read and write: per stage and for the tail the per-solve buffers and the doubles between
// consecutive columns of each (the factors are shared; partR / partL / xq of a stage share a stride)
struct CrRunStage {
  double *partR = nullptr, *partL = nullptr, *xq = nullptr, *stack = nullptr, *mid = nullptr;
  int64_t cs_part = 0, cs_stack = 0, cs_mid = 0;
};
struct CrRun {
  int kc = 1;   // columns: blockIdx.y of every launch
  std::vector<CrRunStage> st;
  CrRunStage tail;   // mid alone
};
// one column in the buffers set-up allocated: every column stride 0
inline CrRunStage cr_run_stage(const CrStage& S) { return {S.partR, S.partL, S.xq, S.stack, S.mid}; }

struct CrDev {
  bool valid = false;
  int m = 0;
  int64_t n0 = 0, N = 0;
  std::vector<CrLevel> lv;      // all reducing levels (device pointers: views of `owned` or of `arena`)
  struct Factors {              // what CrLevel points to, of one level / of the last block (lu, perm)
    DevArray<double> fe, fo, lu;
    DevArray<int32_t> perm;
  };
  std::vector<Factors> owned;   // per level, then the last block; empty where set-up moved the factors into `arena`
  DevArray<char> arena;         // the small levels' factors in one allocation (setup_cr)
  const double* lu_last = nullptr;
  const int32_t* perm_last = nullptr;
  std::vector<CrStage> st;      // chunk stages ...
  // classes of the even / odd rows' factor records per reducing level (setup_cr_dictionary): -1 not classed, 0 more than
  // the search tracks
  std::vector<int> dict_even, dict_odd;
  CrStage tail;                 // ... then the remaining levels in one workgroup
  CrRun run;                    // one column in the buffers of st and tail (set-up fills it in)
  DevArray<double> d0, x0;              // staging for padded systems (N not a multiple of m) / in-place calls / chain order
  // element-chain order (AGGMG_COARSE_DEVICE_CHAIN, setup_cr_chain): the blocks are those of this chain form, N = ne * m is
  // the length of the BLOCK-ordered vectors, and a solve gathers its right-hand side through chain->perm into d0 and
  // scatters x0 back through chain->inv; null: the blocks are the operator's own rows
  std::shared_ptr<CgtDev> chain;
  DevArray<unsigned int> ticket;        // last-arriving-workgroup counter of the fused forward + tail launch
  double cond_est = 0.0;
  // the tail's system by parallel cyclic reduction (cr_pcr_tail_kernel; block sizes 1, 2, up to 1024 blocks -- above 512
  // the parallel part takes the even rows, one ordinary reduction level around it): multipliers
  // of every (level, row), final diagonal blocks factored
  struct Pcr {
    bool valid = false;
    bool pre = false;   // one ordinary cyclic-reduction level of the tail's first level around the parallel part
    int n = 0, L = 0;
    DevArray<double> mult, lu;
    DevArray<int32_t> perm;
  } pcr;
  // set-up only: copies of the (a, b, c) blocks of the small levels, until the plan says which one the tail starts at
  struct Raw {
    int level;
    int64_t n;
    DevArray<double> a, b, c;
  };
  std::vector<Raw> raw;
};

// One column-major matrix of a K-column run: column 0 and the doubles between two columns -- the one way the K-column
// code passes a pointer with its stride.  at(c0): the columns from c0 on (of a null view: a null view).
template <class T>
struct Cols {
  T* p = nullptr;
  int64_t ld = 0;
  Cols(T* p_ = nullptr, int64_t ld_ = 0) : p(p_), ld(ld_) {}
  template <class U, class = std::enable_if_t<std::is_same<const U, T>::value>>
  Cols(Cols<U> o) : p(o.p), ld(o.ld) {}   // what is written may be read
  Cols at(int64_t c0) const { return p ? Cols(p + c0 * ld, ld) : Cols(); }
};
using ColsIn = Cols<const double>;
using ColsOut = Cols<double>;

// The vectors level k of a K-column cycle keeps in h->mu[k] (multi_workspace allocates the ones the level has)
struct LevelCols {
  DevArray<double> u;     // the pre-smoothed iterate; on the coarsest level the solution
  DevArray<double> up;    // the post-smoothed iterate, levels 1 .. n-2 (level 0 writes the caller's X)
  DevArray<double> rhs;   // the right-hand side, levels >= 1 (level 0 reads the caller's B)
  DevArray<double> aux;   // patch levels: the prolonged iterate in front of the post sweeps; second vector of a chunked run
};

struct aggmg_hier {
  std::vector<Level> lv;
  int coarse_mode = 0;
  BandedLU coarse;
  CrDev cr;
  DevArray<double> cyc[2];  // iterate ping-pong for multi-cycle calls (lazy)
  DevArray<double> io[3];   // x0, b, x_out of the host-pointer entry aggmg_vcycle (lazy)
  // K-column cycles (aggmg_vcycle_multi_dev; multi_workspace: lazy, grown to the largest column group asked for): per
  // level, multi_cols columns of each vector the level has, multi_ld(h, k) doubles apart
  std::vector<LevelCols> mu;
  int64_t multi_cols = 0;
  // the coarsest solve of a column group in one launch sequence (cr_run_cols; lazy, grown like mu): per column of the
  // group what a CrStage holds for one (partR / partL / xq, stack, mid of every stage, the tail's mid) in ONE zeroed
  // allocation, and -- only when a call needs them -- the padded staging vectors d0 / x0 of every column in another
  DevArray<double> crw;
  int64_t crw_cols = 0;
  DevArray<double> crw_stage;
  int64_t crw_stage_cols = 0;
  int restriction = 0;  // AGGMG_RESTRICT_EXPLICIT (default) / AGGMG_RESTRICT_PRECONDITIONED
  // The replayed cycle (AGGMG_OPT_REPLAY_PRESMOOTH) leaves no pre-smoothed iterate in lv[0].u[0], and one caller can see
  // that: an ascent of its own (aggmg_vcycle_up_dev, aggmg_vcycle_up_split_dev) after a whole aggmg_vcycle_dev reads the
  // iterate that cycle's descent stored.  So a hierarchy on which a half-cycle entry point has been called keeps storing
  // (halves_used, for good), and an ascent on its own after a replayed cycle is refused instead of reading what is not
  // there (fine_iterate_absent: set by a replayed cycle, cleared by every descent that stores).
  bool halves_used = false, fine_iterate_absent = false;
  std::vector<double> h_coarse;
  double last_coarse_ms = 0.0;
  double cr_probe_backward_error = -1.0;  // ||d - A CR(d)|| / ||d|| of the set-up probe (-1: no device factorisation tried)
};

// The restricted residual L'(b - A u) is formed from r = b - A u evaluated with the operator's own
// entries (the reference's arithmetic, src/solvers.jl:36) -- AGGMG_RESTRICT_EXPLICIT, the default of
// every new hierarchy.  AGGMG_RESTRICT_PRECONDITIONED takes it from the sweeps' preconditioned
// residual instead, (L'D) w with w = g - P u- - Q u+ - u, which reads neither the diagonal blocks nor
// L: equal in exact arithmetic, but w inherits the rounding of the stored block inverses.  On the
// smoothest mode of the model problem that error grows like n^2 and at 2^24 fine elements turns the
// cycle from damping (x0.5, as in reference-order arithmetic) into amplifying (x2.1): measured,
// include/aggmg_hip.h and DESIGN.md section 5 -- aggmg_hier_set_restriction therefore refuses it above
// AGGMG_RESTRICT_PRECONDITIONED_MAX_ELEMS fine elements.
inline int default_restriction() { return AGGMG_RESTRICT_EXPLICIT; }

// How level k of a hierarchy runs its half of a cycle -- the one place that reads it off the level's fields.  Whether a
// given launch has a tile depends on the sweep counts as well: the half-cycle functions ask that, call by call.
enum class LevelPath {
  Coarsest,     // solved, not smoothed
  FusedChain,   // CG chain form + structured transfer: cgt_down / cgt_up / cgt_mid (cgt.hip)
  FusedBtd,     // block-tridiagonal form + structured transfer: btd_down / btd_up / btd_mid
  BtdTransfer,  // block-tridiagonal sweeps, generic residual / restriction / prolongation (the same three functions)
  Patch,        // fused element-patch Schwarz sweeps, zero-sweep fused transfer launches or the generic ones: patch_down / patch_up
  Generic       // generic_down / generic_up
};
// the element-block form a level's structured transfer is built on: the block-Jacobi smoother's, or the patch smoother's
inline const BtdDev* level_btd(const Level& l) {
  if (!l.S || l.S->A != l.A) return nullptr;
  if (l.S->btd) return l.S->btd.get();
  return l.S->patch ? l.S->patch->btd.get() : nullptr;
}
inline LevelPath level_path(const aggmg_hier* h, int k) {
  const Level& l = h->lv[k];
  if (k == (int)h->lv.size() - 1) return LevelPath::Coarsest;
  if (l.cgt_fused) return LevelPath::FusedChain;
  if (l.S && l.S->patch && l.S->A == l.A) return LevelPath::Patch;
  if (l.S && l.S->btd && l.S->A == l.A) return l.tb ? LevelPath::FusedBtd : LevelPath::BtdTransfer;
  return LevelPath::Generic;
}

// ---- the vectors of the K-column cycle (aggmg_vcycle_multi_dev) ------------------------------
// The column stride of level k's vectors in h->mu[k]: multi_workspace sizes them with it, every half-cycle reads and
// writes them with it, the level above included (its restricted residuals, the result it prolongs from).  It is Nalloc.
// aggmg_hier_create sets Nalloc = N on every level and raises it -- to the block-ordered length, the padding rows of the
// trailing block included -- only where the level's smoother has a chain form on the level's own operator: never on the
// coarsest level, which has no smoother.  The set-ups build a chain form only for a smoother with neither a
// block-tridiagonal nor a patch form, so level_path sends such a level to FusedChain or to Generic, and multi_ok accepts it
// as FusedChain alone.  On an accepted hierarchy, then, Nalloc == N on every block-tridiagonal, patch and coarsest level
// (their kernels address N rows per column) and Nalloc is the block-ordered length on every chain level (whose kernels
// address that many, and want the padding rows zero).
inline int64_t multi_ld(const aggmg_hier* h, int k) { return h->lv[k].Nalloc; }
inline ColsOut multi_vec(const aggmg_hier* h, int k, DevArray<double> LevelCols::*v) {
  return ColsOut((h->mu[k].*v).get(), multi_ld(h, k));
}
// the tail MultiArgs and CgtMultiArgs share: the columns of the launch, the column strides of its vectors (null view: none)
template <class Args>
inline void multi_strides(Args& m, int kc, ColsIn uin, ColsIn rhs, ColsOut uout, ColsIn uc, ColsOut rc) {
  m.kc = kc;
  m.ld_uin = uin.ld, m.ld_b = rhs.ld, m.ld_uout = uout.ld, m.ld_uc = uc.ld, m.ld_rc = rc.ld;
}
// Which vectors level k of a cycle on the caller's X0 (null: zero guesses), B and X uses: the K-column counterparts of
// rhs, uin, dst and coarse_result of the single-column driver -- the one place that knows level 0 and the coarsest apart
inline ColsIn multi_rhs(const aggmg_hier* h, int k, ColsIn B) { return k == 0 ? B : ColsIn(multi_vec(h, k, &LevelCols::rhs)); }
inline ColsIn multi_uin(int k, ColsIn X0) { return k == 0 ? X0 : ColsIn(); }   // u[k] = zeros for k > 1 (src/solvers.jl:29-31)
inline ColsOut multi_dst(const aggmg_hier* h, int k, ColsOut X) { return k == 0 ? X : multi_vec(h, k, &LevelCols::up); }
inline ColsIn multi_coarse_result(const aggmg_hier* h, int k) {   // what level k prolongs from
  return multi_vec(h, k + 1, k + 1 == (int)h->lv.size() - 1 ? &LevelCols::u : &LevelCols::up);
}

// A slot of the context's shared vectors for `who` (a string literal), held until *lease goes out of scope.  A slot that
// is held already is a defect of the library, not of the caller: the entry point fails instead of sharing the memory.
template <int NSLOT>
inline int lease_work(aggmg_ctx* ctx, WorkVectors<NSLOT>& w, const char* family, int slot, int64_t len, const char* who,
                      WorkLease* lease) {
  const WorkTake t = w.take(ctx, slot, len, who, lease);
  if (t.refused())
    return fail(ctx, AGGMG_ERR_UNSUPPORTED, std::string("internal: work vector ") + family + "[" + std::to_string(slot) +
                                                "] wanted by " + t.wanted_by + " is held by " + t.held_by);
  return t.code;
}
inline int scratch_lease(aggmg_ctx* ctx, ScratchSlot slot, int64_t len, const char* who, WorkLease* lease) {
  return lease_work(ctx, ctx->scratch, "scratch", slot, len, who, lease);
}
inline int solv_lease(aggmg_ctx* ctx, SolvSlot slot, int64_t len, const char* who, WorkLease* lease) {
  return lease_work(ctx, ctx->solv, "solv", slot, len, who, lease);
}

// ---------------------------------------------------------------------------------------------
// profiler (HIP events on the launch stream)
// ---------------------------------------------------------------------------------------------
// does any level carry a sweep-weight schedule?
inline bool any_schedule(const aggmg_hier* h) {
  for (const Level& l : h->lv)
    if (l.scheduled) return true;
  return false;
}

struct ProfScope {
  aggmg_ctx* ctx;
  int idx = -1;
  ProfScope(aggmg_ctx* c, int kind, int level) : ctx(c) {
    if (!ctx->profiling) return;
    if (ctx->profiling == 2 && !(kind == AGGMG_KIND_FUSED_DOWN && level == 0)) return;
    ProfEvent pe;
    for (hipEvent_t* e : {&pe.a, &pe.b}) {
      if (!ctx->ev_pool.empty()) {
        *e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
      } else if (hipEventCreateWithFlags(e, hipEventDisableSystemFence) != hipSuccess) {
        return;
      }
    }
    pe.tag = kind * 16 + (level & 15);
    (void)hipEventRecord(pe.a, ctx->stream);
    ctx->prof.push_back(pe);
    idx = (int)ctx->prof.size() - 1;
  }
  ~ProfScope() {
    if (idx >= 0) (void)hipEventRecord(ctx->prof[idx].b, ctx->stream);
  }
};


// ---------------------------------------------------------------------------------------------
// CG chain path (cgt.hip)
// ---------------------------------------------------------------------------------------------
int cgt_tile_blocks(int m);
// checkpoints of a chain launch (CgtArgs::chk_*): in -- after `sweep`, `sweep + stride`, ... sweeps and (`final`) after the
// last one, norms' partial sums to `part`, error against `exact` (caller's numbering, may be null); out -- the launch's
// tile count (the stride of `part` between checkpoints)
struct CgtChk {
  int sweep = 0, stride = 1 << 30, final = 0;
  const double* exact = nullptr;
  double* part = nullptr;
  int64_t cap = 0;      // tiles `part` has room for (per checkpoint): a launch of more is refused
  int64_t ntiles = 0;   // out: the tiles of the launch
};
int cgt_max_fused_sweeps(const CgtDev& g);   // sweeps one launch takes (point-Jacobi: + a residual or a closing checkpoint)
int cgt_build(aggmg_ctx* ctx, aggmg_smoother* sm, const int64_t* elems, int64_t m1, int64_t nel, int one_based);
int cgt_attach_schwarz(aggmg_ctx* ctx, aggmg_smoother* sm, int sw);
int cgt_build_transfer(aggmg_ctx* ctx, const aggmg_op* L, const CgtDev& fine, const CgtDev* coarse, int hint_mc,
                       TransferCgt* out, bool* ok);
// nsweeps sweeps on external (reference-numbered) vectors; u_in may be nullptr (zero), u_out != u_in
int cgt_smooth_ext(aggmg_ctx* ctx, const CgtDev& g, const double* u_in, const double* b, Damping alpha, int nsweeps,
                   double* u_out, int level, CgtChk* chk = nullptr);
int cgt_residual_ext(aggmg_ctx* ctx, const CgtDev& g, const double* u, const double* b, double* r_out);
int cgt_down(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* uin, const double* rhs, int nPre, double alpha);
int cgt_up(aggmg_ctx* ctx, aggmg_hier* h, int k, const double* rhs, int nPost, double alpha, double* dst,
           const double* src = nullptr, CgtChk* chk = nullptr);
int cgt_mid(aggmg_ctx* ctx, aggmg_hier* h, const double* cur, double* alt, const double* b, int nsweeps, double alpha,
            CgtChk* chk = nullptr);
// compulsory bytes (every array of the launch once) of a chain level's fused launches / of a stand-alone sweep or residual launch
int cgt_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, bool down, bool up, bool has_x0, int64_t* rd, int64_t* wr);
// K columns per launch (AGGMG_OPT_CHAIN_MULTI): the halves of a fused chain level of the K-column cycle, on the vectors of
// multi_workspace (h->mu); the argument list of every family's K-column halves
int cgt_multi_down(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn uin, ColsIn rhs, int nPre, double alpha, int kc);
int cgt_multi_up(aggmg_ctx* ctx, aggmg_hier* h, int k, ColsIn rhs, int nPost, double alpha, ColsOut dst, int kc);
int cgt_multi_launch_bytes(aggmg_ctx* ctx, const aggmg_hier* h, int level, bool down, bool has_x0, int64_t ncols, int64_t* rd, int64_t* wr);
int cgt_op_launch_bytes(const CgtDev& g, bool sweeps, int64_t* rd, int64_t* wr);

// ---------------------------------------------------------------------------------------------
// device-side set-up (setup.hip)
// ---------------------------------------------------------------------------------------------
int setup_csc_upload(aggmg_ctx* ctx, int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval,
                     const double* nzval, int one_based, CsrDev* out);
int op_ensure_csr(aggmg_ctx* ctx, aggmg_op* op);         // row-gather CSR + its CSR-stream row blocks
int setup_block_order(aggmg_ctx* ctx, aggmg_smoother* sm);   // blocks in ascending order of their smallest index, in place
int setup_block_cover(aggmg_ctx* ctx, aggmg_smoother* sm);   // row -> covering (block, local row) entries, on the device
int op_ensure_csc_blocks(aggmg_ctx* ctx, aggmg_op* op);  // CSR-stream row blocks of the transposed orientation
int op_host_csr(aggmg_ctx* ctx, aggmg_op* op, HostCsr* h);
int setup_jacobi_diag(aggmg_ctx* ctx, const aggmg_op* A, DevArray<double>* diag);
int setup_invert_blocks(aggmg_ctx* ctx, int64_t nb, int m, const double* blocks_dev, int colmajor, double* inv_dev,
                        int64_t* first_singular);
int setup_block_smoother(aggmg_ctx* ctx, aggmg_smoother* sm, const int64_t* blockinds, int one_based, int want_btd);
int setup_transfer_btd(aggmg_ctx* ctx, const aggmg_op* L, const BtdDev* Abtd, int mf, int64_t nef, int hint_mc,
                       TransferBtd* out, bool* ok);
// classes of identical per-element operator records of a fused level; *out stays null where the level does not take the
// form: other block sizes / packings, agglomerates of different sizes, more than kDictMaxClasses distinct records
int setup_op_dictionary(aggmg_ctx* ctx, const BtdDev& b, const TransferBtd& t, std::unique_ptr<DictDev>* out);
// the same for a level of the two-level launches (the caller has checked pair_level_ok: dense blocks of 2 rows, packed
// inverses, two-mode transfer of equal agglomerates)
int setup_pair_dictionary(aggmg_ctx* ctx, const BtdDev& b, const TransferBtd& t, std::unique_ptr<PairDictDev>* out);
// the same for a fused chain level: blocks of 1, 2 or 4 rows, point-Jacobi sweeps, chain or agglomerating transfer
int setup_cgt_dictionary(aggmg_ctx* ctx, const CgtDev& g, const TransferCgt& t, std::unique_ptr<CgtDictDev>* out);
// the same for the sweep launches of a fused element-patch Schwarz smoother: P.dict, or null where the smoother has more
// than kDictMaxClasses distinct records (the full arrays stay in either case)
int setup_patch_dictionary(aggmg_ctx* ctx, PatchDev& P);
// band_out (optional): max(i - j), max(j - i) over the stored entries -- what the host banded LU would have to store
int setup_cr(aggmg_ctx* ctx, const aggmg_op* Ac, int hint_m, CrDev* cr, int* band_out = nullptr);
int setup_cr_chain(aggmg_ctx* ctx, const CgtDev& g, CrDev* cr);   // the same factorisation of the chain-ordered blocks
int cgt_detect(aggmg_ctx* ctx, aggmg_smoother* sm);   // chain form from the operator's own pattern (no element lists)
// chunk-interleaved boundary rows of the element-partitioned coarsest solve (aggmg_hip.hip; used by dist.hip)
int coarse_chunk_forward_interleaved(aggmg_ctx* ctx, aggmg_hier* h, const double* rhs_owned, int64_t blk_lo, int64_t blk_hi, double* Z);
int coarse_boundary_solve_interleaved(aggmg_ctx* ctx, aggmg_hier* h, const double* Z, double* xq);
void cr_discard(CrDev* cr);                                                  // frees the factors, valid = false
int setup_probe_vector(aggmg_ctx* ctx, int64_t n, double* w);                // hash-random entries in [-1, 1)
int setup_smooth_vector(aggmg_ctx* ctx, int64_t n, double* w);               // 1 + cos(pi i / n) / 2
int setup_band_matvec_add(aggmg_ctx* ctx, const aggmg_op* A, int m, const double* x, double sign, double* y);  // y += sign A x, A block-tridiagonal (block size m), deterministic
