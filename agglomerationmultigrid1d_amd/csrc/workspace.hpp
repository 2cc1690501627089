// The context's shared work space: vectors that are leased, scalars that are named.
//
// DevArray (devmem.hpp) says who OWNS an array; WorkVectors says who is USING one of the context's shared vectors at the
// moment.  A function takes a slot with take() and holds the Lease for as long as it uses the pointer; a second take of a
// held slot is refused, with both names, instead of handing out the same memory -- or, worse, growing it, which frees
// what the first holder still points into.  A context is not thread-safe by contract, so a holder is a plain pointer:
// no pool, no search for a free slot, no atomics.  The slots stay numbered, so every buffer keeps the size its users
// ask for.  Host-compilable like devmem.hpp (same Mem policy, no HIP types): tests/host/test_workspace.cpp.
#pragma once
#include "devmem.hpp"

// the use of one slot, move-only; converts to the slot's pointer, gives the slot back when it goes out of scope
class WorkLease {
 public:
  WorkLease() = default;
  WorkLease(const WorkLease&) = delete;
  WorkLease& operator=(const WorkLease&) = delete;
  WorkLease(WorkLease&& o) noexcept : p_(o.p_), holder_(o.holder_) { o.forget(); }
  WorkLease& operator=(WorkLease&& o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_;
      holder_ = o.holder_;
      o.forget();
    }
    return *this;
  }
  ~WorkLease() { release(); }
  operator double*() const { return p_; }
  double* get() const { return p_; }
  bool held() const { return holder_ != nullptr; }
  void release() {
    if (holder_) *holder_ = nullptr;
    forget();
  }

 private:
  template <int NSLOT, typename Mem>
  friend class WorkVectors;
  void forget() {
    p_ = nullptr;
    holder_ = nullptr;
  }
  double* p_ = nullptr;
  const char** holder_ = nullptr;   // the slot's entry of WorkVectors::holder_, which outlives every lease (the context)
};

// what take() answers: the Mem policy's error code of the reserve, or a refusal that names both parties
struct WorkTake {
  int code = 0;
  const char* held_by = nullptr;    // non-null: refused, nothing reserved
  const char* wanted_by = nullptr;
  bool refused() const { return held_by != nullptr; }
};

template <int NSLOT, typename Mem = HipMem>
class WorkVectors {
 public:
  using Ctx = typename Mem::Ctx;
  // slot `slot` with room for `count` doubles (grow only; DevArray::reserve waits for the stream before it frees);
  // `who` is a string literal
  WorkTake take(Ctx* ctx, int slot, int64_t count, const char* who, WorkLease* lease) {
    if (holder_[slot]) return WorkTake{0, holder_[slot], who};
    if (int st = a_[slot].reserve(ctx, count)) return WorkTake{st, nullptr, who};
    lease->release();
    holder_[slot] = who;
    lease->p_ = a_[slot];
    lease->holder_ = &holder_[slot];
    return WorkTake{};
  }
  const char* holder(int slot) const { return holder_[slot]; }
  int64_t size(int slot) const { return a_[slot].size(); }

 private:
  DevArray<double, Mem> a_[NSLOT];
  const char* holder_[NSLOT] = {};
};

// ---- the two families of the context ------------------------------------------------------------------------------------
// ctx->solv, the outer loops' vectors.  A loop holds its slots from its prologue to its return; what it calls may take
// the others.
//
//   slot       | aggmg_pcg_dev | K-column loops (N K) | multigrid / smoother solve        | others
//   -----------+---------------+----------------------+-----------------------------------+----------------------------------
//   kSolvR     | r             | R                    | residual_norm's r (per check)     | aggmg_residual_norm_dev
//   kSolvZ     | z             | pcg Z, multigrid Xa  | the alternate iterate (ping-pong) |
//   kSolvP     | p             | pcg P, multigrid Xb  | chk_buffers: tile sums of the     |
//              |               |                      | checkpoint launches + their `mid` |
//   kSolvQ     | q             | pcg Q, multigrid Bw  |                                   |
//   kSolvZero  | zero rhs      | residual_multi's zero rhs (column-by-column branch, B null) | aggmg_fgmres_dev's zero rhs
enum SolvSlot : int { kSolvR = 0, kSolvZ = 1, kSolvP = 2, kSolvQ = 3, kSolvZero = 4, kSolvSlots = 5 };

// ctx->scratch, the smoothers' temporaries.  smooth_dev holds one slot while the runner below it takes the other two.
//
//   slot          | users
//   --------------+--------------------------------------------------------------------------------------------------------
//   kScratchPing  | btd_smooth: chunk chain (runs of more sweeps than a launch takes); cgt_smooth_ext: the same (t0);
//                 | cgt_mid: t1 of a run of more than two launches; smooth_dev: the generic sweeps' second vector
//   kScratchPong  | btd_smooth: chunk chain of more than two launches; cgt_smooth_ext: t1; generic_sweep: the block results
//                 | Y of the one-pass sweep, r of the four-launch form; aggmg_smoother_apply: the block results (overlapping)
//   kScratchStage | generic_sweep: y of the four-launch form; smooth_dev: the target of an in-place call on a fused form
enum ScratchSlot : int { kScratchPing = 0, kScratchPong = 1, kScratchStage = 2, kScratchSlots = 3 };

// ---- named scalars ------------------------------------------------------------------------------------------------------
struct ScalarRange {
  int at, n;
};
constexpr int kChkMax = 16;   // the most checkpoints one launch forms (chk_collect reads 2 kChkMax norms back)

// ctx->solv_sc (kSolvScalars doubles).  Values a later kernel reads stay in their own places; whatever the host reads
// back at once passes through kScReadBack (reduce_read), which nothing can touch before the value is on the host.
constexpr ScalarRange kScPcg{0, 3};          // aggmg_pcg_dev: [0] rz  [1] p.q  [2] rz_new
constexpr ScalarRange kScMgChk{8, 2};        // aggmg_multigrid_dev's checkpoint: ||A x - b||, ||x - u_exact||
constexpr ScalarRange kScLambda{10, 2};      // aggmg_hier_estimate_lambda_max: ||w||, ||v|| of the last step
constexpr ScalarRange kScReadBack{12, 1};    // reduce_read: ||b||, residual and error norms, aggmg_dot_dev / aggmg_norm2_dev
constexpr ScalarRange kScSmChk{16, 2 * kChkMax};   // aggmg_smoother_solve_dev's checkpoints of a launch, two norms each
constexpr int kSolvScalars = 48;

// ctx->cols_sc: kColsScalars rows of cols_cap columns (cols_sc(ctx, row))
enum ColsScalar : int { kColRz = 0, kColPq = 1, kColRzNew = 2, kColRes = 3, kColErr = 4, kColNormB = 5, kColsUsed = 6 };
constexpr int kColsScalars = 8;

template <int N>
constexpr bool scalar_ranges_fit(const ScalarRange (&t)[N], int total) {
  int end = 0;
  for (int i = 0; i < N; ++i) {   // ascending and disjoint
    if (t[i].n < 1 || t[i].at < end) return false;
    end = t[i].at + t[i].n;
  }
  return end <= total;
}
constexpr ScalarRange kSolvScalarTable[] = {kScPcg, kScMgChk, kScLambda, kScReadBack, kScSmChk};
static_assert(scalar_ranges_fit(kSolvScalarTable, kSolvScalars), "solv_sc: the named ranges overlap or leave the allocation");
static_assert(kScSmChk.at + kScSmChk.n == kSolvScalars, "solv_sc ends with the smoother solve's checkpoints");
static_assert(kScMgChk.n == 2 && kScSmChk.n == 2 * kChkMax, "two norms per checkpoint");
static_assert(kColsUsed <= kColsScalars, "cols_sc: a named row past the allocation");
