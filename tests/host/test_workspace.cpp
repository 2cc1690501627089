// Host-compiled unit test of the leased work vectors (agglomerationmultigrid1d_amd/csrc/workspace.hpp) over malloc / free,
// under AddressSanitizer + UBSan: a pointer into a slot that was grown away under its holder aborts, a lost allocation
// fails the leak check at exit.  Including the header compiles the static_asserts of the two scalar tables.
#include "../../agglomerationmultigrid1d_amd/csrc/workspace.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

struct HostCtx {
  int syncs = 0;
};

struct HostMem {
  using Ctx = HostCtx;
  static int allocate(HostCtx*, void** p, size_t bytes) {
    *p = std::malloc(bytes);
    return *p ? 0 : 1;
  }
  static int release(HostCtx*, void* p) {
    std::free(p);
    return 0;
  }
  static int sync(HostCtx* c) {
    ++c->syncs;
    return 0;
  }
  static int zero(HostCtx*, void* p, size_t bytes) {
    std::memset(p, 0, bytes);
    return 0;
  }
  static int copy_in(HostCtx*, void* dst, const void* src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    return 0;
  }
};

using Work = WorkVectors<kSolvSlots, HostMem>;

#define REQUIRE(cond)                                                  \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int64_t live_n() { return DevMemLive::allocations.load(); }
static int64_t live_b() { return DevMemLive::bytes.load(); }

// the library's wrapper (internal.hpp: lease_work), with the message in place of fail()
static int lease(HostCtx* ctx, Work& w, int slot, int64_t n, const char* who, WorkLease* out, std::string* msg) {
  const WorkTake t = w.take(ctx, slot, n, who, out);
  if (t.refused()) {
    *msg = std::string("internal: work vector solv[") + std::to_string(slot) + "] wanted by " + t.wanted_by + " is held by " + t.held_by;
    return -1;
  }
  return t.code;
}

// takes two slots and leaves early, as a CHECK in the middle of an entry point does
static int early_return(HostCtx* ctx, Work& w, bool fail_midway, std::string* msg) {
  WorkLease a, b;
  if (int st = lease(ctx, w, kSolvR, 8, "early_return", &a, msg)) return st;
  if (fail_midway) return 7;
  if (int st = lease(ctx, w, kSolvZ, 8, "early_return", &b, msg)) return st;
  a[7] = b[7] = 1.0;
  return 0;
}

int main() {
  HostCtx ctx;
  std::string msg;
  REQUIRE(live_n() == 0 && live_b() == 0);
  {
    Work w;
    // take and release
    {
      WorkLease r;
      REQUIRE(!r.held() && r.get() == nullptr);
      REQUIRE(lease(&ctx, w, kSolvR, 5, "first", &r, &msg) == 0);
      REQUIRE(r.held() && r.get() != nullptr && w.size(kSolvR) == 5 && std::strcmp(w.holder(kSolvR), "first") == 0);
      REQUIRE(live_n() == 1 && live_b() == 40);
      r[4] = 2.0;
      // a second take of the held slot: refused, both parties named, nothing reserved (not even for a larger size)
      WorkLease again;
      REQUIRE(lease(&ctx, w, kSolvR, 500, "second", &again, &msg) == -1);
      REQUIRE(msg == "internal: work vector solv[0] wanted by second is held by first");
      REQUIRE(!again.held() && again.get() == nullptr && w.size(kSolvR) == 5 && live_b() == 40 && ctx.syncs == 0);
      REQUIRE(std::strcmp(w.holder(kSolvR), "first") == 0);
      r[4] = 3.0;   // (the first holder's pointer is still good)
      // the other slots are free
      REQUIRE(lease(&ctx, w, kSolvZ, 3, "second", &again, &msg) == 0);
      REQUIRE(again.held() && w.holder(kSolvZ) && live_n() == 2);
    }
    REQUIRE(w.holder(kSolvR) == nullptr && w.holder(kSolvZ) == nullptr);
    REQUIRE(live_n() == 2);   // (the vectors stay with the work space: grow only)
    {
      WorkLease r;
      REQUIRE(lease(&ctx, w, kSolvR, 5, "third", &r, &msg) == 0);
      REQUIRE(ctx.syncs == 0 && r[4] == 3.0);   // the same size: the same array, no wait
      r.release();
      REQUIRE(!r.held() && w.holder(kSolvR) == nullptr);
      r.release();   // twice is harmless
    }

    // a scope left through an early return gives its slots back
    REQUIRE(early_return(&ctx, w, true, &msg) == 7);
    REQUIRE(w.holder(kSolvR) == nullptr && w.holder(kSolvZ) == nullptr);
    REQUIRE(early_return(&ctx, w, false, &msg) == 0);
    REQUIRE(w.holder(kSolvR) == nullptr && w.holder(kSolvZ) == nullptr);

    // moves: the slot is released once, by whoever holds the lease last
    {
      WorkLease a;
      REQUIRE(lease(&ctx, w, kSolvP, 4, "mover", &a, &msg) == 0);
      double* pa = a;
      WorkLease b(std::move(a));
      REQUIRE(!a.held() && a.get() == nullptr && b.held() && b.get() == pa && w.holder(kSolvP) != nullptr);
      {
        WorkLease c;
        REQUIRE(lease(&ctx, w, kSolvQ, 4, "other", &c, &msg) == 0);
        c = std::move(b);   // assignment onto a live lease gives that one's slot back first
        REQUIRE(w.holder(kSolvQ) == nullptr && !b.held() && c.get() == pa && std::strcmp(w.holder(kSolvP), "mover") == 0);
        WorkLease& self = c;
        c = std::move(self);
        REQUIRE(c.get() == pa && w.holder(kSolvP) != nullptr);
      }
      REQUIRE(w.holder(kSolvP) == nullptr);   // c went out of scope; a and b, emptied, release nothing
      WorkLease d;
      REQUIRE(lease(&ctx, w, kSolvP, 4, "after", &d, &msg) == 0);
      REQUIRE(d.get() == pa);
    }
    REQUIRE(w.holder(kSolvP) == nullptr);
    // a lease that takes again gives its former slot back
    {
      WorkLease a;
      REQUIRE(lease(&ctx, w, kSolvP, 4, "one", &a, &msg) == 0);
      REQUIRE(lease(&ctx, w, kSolvQ, 4, "two", &a, &msg) == 0);
      REQUIRE(w.holder(kSolvP) == nullptr && std::strcmp(w.holder(kSolvQ), "two") == 0);
    }

    // growing one slot leaves the pointers into the other held slots valid; the wait is counted only when a
    // non-empty array grows
    {
      const int s0 = ctx.syncs;
      WorkLease h[kSolvSlots];
      for (int s = 0; s < kSolvSlots; ++s) REQUIRE(lease(&ctx, w, s, 6, "holder", &h[s], &msg) == 0);
      // R and Z hold 8 since early_return (nothing to do), P and Q grew 4 -> 6 (a wait each), Zero was empty (no wait)
      REQUIRE(ctx.syncs == s0 + 2);
      for (int i = 0; i < kSolvSlots; ++i) {
        h[i].release();
        const int s1 = ctx.syncs;
        REQUIRE(lease(&ctx, w, i, 6, "same", &h[i], &msg) == 0 && ctx.syncs == s1);          // enough: no wait
        h[i].release();
        REQUIRE(lease(&ctx, w, i, 4096 * (i + 1), "grower", &h[i], &msg) == 0 && ctx.syncs == s1 + 1);
        REQUIRE(w.size(i) == 4096 * (i + 1));
        for (int s = 0; s < kSolvSlots; ++s) {   // every held pointer, the grown one included, is written through
          const int64_t n = w.size(s);
          for (int64_t k = 0; k < n; ++k) h[s][k] = (double)(s + k);
          REQUIRE(h[s][n - 1] == (double)(s + n - 1));
        }
      }
    }
    for (int s = 0; s < kSolvSlots; ++s) REQUIRE(w.holder(s) == nullptr);
    REQUIRE(live_n() == kSolvSlots);
  }
  // the work space is gone, and with it every vector
  REQUIRE(live_n() == 0 && live_b() == 0);

  // the scalar tables (their static_asserts compiled with the header): the rows the loops name
  REQUIRE(kScSmChk.at + 2 * kChkMax == kSolvScalars && kScReadBack.n == 1 && kColNormB < kColsScalars);
  std::printf("workspace OK\n");
  return 0;
}
