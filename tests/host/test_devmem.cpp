// Host-compiled unit test of the device-memory owner (agglomerationmultigrid1d_amd/csrc/devmem.hpp) over malloc / free,
// under AddressSanitizer + UBSan: a double free or a use after free aborts, a lost allocation fails the leak check at exit.
#include "../../agglomerationmultigrid1d_amd/csrc/devmem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <typename T>
using Arr = DevArray<T, HostMem>;

// the std::vector<Level> pattern: a struct of owners (and an array of them) held by value in a vector
struct LevelLike {
  Arr<double> u[2], rhs;
  Arr<int32_t> idx;
  int64_t n = 0;
};

#define REQUIRE(cond)                                                  \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int64_t live_n() { return DevMemLive::allocations.load(); }
static int64_t live_b() { return DevMemLive::bytes.load(); }

int main() {
  HostCtx ctx;
  REQUIRE(live_n() == 0 && live_b() == 0);
  {
    // empty, alloc, the lower bound of one element, zeroing
    Arr<double> a;
    REQUIRE(!a && a.get() == nullptr && a.size() == 0);
    REQUIRE(a.alloc(&ctx, 5, true) == 0);
    REQUIRE(a && a.size() == 5 && live_n() == 1 && live_b() == 40);
    for (int i = 0; i < 5; ++i) REQUIRE(a[i] == 0.0);
    Arr<int32_t> z;
    REQUIRE(z.alloc(&ctx, 0) == 0);
    REQUIRE(z && z.size() == 0 && live_n() == 2 && live_b() == 44);
    z[0] = 7;   // (one element is there)

    // moves: construction empties the source; assignment onto a live buffer frees that buffer first
    double* pa = a;
    Arr<double> b(std::move(a));
    REQUIRE(!a && a.size() == 0 && b.get() == pa && b.size() == 5 && live_n() == 2);
    Arr<double> c;
    REQUIRE(c.alloc(&ctx, 3) == 0);
    REQUIRE(live_n() == 3 && live_b() == 68);
    c = std::move(b);
    REQUIRE(!b && c.get() == pa && c.size() == 5 && live_n() == 2 && live_b() == 44);
    Arr<double>& self = c;
    c = std::move(self);
    REQUIRE(c.get() == pa && c.size() == 5 && live_n() == 2);
    // alloc onto a live buffer frees it as well
    REQUIRE(c.alloc(&ctx, 2) == 0);
    REQUIRE(c.size() == 2 && live_n() == 2 && live_b() == 20);

    // reserve: grows (waiting for the stream only when something is held), and does nothing when the size suffices
    Arr<double> r;
    REQUIRE(r.reserve(&ctx, 0) == 0);
    REQUIRE(!r && ctx.syncs == 0);
    REQUIRE(r.reserve(&ctx, 4) == 0);
    REQUIRE(r.size() == 4 && ctx.syncs == 0 && live_n() == 3);
    double* pr = r;
    REQUIRE(r.reserve(&ctx, 4) == 0 && r.reserve(&ctx, 1) == 0);
    REQUIRE(r.get() == pr && r.size() == 4 && ctx.syncs == 0);
    REQUIRE(r.reserve(&ctx, 9, true) == 0);
    REQUIRE(r.size() == 9 && ctx.syncs == 1 && live_n() == 3 && live_b() == 20 + 72);
    for (int i = 0; i < 9; ++i) REQUIRE(r[i] == 0.0);

    // upload
    Arr<int32_t> up;
    REQUIRE(up.upload(&ctx, std::vector<int32_t>{3, 1, 4, 1, 5}) == 0);
    REQUIRE(up.size() == 5 && up[2] == 4 && up[4] == 5 && ctx.syncs == 2);
    REQUIRE(up.upload(&ctx, std::vector<int32_t>()) == 0);
    REQUIRE(up && up.size() == 0);

    // release hands the allocation over (no longer counted), reset frees
    const int64_t n0 = live_n(), b0 = live_b();
    double* raw = r.release();
    REQUIRE(raw && !r && r.size() == 0 && live_n() == n0 - 1 && live_b() == b0 - 72);
    raw[8] = 1.0;
    std::free(raw);
    REQUIRE(r.release() == nullptr && r.reset() == 0);
    REQUIRE(c.reset(&ctx) == 0);
    REQUIRE(!c && live_n() == n0 - 2);
    REQUIRE(c.reset() == 0);   // twice is harmless
  }
  REQUIRE(live_n() == 0 && live_b() == 0);
  {
    // a vector of structs holding owners: resize up (reallocation moves the elements), erase, resize down
    std::vector<LevelLike> lv;
    lv.resize(2);
    for (size_t k = 0; k < lv.size(); ++k) {
      lv[k].n = 10 + (int64_t)k;
      for (Arr<double>* p : {&lv[k].u[0], &lv[k].u[1], &lv[k].rhs}) REQUIRE(p->alloc(&ctx, lv[k].n, true) == 0);
      REQUIRE(lv[k].idx.alloc(&ctx, lv[k].n) == 0);
    }
    REQUIRE(live_n() == 8);
    double* keep = lv[1].rhs;
    lv.resize(40);
    REQUIRE(live_n() == 8 && lv[1].rhs.get() == keep && lv[1].n == 11 && !lv[39].rhs);
    REQUIRE(lv[39].u[1].alloc(&ctx, 3) == 0);
    lv.erase(lv.begin());          // move-assigns every later element one down
    REQUIRE(live_n() == 5 && lv[0].rhs.get() == keep && lv[0].n == 11 && lv[38].u[1].size() == 3);
    lv.resize(1);
    REQUIRE(live_n() == 4);
    std::vector<Arr<double>> owned(3);
    REQUIRE(owned[1].alloc(&ctx, 2) == 0);
    owned.clear();
    REQUIRE(live_n() == 4);
  }
  REQUIRE(live_n() == 0 && live_b() == 0);
  std::printf("devmem OK\n");
  return 0;
}
