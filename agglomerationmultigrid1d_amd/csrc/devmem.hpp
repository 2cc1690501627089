// DevArray<T>: the one owner of a device allocation.  Every device array the library owns -- members of the objects
// behind the handles, the context's grow-on-demand work space, set-up temporaries -- is one of these, so that a forgotten
// free or a double free cannot be written.  The owner never synchronises except in reserve(): whoever frees an array a
// launch may still read synchronises first, as before (aggmg_*_free, aggmg_destroy).
//
// The runtime calls come in through the Mem policy: HipMem (below, HIP compilations only) for the library, a malloc /
// free stand-in for the host unit test (tests/host/test_devmem.cpp).  A policy names the context type and has
//   allocate(ctx, void**, bytes)  release(ctx, void*)  sync(ctx)  zero(ctx, void*, bytes)  copy_in(ctx, dst, src, bytes)
// each returning 0 or the library's error code; ctx is null where a destructor frees.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

struct HipMem;

// what the owners of this process hold at the moment (aggmg_debug_device_memory)
struct DevMemLive {
  static inline std::atomic<int64_t> allocations{0};
  static inline std::atomic<int64_t> bytes{0};
};

template <typename T, typename Mem = HipMem>
class DevArray {
 public:
  using Ctx = typename Mem::Ctx;
  DevArray() = default;
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  DevArray(DevArray&& o) noexcept : p_(o.p_), n_(o.n_) { o.forget(); }
  DevArray& operator=(DevArray&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = o.p_;
      n_ = o.n_;
      o.forget();
    }
    return *this;
  }
  ~DevArray() { (void)reset(); }

  operator T*() const { return p_; }   // implicit on purpose: kernel argument structs are built from the members
  T* get() const { return p_; }
  int64_t size() const { return n_; }  // elements asked for (the allocation holds at least one)

  // a fresh allocation of max(count, 1) elements, zeroed on the context's stream if asked; frees what was held
  int alloc(Ctx* ctx, int64_t count, bool zero = false) {
    if (int st = reset(ctx)) return st;
    const size_t b = bytes_of(count);
    void* p = nullptr;
    if (int st = Mem::allocate(ctx, &p, b)) return st;
    p_ = static_cast<T*>(p);
    n_ = count;
    DevMemLive::allocations += 1;
    DevMemLive::bytes += (int64_t)b;
    return zero ? Mem::zero(ctx, p_, b) : 0;
  }
  // grow only: nothing when size() >= count; else waits for the stream (a launch may read the old array), frees, allocates
  int reserve(Ctx* ctx, int64_t count, bool zero = false) {
    if (n_ >= count) return 0;
    if (p_)
      if (int st = Mem::sync(ctx)) return st;
    return alloc(ctx, count, zero);
  }
  // a host vector's copy; returns once it has arrived
  int upload(Ctx* ctx, const std::vector<T>& h) {
    if (int st = alloc(ctx, (int64_t)h.size())) return st;
    if (!h.empty())
      if (int st = Mem::copy_in(ctx, p_, h.data(), h.size() * sizeof(T))) return st;
    return Mem::sync(ctx);
  }
  int reset(Ctx* ctx = nullptr) {
    if (!p_) return 0;
    T* p = release();
    return Mem::release(ctx, p);
  }
  // hands the allocation to the caller, who frees it
  T* release() {
    T* p = p_;
    if (p) {
      DevMemLive::allocations -= 1;
      DevMemLive::bytes -= (int64_t)bytes_of(n_);
    }
    forget();
    return p;
  }

 private:
  static size_t bytes_of(int64_t count) { return (size_t)std::max<int64_t>(count, 1) * sizeof(T); }
  void forget() {
    p_ = nullptr;
    n_ = 0;
  }
  T* p_ = nullptr;
  int64_t n_ = 0;
};

#ifdef __HIPCC__
// the device: hipMalloc / hipFree, the context's stream; errors through HIPCHK (internal.hpp, which includes this header)
struct HipMem {
  using Ctx = aggmg_ctx;
  static int allocate(aggmg_ctx* ctx, void** p, size_t bytes) {
    HIPCHK(hipMalloc(p, bytes));
    return AGGMG_OK;
  }
  static int release(aggmg_ctx* ctx, void* p) {
    if (!ctx) return hipFree(p) == hipSuccess ? AGGMG_OK : AGGMG_ERR_HIP;
    HIPCHK(hipFree(p));
    return AGGMG_OK;
  }
  static int sync(aggmg_ctx* ctx) {
    HIPCHK(hipStreamSynchronize(stream_of(ctx)));
    return AGGMG_OK;
  }
  static int zero(aggmg_ctx* ctx, void* p, size_t bytes) {
    HIPCHK(hipMemsetAsync(p, 0, bytes, stream_of(ctx)));
    return AGGMG_OK;
  }
  static int copy_in(aggmg_ctx* ctx, void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream_of(ctx)));
    return AGGMG_OK;
  }
  static hipStream_t stream_of(aggmg_ctx* ctx);   // ctx->stream (aggmg_ctx is complete only further down internal.hpp)
};
#endif
