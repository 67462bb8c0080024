// One owner per device resource.  LsdOwned<V, Release> holds one value — a pointer or an opaque handle — and hands it to
// Release::call exactly once: when the owner dies, is reset or is assigned over.  Move-only.  Every kind of resource (= every Release)
// keeps a process-wide count of the values its owners hold, so a test can ask whether anything was left behind
// (lsdhip_live_resources).  Plain C++17 without HIP headers: tests/cpp/owned_test.cpp compiles it with fake release functions;
// lsdhip_internal.hpp instantiates it for device memory, pinned memory, events and streams.
#pragma once
#include <atomic>
#include <utility>

template <class Release> struct LsdLive {
  static inline std::atomic<long long> count{0};
};

template <class V, class Release> class LsdOwned {
  V v_{};
  static void counted(const V& v, long long d) { if (v) LsdLive<Release>::count.fetch_add(d, std::memory_order_relaxed); }

 public:
  LsdOwned() = default;
  explicit LsdOwned(V v) : v_(v) { counted(v_, +1); }
  LsdOwned(const LsdOwned&) = delete;
  LsdOwned& operator=(const LsdOwned&) = delete;
  LsdOwned(LsdOwned&& o) noexcept : v_(o.v_) { o.v_ = V{}; }     // (the value changes hands: the count stays)
  LsdOwned& operator=(LsdOwned&& o) noexcept {
    if (this != &o) { reset(); v_ = o.v_; o.v_ = V{}; }
    return *this;
  }
  ~LsdOwned() { reset(); }
  // releases what is held, then holds v
  void reset(V v = V{}) {
    V old = v_;
    v_ = v;
    counted(v_, +1);
    if (old) { counted(old, -1); (void)Release::call(old); }
  }
  // hands the value to the caller, who owns it from here on
  V release() { V v = v_; v_ = V{}; counted(v, -1); return v; }
  V get() const { return v_; }
  operator V() const { return v_; }
  V operator->() const { return v_; }
  explicit operator bool() const { return v_ ? true : false; }
};
