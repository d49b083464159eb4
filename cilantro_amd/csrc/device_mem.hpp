// device_mem.hpp -- who owns a device allocation.  The only file of csrc/ that calls hipMalloc / hipFree: every buffer of the
// library is a member or a local of one of the types below, so its lifetime is written once, where it is declared.
//   DevBuf<T>     move-only owner of one typed device array (alloc / ensure / reset)
//   SharedBuf<T>  the same reading interface, reference-counted: copies hold the SAME block, the last holder frees it
//   DevPool       the allocations of one call: freed together when the pool leaves scope
//   StreamGuard / EventGuard   a stream (drained first) / an event destroyed at scope exit
// The ownership logic is plain C++ over an allocator policy A { error_t, ok, oom, alloc(void**, bytes), free(void*) } -- the HIP one
// (HipAlloc, and the unsuffixed aliases) exists under hipcc only; tests/cpp/test_device_mem.cpp runs the same templates over malloc.
// None of these types is ever passed to a kernel: the structs kernels take (GridDev, IterArgs, TieDev ...) stay plain views the owners fill in.
#pragma once

#include <atomic>
#include <cstddef>
#include <memory>
#include <new>
#include <utility>
#include <vector>

namespace cilhip {

// live allocations / live bytes of the process, all policies together (cilhip_debug_live_allocations)
struct DevMemLive { std::atomic<unsigned long long> count{0}, bytes{0}; };
inline DevMemLive& dev_mem_live() { static DevMemLive live; return live; }

// the two functions every allocation and every free goes through.  A request for 0 bytes allocates a non-empty block.
template <class A> typename A::error_t dev_mem_alloc(void** p, size_t bytes) {
  *p = nullptr;
  const typename A::error_t e = A::alloc(p, bytes ? bytes : 16);
  if (e != A::ok) { *p = nullptr; return e; }
  dev_mem_live().count.fetch_add(1, std::memory_order_relaxed);
  dev_mem_live().bytes.fetch_add(bytes, std::memory_order_relaxed);
  return e;
}
template <class A> void dev_mem_free(void* p, size_t bytes) {
  if (!p) return;
  A::free(p);
  dev_mem_live().count.fetch_sub(1, std::memory_order_relaxed);
  dev_mem_live().bytes.fetch_sub(bytes, std::memory_order_relaxed);
}

template <class T, class A> class BasicDevBuf {
 public:
  using error_t = typename A::error_t;
  BasicDevBuf() = default;
  BasicDevBuf(const BasicDevBuf&) = delete;
  BasicDevBuf& operator=(const BasicDevBuf&) = delete;
  BasicDevBuf(BasicDevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  BasicDevBuf& operator=(BasicDevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~BasicDevBuf() { reset(); }

  // a fresh block of n elements (contents undefined); what was held is freed first.  On failure the buffer is empty.
  error_t alloc(size_t n) {
    reset();
    void* q = nullptr;
    const error_t e = dev_mem_alloc<A>(&q, n * sizeof(T));
    if (e == A::ok) { p_ = static_cast<T*>(q); cap_ = n; }
    return e;
  }
  // at least n elements: grows (contents are NOT carried over), never shrinks
  error_t ensure(size_t n) { return (p_ && n <= cap_) ? A::ok : alloc(n); }
  void reset() { dev_mem_free<A>(p_, cap_ * sizeof(T)); p_ = nullptr; cap_ = 0; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// Copies share one block; alloc / reset re-point THIS holder only (the others keep what they hold).
template <class T, class A> class BasicSharedBuf {
 public:
  using error_t = typename A::error_t;
  error_t alloc(size_t n) {
    b_.reset();
    std::shared_ptr<BasicDevBuf<T, A>> nb;
    try { nb = std::make_shared<BasicDevBuf<T, A>>(); } catch (const std::bad_alloc&) { return A::oom; }
    const error_t e = nb->alloc(n);
    if (e == A::ok) b_ = std::move(nb);
    return e;
  }
  // takes over a block somebody built as a plain DevBuf (left empty); on failure this holder is empty and the block freed
  error_t adopt(BasicDevBuf<T, A>&& b) {
    b_.reset();
    BasicDevBuf<T, A> mine(std::move(b));
    try { b_ = std::make_shared<BasicDevBuf<T, A>>(std::move(mine)); } catch (const std::bad_alloc&) { return A::oom; }
    return A::ok;
  }
  void reset() { b_.reset(); }
  T* get() const { return b_ ? b_->get() : nullptr; }
  operator T*() const { return get(); }
  size_t capacity() const { return b_ ? b_->capacity() : 0; }
  long holders() const { return b_.use_count(); }

 private:
  std::shared_ptr<BasicDevBuf<T, A>> b_;
};

template <class A> class BasicDevPool {
 public:
  using error_t = typename A::error_t;
  BasicDevPool() = default;
  BasicDevPool(const BasicDevPool&) = delete;
  BasicDevPool& operator=(const BasicDevPool&) = delete;
  ~BasicDevPool() { clear(); }
  void clear() { for (const auto& b : blocks_) dev_mem_free<A>(b.first, b.second); blocks_.clear(); }
  // *out = n elements of T, owned by the pool (null on failure)
  template <class T> error_t get(T** out, size_t n) { return bytes(out, n * sizeof(T)); }
  template <class T> error_t bytes(T** out, size_t nbytes) {
    void* q = nullptr;
    *out = nullptr;
    try { blocks_.reserve(blocks_.size() + 1); } catch (const std::bad_alloc&) { return A::oom; }
    const error_t e = dev_mem_alloc<A>(&q, nbytes);
    if (e == A::ok) { blocks_.emplace_back(q, nbytes); *out = static_cast<T*>(q); }
    return e;
  }
  size_t size() const { return blocks_.size(); }

 private:
  std::vector<std::pair<void*, size_t>> blocks_;
};

}  // namespace cilhip

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace cilhip {
struct HipAlloc {
  using error_t = hipError_t;
  static constexpr hipError_t ok = hipSuccess, oom = hipErrorOutOfMemory;
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
template <class T> using DevBuf = BasicDevBuf<T, HipAlloc>;
template <class T> using SharedBuf = BasicSharedBuf<T, HipAlloc>;
using DevPool = BasicDevPool<HipAlloc>;

// a stream a stateless call created: drained, then destroyed.  Declare it AFTER the buffers its work uses (destroyed before them).
struct StreamGuard {
  hipStream_t s = nullptr;
  StreamGuard() = default;
  StreamGuard(const StreamGuard&) = delete;
  StreamGuard& operator=(const StreamGuard&) = delete;
  ~StreamGuard() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
  hipError_t create(unsigned flags = hipStreamNonBlocking) { return hipStreamCreateWithFlags(&s, flags); }
  operator hipStream_t() const { return s; }
};
struct EventGuard {
  hipEvent_t e = nullptr;
  EventGuard() = default;
  EventGuard(const EventGuard&) = delete;
  EventGuard& operator=(const EventGuard&) = delete;
  ~EventGuard() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return hipEventCreate(&e); }
  operator hipEvent_t() const { return e; }
};
}  // namespace cilhip
#endif
