// devbuf.h -- owning buffers and events of the host code.
// A buffer that is a member of a context (or of a batched call's buffer set) is freed because it is a member: there
// is no list of frees to keep in step with the declarations.  Buf itself knows nothing of HIP -- the allocator is a
// policy -- so that its ownership rules are tested on the CPU (tests/cpp/devbuf_test.cpp) with a counting malloc.
#pragma once
#include <cstddef>
#include <utility>

namespace lsqr {

// T: element type.  Alloc: { static E alloc(void **p, size_t bytes); static void free(void *p); } where E is an error
// code whose zero value means success (hipError_t).  The capacity is in elements.
template <class T, class Alloc>
struct Buf {
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~Buf() { reset(); }

  void reset() {
    if (p_) Alloc::free(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // frees what is held, then allocates exactly n elements; on failure the buffer is empty
  auto alloc(size_t n) {
    reset();
    void *p = nullptr;
    auto e = Alloc::alloc(&p, sizeof(T) * n);
    if (e == decltype(e){}) {
      p_ = static_cast<T *>(p);
      cap_ = n;
    }
    return e;
  }
  T *get() const { return p_; }
  size_t cap() const { return cap_; }
  // launches, copies and pointer arithmetic read a buffer as the pointer it owns
  operator T *() const { return p_; }
  T *operator->() const { return p_; }

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};

// The growth rules of the three kinds of user.  Each returns the element count to allocate, or 0 when the buffer
// already serves `need`.
//   grow_double: the context's buffers (ensure): what is asked for, at least twice what is there
//   grow_quarter: the batched calls' device buffers (many_grow): a quarter of head room, at least 64 elements;
//                 their pinned buffers (many_grow_pinned) likewise in bytes, at least 64 KiB.  An EMPTY buffer gets
//                 that least size even for need == 0: assign_grouped_rounds relies on it for its empty lists
template <class B>
size_t grow_double(const B &b, size_t need) {
  if (need <= b.cap() && b.get()) return 0;
  return need > b.cap() * 2 ? need : b.cap() * 2;
}
template <class B>
size_t grow_quarter(const B &b, size_t need, size_t least) {
  if (need <= b.cap() && b.get()) return 0;
  size_t want = need + need / 4;
  return want < least ? least : want;
}

}  // namespace lsqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace lsqr {

struct DevAlloc {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void *p) { (void)hipFree(p); }
};
template <unsigned Flags>
struct PinAlloc {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
  static void free(void *p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = Buf<T, DevAlloc>;
template <class T> using PinBuf = Buf<T, PinAlloc<hipHostMallocDefault>>;
template <class T> using PinBufCoherent = Buf<T, PinAlloc<hipHostMallocCoherent>>;  // polled while a kernel writes it

struct Event {
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event &operator=(Event &&o) noexcept {
    if (this != &o) {
      reset();
      e_ = std::exchange(o.e_, nullptr);
    }
    return *this;
  }
  ~Event() { reset(); }
  void reset() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    return hipEventCreateWithFlags(&e_, flags);
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace lsqr
#endif
