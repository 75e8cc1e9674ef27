// Ownership rules of csrc/devbuf.h's Buf, on the CPU: the same template the library instantiates with hipMalloc /
// hipHostMalloc, here with a malloc policy that counts what is live and can be told to fail.  Built with the address
// and undefined-behaviour sanitizers by tests/test_devbuf.py; a double free or a leak ends the run there as well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "devbuf.h"

namespace {

int live = 0, allocs = 0, frees = 0;
bool fail_next = false;
std::vector<size_t> sizes;  // bytes of every successful allocation, in order

struct CountAlloc {
  static int alloc(void **p, size_t bytes) {
    if (fail_next) {
      fail_next = false;
      *p = nullptr;
      return 2;
    }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return 2;
    live++, allocs++;
    sizes.push_back(bytes);
    return 0;
  }
  static void free(void *p) {
    ::free(p);
    live--, frees++;
  }
};
template <class T> using TBuf = lsqr::Buf<T, CountAlloc>;

int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      failures++;                                                     \
    }                                                                 \
  } while (0)

// the growth helpers of the library, over the counting policy
template <class T> int ensure(TBuf<T> &b, size_t need) {  // lsqr_hip.hip: ensure
  const size_t n = lsqr::grow_double(b, need);
  return n ? b.alloc(n) : 0;
}
template <class T> int many_grow(TBuf<T> &b, size_t need) {  // many.h: many_grow
  const size_t n = lsqr::grow_quarter(b, need, 64);
  return n ? b.alloc(n) : 0;
}
int many_grow_pinned(TBuf<char> &b, size_t bytes) {  // many.h: many_grow_pinned
  const size_t n = lsqr::grow_quarter(b, bytes, 1 << 16);
  return n ? b.alloc(n) : 0;
}

struct Several {  // a context in small: nothing to remember at delete
  TBuf<double> a, b;
  TBuf<char> c[3];
  TBuf<int> never;
};

}  // namespace

int main() {
  {  // alloc, then destruction
    TBuf<double> b;
    CHECK(!b && b.get() == nullptr && b.cap() == 0);
    CHECK(b.alloc(10) == 0 && b && b.cap() == 10 && live == 1 && sizes.back() == 10 * sizeof(double));
    b[9] = 1.0;            // reads as the pointer it owns
    double *p = b;
    CHECK(p == b.get() && *(b + 9) == 1.0);
    CHECK(b.alloc(20) == 0 && b.cap() == 20 && live == 1);  // frees what it held
  }
  CHECK(live == 0 && allocs == 2 && frees == 2);

  {  // a failed alloc leaves the buffer empty and frees nothing twice
    TBuf<int> b;
    CHECK(b.alloc(4) == 0 && live == 1);
    fail_next = true;
    CHECK(b.alloc(8) != 0 && !b && b.cap() == 0 && live == 0);
    b.reset();
    CHECK(live == 0);
    fail_next = true;
    CHECK(b.alloc(8) != 0 && !b && b.cap() == 0 && live == 0);  // ... from empty as well
    CHECK(b.alloc(8) == 0 && b.cap() == 8 && live == 1);
  }
  CHECK(live == 0 && allocs == frees);

  {  // moves and swaps leave exactly one owner
    TBuf<int> a;
    CHECK(a.alloc(3) == 0);
    int *pa = a;
    TBuf<int> b(std::move(a));
    CHECK(!a && a.cap() == 0 && b.get() == pa && b.cap() == 3 && live == 1);
    TBuf<int> c;
    CHECK(c.alloc(5) == 0 && live == 2);
    int *pc = c;
    c = std::move(b);  // what c held is freed
    CHECK(!b && c.get() == pa && c.cap() == 3 && live == 1);
    TBuf<int> &self = c;
    c = std::move(self);
    CHECK(c.get() == pa && c.cap() == 3 && live == 1);
    std::swap(c, self);
    CHECK(c.get() == pa && c.cap() == 3 && live == 1);
    TBuf<int> d;
    CHECK(d.alloc(7) == 0);
    int *pd = d;
    std::swap(c, d);  // the records / survivors exchange of many_sequential.h
    CHECK(c.get() == pd && c.cap() == 7 && d.get() == pa && d.cap() == 3 && live == 2);
    (void)pc;
  }
  CHECK(live == 0 && allocs == frees);

  {  // reset is idempotent
    TBuf<char> b;
    b.reset();
    CHECK(b.alloc(1) == 0);
    b.reset();
    CHECK(!b && b.cap() == 0 && live == 0);
    b.reset();
    CHECK(live == 0);
  }

  {  // ensure: what is asked for, at least twice what is there
    TBuf<double> b;
    const size_t req[] = {100, 50, 100, 101, 150, 500, 0}, cap[] = {100, 100, 100, 200, 200, 500, 500};
    for (int i = 0; i < 7; i++) CHECK(ensure(b, req[i]) == 0 && b.cap() == cap[i]);
    fail_next = true;
    CHECK(ensure(b, 501) != 0 && !b && b.cap() == 0);
    CHECK(ensure(b, 10) == 0 && b.cap() == 10);
  }
  {  // many_grow: n + n / 4, at least 64 elements; an empty buffer is allocated even for n = 0
    TBuf<uint32_t> b;
    const size_t req[] = {0, 64, 65, 81, 82, 1000, 1250, 1251}, cap[] = {64, 64, 81, 81, 102, 1250, 1250, 1563};
    for (int i = 0; i < 8; i++) CHECK(many_grow(b, req[i]) == 0 && b.cap() == cap[i]);
    CHECK(sizes.back() == 1563 * sizeof(uint32_t));
  }
  {  // many_grow_pinned: bytes + bytes / 4, at least 64 KiB
    TBuf<char> b;
    const size_t req[] = {1, 65536, 65537, 81921, 81922}, cap[] = {65536, 65536, 81921, 81921, 102402};
    for (int i = 0; i < 5; i++) CHECK(many_grow_pinned(b, req[i]) == 0 && b.cap() == cap[i]);
  }
  CHECK(live == 0 && allocs == frees);

  {  // a struct of several buffers releases all of them on delete
    Several *s = new Several();
    CHECK(s->a.alloc(1) == 0 && s->b.alloc(2) == 0);
    for (auto &c : s->c) CHECK(c.alloc(3) == 0);
    CHECK(live == 5);
    delete s;
    CHECK(live == 0);
  }

  if (failures || live != 0 || allocs != frees) {
    printf("devbuf test FAILED: %d checks, live allocations %d (%d allocated, %d freed)\n", failures, live, allocs, frees);
    return 1;
  }
  printf("devbuf test ok: live allocations %d (%d allocated, %d freed)\n", live, allocs, frees);
  return 0;
}
