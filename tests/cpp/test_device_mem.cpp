// Host-only check of cilantro_amd/csrc/device_mem.hpp: the owners of device allocations, instantiated over a counting allocator
// backed by malloc that can be told to fail its k-th request.  Every case ends with the process-wide live count / live bytes back at
// their starting values and every block the allocator handed out freed exactly once.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#ifndef DEVICE_MEM_HEADER
#define DEVICE_MEM_HEADER "../../cilantro_amd/csrc/device_mem.hpp"
#endif
#include DEVICE_MEM_HEADER

using namespace cilhip;

static int g_fail = 0;
static std::string g_what;
#define CHECK(cond) do { if (!(cond)) { if (g_fail < 40) std::printf("FAIL line %d [%s]: %s\n", __LINE__, g_what.c_str(), #cond); ++g_fail; } } while (0)

struct TestAlloc {
  using error_t = int;
  static constexpr int ok = 0, oom = 2;
  static std::map<void*, int> freed;      // block -> times freed (0 while live)
  static int requests, fail_at, allocs, frees, double_frees, foreign_frees;
  static size_t last_bytes;
  static int alloc(void** p, size_t bytes) {
    ++requests;
    if (requests == fail_at) return oom;
    *p = std::malloc(bytes);
    if (!*p) return oom;
    freed[*p] = 0; ++allocs; last_bytes = bytes;
    return ok;
  }
  static void free(void* p) {
    auto it = freed.find(p);
    if (it == freed.end()) { ++foreign_frees; return; }
    if (it->second++) { ++double_frees; return; }      // (malloc may hand the address out again: a freed block leaves the map below)
    ++frees;
    std::free(p);
    freed.erase(it);
  }
  static void begin(int fail_k = 0) { requests = 0; fail_at = fail_k; }
  static int live() { return allocs - frees; }
};
std::map<void*, int> TestAlloc::freed;
int TestAlloc::requests = 0, TestAlloc::fail_at = 0, TestAlloc::allocs = 0, TestAlloc::frees = 0, TestAlloc::double_frees = 0, TestAlloc::foreign_frees = 0;
size_t TestAlloc::last_bytes = 0;

using Buf = BasicDevBuf<double, TestAlloc>;
using Shared = BasicSharedBuf<float, TestAlloc>;
using Pool = BasicDevPool<TestAlloc>;

// brackets one case: nothing live before, nothing live after, nothing freed twice
struct Case {
  unsigned long long count0, bytes0;
  explicit Case(const char* name) : count0(dev_mem_live().count.load()), bytes0(dev_mem_live().bytes.load()) { g_what = name; TestAlloc::begin(); CHECK(TestAlloc::live() == 0); }
  ~Case() {
    CHECK(dev_mem_live().count.load() == count0);
    CHECK(dev_mem_live().bytes.load() == bytes0);
    CHECK(TestAlloc::live() == 0);
    CHECK(TestAlloc::double_frees == 0);
    CHECK(TestAlloc::foreign_frees == 0);
  }
  unsigned long long count() const { return dev_mem_live().count.load() - count0; }
  unsigned long long bytes() const { return dev_mem_live().bytes.load() - bytes0; }
};

static void test_ensure() {
  Case k("ensure");
  Buf b;
  CHECK(b.get() == nullptr && b.capacity() == 0);
  CHECK(b.ensure(100) == 0);
  double* p = b.get();
  CHECK(p != nullptr && b.capacity() == 100 && (double*)b == p);
  CHECK(k.count() == 1 && k.bytes() == 100 * sizeof(double));
  const int frees = TestAlloc::frees, allocs = TestAlloc::allocs;
  CHECK(b.ensure(100) == 0 && b.get() == p);      // at capacity
  CHECK(b.ensure(7) == 0 && b.get() == p);        // below it
  CHECK(b.ensure(0) == 0 && b.get() == p && b.capacity() == 100);
  CHECK(TestAlloc::frees == frees && TestAlloc::allocs == allocs);
  CHECK(b.ensure(101) == 0);      // above: a new block, the old one freed once
  CHECK(b.get() != nullptr && b.capacity() == 101);
  CHECK(TestAlloc::frees == frees + 1 && TestAlloc::allocs == allocs + 1);
  CHECK(k.count() == 1 && k.bytes() == 101 * sizeof(double));
  CHECK(b.alloc(5) == 0 && b.capacity() == 5);      // alloc is always fresh, smaller too
  CHECK(TestAlloc::frees == frees + 2 && k.bytes() == 5 * sizeof(double));
}

static void test_zero() {
  Case k("zero elements");
  Buf a, b;
  CHECK(a.alloc(0) == 0 && a.get() != nullptr && a.capacity() == 0);
  CHECK(TestAlloc::last_bytes > 0);
  CHECK(b.ensure(0) == 0 && b.get() != nullptr);
  double* p = b.get();
  CHECK(b.ensure(0) == 0 && b.get() == p);
  CHECK(k.count() == 2 && k.bytes() == 0);
  Pool pool;
  int* q = nullptr;
  CHECK(pool.get(&q, 0) == 0 && q != nullptr);
}

static void test_failure() {
  Case k("failed allocation");
  Buf b;
  TestAlloc::begin(1);
  CHECK(b.alloc(10) == TestAlloc::oom && b.get() == nullptr && b.capacity() == 0);
  CHECK(k.count() == 0);
  TestAlloc::begin();
  CHECK(b.alloc(10) == 0);
  const int frees = TestAlloc::frees;
  TestAlloc::begin(1);
  CHECK(b.ensure(20) == TestAlloc::oom);      // the old block goes (once), nothing replaces it
  CHECK(b.get() == nullptr && b.capacity() == 0 && TestAlloc::frees == frees + 1);
  CHECK(k.count() == 0 && k.bytes() == 0);
  b.reset();
  CHECK(TestAlloc::frees == frees + 1);
  TestAlloc::begin();
  CHECK(b.alloc(3) == 0);
  TestAlloc::begin(1);
  CHECK(b.alloc(3) == TestAlloc::oom && b.get() == nullptr && b.capacity() == 0 && TestAlloc::frees == frees + 2);
  Shared s;
  TestAlloc::begin();
  CHECK(s.alloc(4) == 0 && s.get() != nullptr);
  TestAlloc::begin(1);
  CHECK(s.alloc(8) == TestAlloc::oom && s.get() == nullptr && s.capacity() == 0);
  CHECK(k.count() == 0);
}

static void test_reset_and_move() {
  Case k("reset / move");
  Buf a;
  a.reset(); a.reset();
  CHECK(a.alloc(9) == 0);
  a.reset();
  CHECK(a.get() == nullptr && a.capacity() == 0 && k.count() == 0);
  a.reset();
  CHECK(a.alloc(9) == 0);
  double* p = a.get();
  const int frees = TestAlloc::frees;
  Buf b(std::move(a));
  CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 9 && TestAlloc::frees == frees);
  Buf c;
  CHECK(c.alloc(2) == 0);
  c = std::move(b);      // the destination's own block goes, the moved one does not
  CHECK(b.get() == nullptr && c.get() == p && c.capacity() == 9 && TestAlloc::frees == frees + 1);
  CHECK(k.count() == 1 && k.bytes() == 9 * sizeof(double));
  Buf& self = c;
  c = std::move(self);
  CHECK(c.get() == p && TestAlloc::frees == frees + 1);
}

static void test_shared() {
  int order[3] = {0, 1, 2};
  do {
    Case k("shared owner");
    Shared h[3];
    CHECK(h[0].alloc(32) == 0);
    float* p = h[0].get();
    h[1] = h[0];
    h[2] = h[1];      // a borrower lends on
    CHECK(h[1].get() == p && h[2].get() == p && h[2].capacity() == 32 && h[0].holders() == 3);
    CHECK(k.count() == 1 && k.bytes() == 32 * sizeof(float));
    const int frees = TestAlloc::frees;
    for (int i = 0; i < 3; ++i) {
      CHECK(TestAlloc::frees == frees && k.count() == 1);
      for (int j = i; j < 3; ++j) CHECK(h[order[j]].get() == p);
      h[order[i]].reset();
      CHECK(h[order[i]].get() == nullptr && h[order[i]].capacity() == 0);
      h[order[i]].reset();
    }
    CHECK(TestAlloc::frees == frees + 1 && k.count() == 0);
  } while (std::next_permutation(order, order + 3));
  {
    Case k("shared owner: re-assignment");
    Shared a, b, c;
    CHECK(a.alloc(8) == 0 && c.alloc(16) == 0);
    b = a;
    float *pa = a.get(), *pc = c.get();
    const int frees = TestAlloc::frees;
    b = c;      // lets go of a's block, which a still holds
    CHECK(TestAlloc::frees == frees && a.get() == pa && b.get() == pc && a.holders() == 1 && c.holders() == 2);
    a = c;      // the last holder of pa re-assigned: freed now
    CHECK(TestAlloc::frees == frees + 1 && k.count() == 1);
    CHECK(b.alloc(4) == 0);      // a holder that allocates anew leaves the others what they have
    CHECK(b.get() != pc && a.get() == pc && c.get() == pc && k.count() == 2);
  }
  {
    Case k("shared owner: adopting a plain buffer");
    BasicDevBuf<float, TestAlloc> plain;
    CHECK(plain.alloc(12) == 0);
    float* p = plain.get();
    Shared a, b;
    CHECK(a.alloc(3) == 0);
    const int frees = TestAlloc::frees;
    CHECK(a.adopt(std::move(plain)) == 0);      // a's own block goes, the adopted one moves without a copy
    CHECK(plain.get() == nullptr && a.get() == p && a.capacity() == 12 && TestAlloc::frees == frees + 1 && k.count() == 1);
    b = a;
    a.reset();
    CHECK(b.get() == p && TestAlloc::frees == frees + 1);
  }
}

static int pool_user(int fail_k, int* got) {
  Pool pool;
  TestAlloc::begin(fail_k);
  for (int i = 0; i < 5; ++i) {
    float* p = nullptr;
    if (int e = pool.get(&p, 10 + i)) { if (p) *got = -1000; return e; }      // early return: the pool frees what it has
    ++*got;
  }
  return 0;
}

static void test_pool() {
  Case k("pool");
  int got = 0;
  {
    Pool pool;
    float* a = nullptr; unsigned char* b = nullptr;
    CHECK(pool.get(&a, 10) == 0 && pool.bytes(&b, 33) == 0 && a && b && pool.size() == 2);
    CHECK(k.count() == 2 && k.bytes() == 10 * sizeof(float) + 33);
  }
  CHECK(k.count() == 0 && k.bytes() == 0);
  CHECK(pool_user(0, &got) == 0 && got == 5 && TestAlloc::live() == 0);
  got = 0;
  const int frees = TestAlloc::frees;
  CHECK(pool_user(3, &got) == TestAlloc::oom && got == 2);
  CHECK(TestAlloc::frees == frees + 2 && TestAlloc::live() == 0);
}

int main() {
  test_ensure();
  test_zero();
  test_failure();
  test_reset_and_move();
  test_shared();
  test_pool();
  if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
