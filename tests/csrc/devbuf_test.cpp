// Stand-alone check of DevBuf<T> (cmvs-pmvs_amd/csrc/pmvs_devbuf.h) against the host stub of HIP in
// tests/csrc/hip/hip_runtime.h; tests/test_devbuf.py builds and runs it.  Argument "poison": the run
// has PMVS_POISON_ALLOC=165 set and every new allocation must hold that byte; without it none does.
#include "pmvs_devbuf.h"

#include <cstdio>
#include <cstring>
#include <utility>

using pmvsdev::DevBuf;

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "devbuf_test:%d: %s\n", __LINE__, #c);      \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static const size_t kSizes[] = {0, 1, 5, 1000};
static unsigned char g_fill = 0x11;  // what new memory holds: the stub's fill, or the poison byte

static bool all_bytes(const void* p, size_t bytes, unsigned char v) {
  const unsigned char* c = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < bytes; ++i)
    if (c[i] != v) return false;
  return true;
}
static size_t max2(size_t a, size_t b) { return a > b ? a : b; }

static void test_alloc_and_grow() {
  HipStub& s = hip_stub();
  for (size_t n : kSizes) {
    DevBuf<int> b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.alloc(n) == hipSuccess);
    CHECK(b.p != nullptr && b.cap == n);
    CHECK(s.last_bytes == max2(n, 1) * sizeof(int));  // n == 0 holds one element
    CHECK(all_bytes(b.p, max2(n, 1) * sizeof(int), g_fill));
    int* raw = b;  // the implicit conversion kernels and HIP calls use
    CHECK(raw == b.p);
    // alloc always allocates anew, even the same size
    const long a0 = s.allocs;
    CHECK(b.alloc(n) == hipSuccess && s.allocs == a0 + 1 && b.cap == n);
    // exact grow: nothing at or below the capacity, exactly `need` above it
    for (size_t need : kSizes) {
      const long a1 = s.allocs;
      int* const before = b.p;
      const size_t cap = b.cap;
      CHECK(b.grow(need) == hipSuccess);
      if (need <= cap) {
        CHECK(s.allocs == a1 && b.p == before && b.cap == cap);
      } else {
        CHECK(s.allocs == a1 + 1 && b.cap == need && s.last_bytes == need * sizeof(int));
        CHECK(all_bytes(b.p, need * sizeof(int), g_fill));
      }
    }
  }
  // an empty buffer grows even to 0 elements (one element is allocated), and then stays
  DevBuf<double> e;
  const long a0 = s.allocs;
  CHECK(e.grow(0) == hipSuccess && e.p != nullptr && e.cap == 0 && s.allocs == a0 + 1 && s.last_bytes == sizeof(double));
  CHECK(e.grow(0) == hipSuccess && s.allocs == a0 + 1);
}

static void test_headroom() {
  HipStub& s = hip_stub();
  for (size_t c : kSizes)
    for (size_t need : kSizes) {
      DevBuf<short> b;
      CHECK(b.grow_headroom(c) == hipSuccess && b.cap == c);  // from empty: exactly the need
      const long a0 = s.allocs;
      short* const before = b.p;
      CHECK(b.grow_headroom(need) == hipSuccess);
      if (need <= c) {
        CHECK(s.allocs == a0 && b.p == before && b.cap == c);
      } else {
        const size_t want = max2(need, c + c / 4);
        CHECK(s.allocs == a0 + 1 && b.cap == want && s.last_bytes == max2(want, 1) * sizeof(short));
        CHECK(all_bytes(b.p, want * sizeof(short), g_fill));
      }
    }
  DevBuf<int> b;  // 1000 -> 1001: the 25 % of the old capacity win
  CHECK(b.grow_headroom(1000) == hipSuccess && b.grow_headroom(1001) == hipSuccess && b.cap == 1250);
}

static void test_grow_keep() {
  HipStub& s = hip_stub();
  for (size_t c : kSizes)
    for (size_t need : kSizes)
      for (size_t used : kSizes) {
        if (used > c) continue;
        DevBuf<int> b;
        CHECK(b.alloc(c) == hipSuccess);
        for (size_t i = 0; i < used; ++i) b.p[i] = (int)(7 * i + 3);
        const long a0 = s.allocs, y0 = s.syncs;
        int* const before = b.p;
        CHECK(b.grow_keep(need, used, nullptr) == hipSuccess);
        if (need <= c) {
          CHECK(s.allocs == a0 && b.p == before && b.cap == c);
        } else {
          const size_t want = max2(need, c + c / 2 + 1024);
          CHECK(s.allocs == a0 + 1 && b.cap == want && s.last_bytes == want * sizeof(int));
          CHECK(s.syncs == y0 + 1);  // the copy has finished before the old array is freed
          CHECK(all_bytes(b.p + used, (want - used) * sizeof(int), g_fill));
        }
        for (size_t i = 0; i < used; ++i) CHECK(b.p[i] == (int)(7 * i + 3));
      }
  // an empty buffer grows even for need 0, to the 1024 elements of the rule
  DevBuf<int> e;
  CHECK(e.grow_keep(0, 0, nullptr) == hipSuccess && e.p != nullptr && e.cap == 1024);
  // the free-function form on a raw pointer and capacity (the model the API owns)
  int* raw = nullptr;
  size_t cap = 0;
  CHECK(pmvsdev::grow_keep(raw, cap, 5, 0, nullptr) == hipSuccess && raw && cap == 1024);
  raw[0] = 41;
  raw[1] = 42;
  CHECK(pmvsdev::grow_keep(raw, cap, 5000, 2, nullptr) == hipSuccess && cap == 5000 && raw[0] == 41 && raw[1] == 42);
  CHECK(pmvsdev::grow_keep(raw, cap, 5001, 2, nullptr) == hipSuccess && cap == 5000 + 2500 + 1024 && raw[1] == 42);
  CHECK(hipFree(raw) == hipSuccess);
}

static void test_move_and_release() {
  HipStub& s = hip_stub();
  DevBuf<int> a;
  CHECK(a.alloc(5) == hipSuccess);
  int* const pa = a.p;
  DevBuf<int> b(std::move(a));
  CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 5);
  DevBuf<int> c;
  CHECK(c.alloc(1) == hipSuccess);
  const size_t live = s.live.size();
  c = std::move(b);  // the target's old array is freed, the source is left empty
  CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 5 && s.live.size() == live - 1);
  c.release();
  CHECK(c.p == nullptr && c.cap == 0 && s.live.size() == live - 2);
  c.release();  // idempotent
  a.release();
  CHECK(s.bad_frees == 0 && s.live.size() == live - 2);
  struct Two {
    DevBuf<int> x;
    DevBuf<float> y;
    int n = 0;
  } t;
  CHECK(t.x.alloc(5) == hipSuccess && t.y.alloc(1000) == hipSuccess);
  t.n = 3;
  t = Two();  // how the buffer structs release everything
  CHECK(t.x.p == nullptr && t.y.p == nullptr && t.n == 0 && s.live.size() == live - 2);
}

static void test_failure() {
  HipStub& s = hip_stub();
  for (int form = 0; form < 3; ++form) {
    DevBuf<int> b;
    CHECK(b.alloc(5) == hipSuccess);
    s.fail_next = true;
    const hipError_t e = form == 0 ? b.alloc(1000) : form == 1 ? b.grow(1000) : b.grow_headroom(1000);
    CHECK(e == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0);  // empty, the old array freed
    CHECK(b.grow(5) == hipSuccess && b.cap == 5);                     // and usable again
  }
  DevBuf<int> e;
  s.fail_next = true;
  CHECK(e.grow_keep(5, 0, nullptr) == hipErrorOutOfMemory && e.p == nullptr && e.cap == 0);
  // grow_keep allocates before it frees: a failure leaves the kept contents where they were
  DevBuf<int> k;
  CHECK(k.alloc(5) == hipSuccess);
  k.p[4] = 99;
  int* const before = k.p;
  s.fail_next = true;
  CHECK(k.grow_keep(1000, 5, nullptr) == hipErrorOutOfMemory && k.p == before && k.cap == 5 && k.p[4] == 99);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "poison")) g_fill = 165;
  test_alloc_and_grow();
  test_headroom();
  test_grow_keep();
  test_move_and_release();
  test_failure();
  CHECK(hip_stub().live.empty());  // every DevBuf above has freed its array
  CHECK(hip_stub().bad_frees == 0);
  if (g_fail) return 1;
  printf("devbuf ok: %ld allocations\n", hip_stub().allocs);
  return 0;
}
