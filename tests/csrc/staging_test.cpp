// Stand-alone check of CallArena and Staging (cmvs-pmvs_amd/csrc/pmvs_devbuf.h), the call-scoped device
// memory and the output staging of the model-output calls, against the host stub of HIP in
// tests/csrc/hip/hip_runtime.h; tests/test_staging.py builds and runs it.  Argument "poison": the run has
// PMVS_POISON_ALLOC=165 set and every new allocation must hold that byte; without it none does.
#include "pmvs_devbuf.h"

#include <cstdio>
#include <cstring>

using pmvsdev::CallArena;
using pmvsdev::Staging;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "staging_test:%d: %s\n", __LINE__, #c);      \
      ++g_fail;                                                    \
    }                                                              \
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

static void test_arena() {
  HipStub& s = hip_stub();
  const size_t live = s.live.size();
  {
    CallArena a;
    size_t held = 0;
    for (size_t n : kSizes) {  // arrays of different types in one arena
      int* pi = nullptr;
      double* pd = nullptr;
      const long a0 = s.allocs;
      CHECK(a.alloc(&pi, n) == hipSuccess && pi && s.allocs == a0 + 1);
      CHECK(s.last_bytes == max2(n, 1) * sizeof(int));  // n == 0 holds one element
      CHECK(all_bytes(pi, max2(n, 1) * sizeof(int), g_fill));
      CHECK(a.alloc(&pd, n) == hipSuccess && pd && s.last_bytes == max2(n, 1) * sizeof(double));
      CHECK(all_bytes(pd, max2(n, 1) * sizeof(double), g_fill));
      held += 2;
      CHECK(s.live.size() == live + held && s.live.count(pi) && s.live.count(pd));
    }
  }
  CHECK(s.live.size() == live && s.bad_frees == 0);  // freed with the arena, once each
}

static void test_host_mode() {
  HipStub& s = hip_stub();
  const size_t live = s.live.size();
  {
    CallArena a;
    Staging g(a, false);
    for (size_t n : kSizes) {
      int host[1000];
      memset(host, 0x77, sizeof(host));
      int* d = nullptr;
      const long a0 = s.allocs;
      CHECK(g.fixed(&d, host, n) == hipSuccess);
      CHECK(d && d != host && s.live.count(d) && s.allocs == a0 + 1 && s.last_bytes == max2(n, 1) * sizeof(int));
      CHECK(all_bytes(d, max2(n, 1) * sizeof(int), g_fill));
      for (size_t i = 0; i < max2(n, 1); ++i) d[i] = (int)(3 * i + 1);
      // a NULL array is not wanted: NULL on the device, nothing allocated, nothing copied
      float* none = reinterpret_cast<float*>(&host);
      CHECK(g.fixed(&none, (float*)nullptr, n) == hipSuccess && none == nullptr && s.allocs == a0 + 1);
      const long y0 = s.syncs;
      CHECK(g.finish(nullptr) == hipSuccess && s.syncs == y0 + 1);
      for (size_t i = 0; i < n; ++i) CHECK(host[i] == (int)(3 * i + 1));
      CHECK(all_bytes(host + n, (1000 - n) * sizeof(int), 0x77));  // count 0: one element held, none copied
    }
    // 64-bit arrays of the ABI (int64_t) are long long on the device
    long host64[3] = {0, 0, 0};
    long long* d64 = nullptr;
    CHECK(g.fixed(&d64, host64, 3) == hipSuccess && d64);
    d64[0] = 1, d64[1] = -2, d64[2] = 1LL << 40;
    CHECK(g.finish(nullptr) == hipSuccess && host64[0] == 1 && host64[1] == -2 && host64[2] == (1L << 40));
  }
  CHECK(s.live.size() == live);
}

static void test_device_mode() {
  HipStub& s = hip_stub();
  CallArena a;
  Staging g(a, true);
  int caller[8];
  memset(caller, 0x77, sizeof(caller));
  const long a0 = s.allocs, y0 = s.syncs;
  int *d = nullptr, *c = nullptr, *z = nullptr;
  float* none = reinterpret_cast<float*>(&caller);
  CHECK(g.fixed(&d, caller, 8) == hipSuccess && d == caller);  // the caller's pointer, as it is
  CHECK(g.capped(&c, caller, 2, 3, 1) == hipSuccess && c == caller);
  CHECK(g.capped(&z, caller, 0, 3, 1) == hipSuccess && z == caller);  // at a zero cap too
  CHECK(g.fixed(&none, (float*)nullptr, 8) == hipSuccess && none == nullptr);
  g.wrote(1, 1);
  CHECK(g.finish(nullptr) == hipSuccess);
  CHECK(s.allocs == a0 && s.syncs == y0 && a.ptrs.empty());  // no allocation, no copy, no synchronisation
  CHECK(g.finish(nullptr, true) == hipSuccess && s.syncs == y0 + 1);  // unless the stage asks for it
  CHECK(all_bytes(caller, sizeof(caller), 0x77));
}

static void test_partial_copy_back() {
  HipStub& s = hip_stub();
  const size_t live = s.live.size();
  {
    CallArena a;
    Staging g(a, false);
    float vert[8 * 3], norm[8 * 3];
    int face[4 * 3];
    unsigned char map[6], skipped[4];
    memset(vert, 0x77, sizeof(vert));
    memset(norm, 0x77, sizeof(norm));
    memset(face, 0x77, sizeof(face));
    memset(map, 0x77, sizeof(map));
    memset(skipped, 0x77, sizeof(skipped));
    float *dv = nullptr, *dn = nullptr;
    int* df = nullptr;
    unsigned char *dm = nullptr, *dz = reinterpret_cast<unsigned char*>(&skipped);
    CHECK(g.capped(&dv, vert, 8, 3, 1) == hipSuccess && dv && s.last_bytes == 8 * 3 * sizeof(float));
    CHECK(g.capped(&dn, norm, 8, 3, 1) == hipSuccess && dn);
    CHECK(g.capped(&df, face, 4, 3, 2) == hipSuccess && df && s.last_bytes == 4 * 3 * sizeof(int));
    CHECK(g.fixed(&dm, map, 6) == hipSuccess && dm);
    const long a0 = s.allocs;
    CHECK(g.capped(&dz, skipped, 0, 3, 1) == hipSuccess && dz == nullptr && s.allocs == a0);  // a zero cap: NULL, no allocation
    for (int i = 0; i < 24; ++i) dv[i] = (float)i, dn[i] = (float)-i;
    for (int i = 0; i < 12; ++i) df[i] = 100 + i;
    for (int i = 0; i < 6; ++i) dm[i] = (unsigned char)i;
    g.wrote(1, 5);  // 5 of 8 vertices
    g.wrote(2, 9);  // more faces exist than the cap: the 4 that were written
    CHECK(g.finish(nullptr) == hipSuccess);
    for (int i = 0; i < 15; ++i) CHECK(vert[i] == (float)i && norm[i] == (float)-i);
    CHECK(all_bytes(vert + 15, 9 * sizeof(float), 0x77) && all_bytes(norm + 15, 9 * sizeof(float), 0x77));
    for (int i = 0; i < 12; ++i) CHECK(face[i] == 100 + i);
    for (int i = 0; i < 6; ++i) CHECK(map[i] == i);  // a fixed array is copied whole
    CHECK(all_bytes(skipped, sizeof(skipped), 0x77));
    // nothing written: nothing copied
    Staging h(a, false);
    float* dw = nullptr;
    memset(vert, 0x55, sizeof(vert));
    CHECK(h.capped(&dw, vert, 8, 3, 1) == hipSuccess && dw);
    h.wrote(1, 0);
    CHECK(h.finish(nullptr) == hipSuccess && all_bytes(vert, sizeof(vert), 0x55));
  }
  CHECK(s.live.size() == live);
}

// The shape of a stage: every array staged or the first error returned, the arena freeing what was made.
static hipError_t stage_three(int* h0, int* h1, int* h2, int fail_at) {
  HipStub& s = hip_stub();
  CallArena a;
  Staging g(a, false);
  int* d[3] = {nullptr, nullptr, nullptr};
  int* const h[3] = {h0, h1, h2};
  for (int k = 0; k < 3; ++k) {
    s.fail_next = k == fail_at;
    const hipError_t e = k == 1 ? g.capped(&d[k], h[k], 4, 1, 1) : g.fixed(&d[k], h[k], 4);
    if (e != hipSuccess) {
      CHECK(d[k] == nullptr);
      return e;
    }
    for (int i = 0; i < 4; ++i) d[k][i] = 10 * k + i;
  }
  return g.finish(nullptr);
}

static void test_failure() {
  HipStub& s = hip_stub();
  const size_t live = s.live.size();
  for (int fail_at = 0; fail_at < 3; ++fail_at) {
    int h[3][4];
    memset(h, 0x77, sizeof(h));
    CHECK(stage_three(h[0], h[1], h[2], fail_at) == hipErrorOutOfMemory);
    CHECK(s.live.size() == live && s.bad_frees == 0);  // nothing leaked, nothing freed twice
    CHECK(all_bytes(h, sizeof(h), 0x77));              // and nothing copied
  }
  int h[3][4];
  CHECK(stage_three(h[0], h[1], h[2], -1) == hipSuccess && h[2][3] == 23 && s.live.size() == live);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "poison")) g_fill = 165;
  test_arena();
  test_host_mode();
  test_device_mode();
  test_partial_copy_back();
  test_failure();
  CHECK(hip_stub().live.empty());  // every arena above has freed its arrays
  CHECK(hip_stub().bad_frees == 0);
  if (g_fail) return 1;
  printf("staging ok: %ld allocations\n", hip_stub().allocs);
  return 0;
}
