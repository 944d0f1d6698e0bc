// pmvs_devbuf.h -- the one owner type of a device array: DevBuf<T> holds a hipMalloc'ed pointer and its
// capacity in elements, frees in its destructor, moves but does not copy, and converts to T* so that
// it is passed to kernels and HIP calls like the raw pointer.  Its four (re)allocation forms differ
// in their growth rule only; the rule a call site uses decides the peak memory at full scale.
// Needs nothing of HIP but hipMalloc / hipFree / hipMemset / hipMemcpyAsync / hipStreamSynchronize /
// hipDeviceSynchronize (tests/csrc/devbuf_test.cpp runs it on the host against a stub of those).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

namespace pmvsdev {

// Debug builds of the tests: PMVS_POISON_ALLOC=<byte> fills every new device allocation with that
// byte, so a read of memory no kernel wrote shows up as a result change (tests/test_gpu_poison.py).
inline void poison_alloc(void* p, size_t bytes) {
  static const int v = [] {
    const char* e = getenv("PMVS_POISON_ALLOC");
    return e ? atoi(e) : -1;
  }();
  if (v >= 0 && p && bytes) {
    (void)hipMemset(p, v & 0xff, bytes);
    (void)hipDeviceSynchronize();
  }
}

// Grows a raw device array keeping its first `used` elements (a model the API owns; DevBuf::grow_keep).
// 1.5x: old and new coexist during the copy, and at C5 scale the model alone is ~80 GB.
template <class T>
inline hipError_t grow_keep(T*& p, size_t& cap, size_t need, size_t used, hipStream_t st) {
  if (need <= cap && p) return hipSuccess;
  const size_t half = cap + cap / 2 + 1024;
  const size_t ncap = need > half ? need : half;
  T* q = nullptr;
  hipError_t e = hipMalloc((void**)&q, ncap * sizeof(T));
  if (e != hipSuccess) return e;
  poison_alloc(q, ncap * sizeof(T));
  if (p && used) e = hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(q);
    return e;
  }
  if (p) (void)hipFree(p);
  p = q;
  cap = ncap;
  return hipSuccess;
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements asked for (an allocation is never empty: alloc(0) holds one element)

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {  // the old array is freed, o is left empty
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p; }

  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // Exactly n elements, the old contents discarded (always a new allocation; n == 0 holds one element,
  // as the loop's allocation helpers did -- no caller in pmvs_api.cpp asks for 0).  On failure the
  // buffer is empty.  Every allocation is poisoned under PMVS_POISON_ALLOC, the hipcub temp storage and
  // the other buffers that were plain hipMalloc's included.
  hipError_t alloc(size_t n) {
    release();
    const size_t bytes = (n ? n : 1) * sizeof(T);
    const hipError_t e = hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    poison_alloc(p, bytes);
    cap = n;
    return hipSuccess;
  }
  // At least `need` elements, contents discarded when it grows: to exactly `need` ...
  hipError_t grow(size_t need) { return (need <= cap && p) ? hipSuccess : alloc(need); }
  // ... or with 25 % headroom over the old capacity (buffers that follow a slowly growing model)
  hipError_t grow_headroom(size_t need) {
    if (need <= cap && p) return hipSuccess;
    const size_t head = cap + cap / 4;
    return alloc(need > head ? need : head);
  }
  // At least `need` elements, the first `used` kept: max(need, cap + cap / 2 + 1024), copied on `st`,
  // which is synchronised before the old array is freed.  On failure the buffer is unchanged.
  hipError_t grow_keep(size_t need, size_t used, hipStream_t st) { return pmvsdev::grow_keep(p, cap, need, used, st); }
};

}  // namespace pmvsdev
