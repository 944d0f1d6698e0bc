// pmvs_devbuf.h -- the one owner type of a device array: DevBuf<T> holds a hipMalloc'ed pointer and its
// capacity in elements, frees in its destructor, moves but does not copy, and converts to T* so that
// it is passed to kernels and HIP calls like the raw pointer.  Its four (re)allocation forms differ
// in their growth rule only; the rule a call site uses decides the peak memory at full scale.
// CallArena is the owner of the device memory one API call needs for its own duration, and Staging
// decides, per output array of such a call, between the caller's device pointer and a staging array
// that is copied back at the end.
// Needs nothing of HIP but hipMalloc / hipFree / hipMemset / hipMemcpyAsync / hipStreamSynchronize /
// hipDeviceSynchronize (tests/csrc/devbuf_test.cpp and staging_test.cpp run it on the host against a
// stub of those).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <vector>

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

// The device memory of one API call: arrays of any type, all freed when the call returns.  The work
// that uses them must have finished by then: the call synchronises its stream before it returns.
struct CallArena {
  std::vector<void*> ptrs;

  CallArena() = default;
  CallArena(const CallArena&) = delete;
  CallArena& operator=(const CallArena&) = delete;
  ~CallArena() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  // `count` elements (0 holds one element, as DevBuf::alloc), poisoned as DevBuf's.  On failure *p is null.
  template <class T>
  hipError_t alloc(T** p, size_t count) {
    void* v = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    const hipError_t e = hipMalloc(&v, bytes);
    if (e == hipSuccess) {
      poison_alloc(v, bytes);
      ptrs.push_back(v);
    }
    *p = static_cast<T*>(v);
    return e;
  }
};

// The output arrays of one call.  Per array: *d = the device pointer the pass writes -- null when the
// caller does not want the array (a null pointer), the caller's own pointer in device mode, an arena
// array otherwise, which finish() copies to the caller's.  Two kinds of array:
//   fixed   `count` elements, all written by the pass and all copied back (count 0 holds one element)
//   capped  rows * per_row elements, `rows` bounded by a cap of the caller's; the pass writes the first
//           rows of it and reports how many: wrote(part, n) cuts the copy-back of the arrays of `part`
//           to min(rows, n) rows.  At rows == 0 there is no staging array: *d is null, and the pass,
//           which was given the cap 0, writes nothing.
// T is the pass's element type and U the ABI's (int64_t for long long, uint8_t for unsigned char).
class Staging {
 public:
  Staging(CallArena& arena, bool device_mode) : arena_(arena), dev_(device_mode) {}

  template <class T, class U>
  hipError_t fixed(T** d, U* caller, size_t count) {
    return stage(d, caller, count, 1, 0, true);
  }
  template <class T, class U>
  hipError_t capped(T** d, U* caller, size_t rows, size_t per_row, int part) {
    return stage(d, caller, rows, per_row, part, false);
  }
  void wrote(int part, size_t rows) {
    for (Copy& c : copies_)
      if (c.part == part && rows < c.rows) c.rows = rows;
  }
  // Host mode: the copies back, then the stream is synchronised (the arena may be freed after it).
  // Device mode: nothing, unless the stage has scratch of its own in flight and asks for the wait.
  hipError_t finish(hipStream_t st, bool sync_in_device_mode = false) {
    for (const Copy& c : copies_) {
      const size_t bytes = c.rows * c.row_bytes;
      if (!bytes) continue;
      const hipError_t e = hipMemcpyAsync(c.dst, c.src, bytes, hipMemcpyDeviceToHost, st);
      if (e != hipSuccess) return e;
    }
    copies_.clear();
    return (!dev_ || sync_in_device_mode) ? hipStreamSynchronize(st) : hipSuccess;
  }

 private:
  struct Copy {
    void* dst;
    const void* src;
    size_t rows, row_bytes;
    int part;
  };
  template <class T, class U>
  hipError_t stage(T** d, U* caller, size_t rows, size_t per_row, int part, bool hold_one) {
    static_assert(sizeof(T) == sizeof(U), "the pass's element type and the ABI's");
    *d = nullptr;
    if (!caller) return hipSuccess;
    if (dev_) {
      *d = reinterpret_cast<T*>(caller);
      return hipSuccess;
    }
    if (!rows && !hold_one) return hipSuccess;
    const hipError_t e = arena_.alloc(d, rows * per_row);
    if (e == hipSuccess) copies_.push_back(Copy{caller, *d, rows, per_row * sizeof(T), part});
    return e;
  }
  CallArena& arena_;
  const bool dev_;
  std::vector<Copy> copies_;
};

}  // namespace pmvsdev
