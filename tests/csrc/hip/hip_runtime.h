// Host stub of the few HIP calls cmvs-pmvs_amd/csrc/pmvs_devbuf.h makes (tests/csrc/devbuf_test.cpp, staging_test.cpp):
// device memory is malloc'ed host memory, every live allocation is recorded, freeing an address that
// is not live (a double free) is counted, and the next allocation can be made to fail.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <set>

typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };

struct HipStub {
  std::set<void*> live;
  long allocs = 0, bad_frees = 0, syncs = 0;
  size_t last_bytes = 0;
  bool fail_next = false;
};
inline HipStub& hip_stub() {
  static HipStub s;
  return s;
}

inline hipError_t hipMalloc(void** p, size_t bytes) {
  HipStub& s = hip_stub();
  if (s.fail_next) {
    s.fail_next = false;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  memset(*p, 0x11, bytes);  // never the poison byte of the test, never zero
  s.live.insert(*p);
  s.allocs++;
  s.last_bytes = bytes;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  HipStub& s = hip_stub();
  if (!s.live.erase(p)) {
    s.bad_frees++;
    return hipErrorInvalidValue;
  }
  free(p);
  return hipSuccess;
}
inline hipError_t hipMemset(void* p, int v, size_t bytes) {
  memset(p, v, bytes);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t bytes, hipMemcpyKind, hipStream_t) {
  memcpy(d, s, bytes);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  hip_stub().syncs++;
  return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
