// pmvs_text.hip -- the .ply / .patch / .pset text of a model, formatted on the device
// (pmvs_loop_text / pmvs_text_patches, include/pmvs_amd.h).
//
// The rows are those of the export (pmvs_export.hip): the kernels read its device arrays -- fields,
// colours, list offsets and ids -- so the row order, index2image and the colours come from that code.
// Formatting is independent per row, and the file is one contiguous buffer:
//   *_len_kernel     every row's byte count (pmvs_fmt.h, nothing written)
//   hipcub scan      64-bit exclusive sums from the header's size: the rows' byte offsets
//   *_write_kernel   formats again into an LDS tile at the row's place, and consecutive lanes store the
//                    tile as aligned 32-bit words (single bytes at its two ends)
// .ply and .pset rows are short (10 and 6 tokens): one lane per row, a tile of 64 rows per wavefront.
// .patch rows carry up to 128 + 128 ids: one wavefront per row, as export_gather_kernel -- lanes 0-10
// format the 11 floats, lanes take list entries k, k + 64, and wave-wide prefix sums of the token
// lengths place them.
// The bytes are those of pmvs_write_ply / _patches / _pset (pmvs_io.cpp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "pmvs_device.h"
#include "pmvs_fmt.h"
#include "pmvs_launch.h"

namespace pmvsdev {
namespace {

#define TCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

using pmvsfmt::fmt_g_t;
using pmvsfmt::fmt_i32_t;
using pmvsfmt::kMaxFloatBytes;
using pmvsfmt::kMaxIntBytes;

constexpr int kTileRows = 64;  // rows of one .ply / .pset tile: one per lane of a wavefront
// longest rows: every token at its longest, its separator included
constexpr int kPlyRowMax = 7 * (kMaxFloatBytes + 1) + 3 * (kMaxIntBytes + 1);
constexpr int kPsetRowMax = 6 * (12 + 1);
constexpr int kPatchRowMax = 7 + 11 * (kMaxFloatBytes + 1) + 2 * (3 + 1) + 2 * (PMVS_MAX_IMAGES * (kMaxIntBytes + 1) + 1) + 1;

template <int KIND>
struct RowKind;
template <>
struct RowKind<PMVS_TEXT_PLY> {
  static constexpr int kTokens = 10, kPrecision = 17, kRowMax = kPlyRowMax;
};
template <>
struct RowKind<PMVS_TEXT_PSET> {
  static constexpr int kTokens = 6, kPrecision = 6, kRowMax = kPsetRowMax;
};

// One .ply row "x y z nx ny nz r g b quality\n" or .pset row "x y z nx ny nz\n" at out; returns its bytes.
template <int KIND, bool WRITE>
__device__ __forceinline__ int format_row(const float* __restrict__ f, const int* __restrict__ c, char* out) {
  int p = 0;
#pragma unroll 1
  for (int t = 0; t < RowKind<KIND>::kTokens; ++t) {
    if (t >= 6 && t < 9) {
      p += fmt_i32_t<WRITE>(c[t - 6], out + p);
    } else {
      const int k = t < 3 ? t : (t < 6 ? t + 1 : 8);  // coord xyz, normal xyz, ncc
      p += fmt_g_t<WRITE>(f[k], RowKind<KIND>::kPrecision, out + p);
    }
    if (WRITE) out[p] = t + 1 == RowKind<KIND>::kTokens ? '\n' : ' ';
    ++p;
  }
  return p;
}

// tile[pad, pad + total) -> dst[0, total) by `lanes` consecutive lanes; pad = dst's address & 3, so the
// LDS and the global side are aligned alike: whole 32-bit words in the middle, bytes at the ends.
__device__ __forceinline__ void flush_tile(const uint32_t* tile, int pad, int total, char* dst, int lane, int lanes) {
  const char* tb = reinterpret_cast<const char*>(tile);
  char* base = dst - pad;  // 4-aligned
  const int end = pad + total;
  const int w0 = (pad + 3) >> 2, w1 = end >> 2;  // whole words [w0, w1)
  const int head_end = w0 * 4 < end ? w0 * 4 : end;
  for (int i = pad + lane; i < head_end; i += lanes) base[i] = tb[i];
  for (int w = w0 + lane; w < w1; w += lanes) reinterpret_cast<uint32_t*>(base)[w] = tile[w];
  const int tail = w1 > w0 ? w1 * 4 : head_end;
  for (int i = tail + lane; i < end; i += lanes) base[i] = tb[i];
}

template <int KIND>
__global__ __launch_bounds__(256) void rows_len_kernel(const float* __restrict__ fields, const int* __restrict__ colors,
                                                       int n, long long* __restrict__ len) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += stride)
    len[r] = r == n ? 0 : format_row<KIND, false>(fields + r * 11, colors ? colors + r * 3 : nullptr, nullptr);
}

// One wavefront per block and 64 rows per tile; off[r] = row r's byte offset in out (n + 1 entries).
template <int KIND>
__global__ __launch_bounds__(kTileRows) void rows_write_kernel(const float* __restrict__ fields,
                                                                const int* __restrict__ colors, int n,
                                                                const long long* __restrict__ off, char* __restrict__ out) {
  __shared__ uint32_t tile[(kTileRows * RowKind<KIND>::kRowMax + 4 + 3) / 4];
  const int lane = threadIdx.x;
  const long long tiles = ((long long)n + kTileRows - 1) / kTileRows;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long row0 = t * kTileRows, r = row0 + lane;
    const long long rows = n - row0 < kTileRows ? n - row0 : kTileRows;
    const long long base = off[row0];
    const int total = (int)(off[row0 + rows] - base);
    const int pad = (int)(reinterpret_cast<uintptr_t>(out + base) & 3);
    if (r < n)
      format_row<KIND, true>(fields + r * 11, colors ? colors + r * 3 : nullptr,
                             reinterpret_cast<char*>(tile) + pad + (int)(off[r] - base));
    __syncthreads();
    flush_tile(tile, pad, total, out + base, lane, kTileRows);
    __syncthreads();
  }
}

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// The ids of one list, each followed by a space, from row + cur on, then '\n'; returns the new cur.
template <bool WRITE>
__device__ __forceinline__ int format_list(const int* __restrict__ ids, int cnt, char* row, int cur, int lane) {
  for (int base = 0; base < cnt; base += 64) {
    const int k = base + lane;
    const int id = k < cnt ? ids[k] : 0;
    const int mine = k < cnt ? fmt_i32_t<false>(id, nullptr) + 1 : 0;
    const int incl = wave_inclusive_sum(mine, lane);
    if (WRITE && k < cnt) {
      char* at = row + cur + incl - mine;
      at[fmt_i32_t<true>(id, at)] = ' ';
    }
    cur += __shfl(incl, 63);
  }
  if (WRITE && lane == 0) row[cur] = '\n';
  return cur + 1;
}

// One .patch record (Patch::operator<<) by one wavefront at row; every lane returns its byte count.
template <bool WRITE>
__device__ __forceinline__ int format_patch(const float* __restrict__ f, const int* __restrict__ ids, int ni,
                                            const int* __restrict__ vids, int nv, char* row, int lane) {
  float fv = 0.0f;
  int mine = 0;
  if (lane < 11) {
    fv = f[lane];
    mine = fmt_g_t<false>(fv, 17, nullptr) + 1;
  }
  const int incl = wave_inclusive_sum(mine, lane);
  if (WRITE) {
    if (lane < 7) row[lane] = "PATCHS\n"[lane];
    if (lane < 11) {
      char* at = row + 7 + incl - mine;
      at[fmt_g_t<true>(fv, 17, at)] = (lane == 3 || lane == 7 || lane == 10) ? '\n' : ' ';
    }
  }
  int cur = 7 + __shfl(incl, 63);
  int w = fmt_i32_t<false>(ni, nullptr);
  if (WRITE && lane == 0) row[cur + fmt_i32_t<true>(ni, row + cur)] = '\n';
  cur = format_list<WRITE>(ids, ni, row, cur + w + 1, lane);
  w = fmt_i32_t<false>(nv, nullptr);
  if (WRITE && lane == 0) row[cur + fmt_i32_t<true>(nv, row + cur)] = '\n';
  cur = format_list<WRITE>(vids, nv, row, cur + w + 1, lane);
  if (WRITE && lane == 0) row[cur] = '\n';
  return cur + 1;
}

__global__ __launch_bounds__(256) void patch_len_kernel(const float* __restrict__ fields, const long long* __restrict__ ioff,
                                                        const int* __restrict__ ids, const long long* __restrict__ voff,
                                                        const int* __restrict__ vids, int n, long long* __restrict__ len) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * (blockDim.x / 64);
  for (long long r = (long long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; r <= n; r += stride) {
    int bytes = 0;
    if (r < n) {
      const long long io = ioff[r], vo = voff[r];
      bytes = format_patch<false>(fields + r * 11, ids + io, (int)(ioff[r + 1] - io), vids + vo, (int)(voff[r + 1] - vo),
                                  nullptr, lane);
    }
    if (lane == 0) len[r] = bytes;
  }
}

constexpr int kPatchTileWords = (kPatchRowMax + 4 + 3) / 4;

__global__ __launch_bounds__(256) void patch_write_kernel(const float* __restrict__ fields, const long long* __restrict__ ioff,
                                                          const int* __restrict__ ids, const long long* __restrict__ voff,
                                                          const int* __restrict__ vids, int n,
                                                          const long long* __restrict__ off, char* __restrict__ out) {
  __shared__ uint32_t tiles[4][kPatchTileWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  const long long stride = (long long)gridDim.x * 4;
  const long long last = ((long long)n + stride - 1) / stride * stride;  // every wavefront of a block runs the same trips
  for (long long r = (long long)blockIdx.x * 4 + wave; r < last; r += stride) {
    const bool live = r < n;
    const long long base = live ? off[r] : 0;
    const int pad = (int)(reinterpret_cast<uintptr_t>(out + base) & 3);
    int total = 0;
    if (live) {
      const long long io = ioff[r], vo = voff[r];
      total = format_patch<true>(fields + r * 11, ids + io, (int)(ioff[r + 1] - io), vids + vo, (int)(voff[r + 1] - vo),
                                 reinterpret_cast<char*>(tiles[wave]) + pad, lane);
    }
    __syncthreads();
    if (live) flush_tile(tiles[wave], pad, total, out + base, lane, 64);
    __syncthreads();
  }
}

__global__ void format_selftest_kernel(int precision, const float* __restrict__ in, int n, char* __restrict__ out,
                                       int* __restrict__ len) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) len[i] = fmt_g_t<true>(in[i], precision, out + i * 24);
}

inline int text_grid(long long items, int per_block) {
  const long long g = (items + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > (1 << 16) ? (1 << 16) : g));
}

}  // namespace

hipError_t text_offsets(int kind, const TextArrays& in, int n, long long header_bytes, long long* d_off, hipStream_t st) {
  const int n1 = n + 1;
  DevBuf<long long> len;
  DevBuf<char> temp;
  size_t tb = 0;
  TCHK(len.alloc((size_t)n1));
  long long* const d_len = len.p;
  TCHK(hipcub::DeviceScan::ExclusiveScan(nullptr, tb, d_len, d_off, hipcub::Sum(), header_bytes, n1, st));
  TCHK(temp.alloc(tb));
  if (kind == PMVS_TEXT_PLY)
    hipLaunchKernelGGL(rows_len_kernel<PMVS_TEXT_PLY>, dim3(text_grid(n1, 256)), dim3(256), 0, st, in.fields, in.colors, n, d_len);
  else if (kind == PMVS_TEXT_PSET)
    hipLaunchKernelGGL(rows_len_kernel<PMVS_TEXT_PSET>, dim3(text_grid(n1, 256)), dim3(256), 0, st, in.fields,
                       (const int*)nullptr, n, d_len);
  else
    hipLaunchKernelGGL(patch_len_kernel, dim3(text_grid(n1, 4)), dim3(256), 0, st, in.fields, in.image_off, in.image_ids,
                       in.vimage_off, in.vimage_ids, n, d_len);
  TCHK(hipGetLastError());
  TCHK(hipcub::DeviceScan::ExclusiveScan(temp.p, tb, d_len, d_off, hipcub::Sum(), header_bytes, n1, st));
  // the scratch above is freed on return: the work that reads it must have finished
  return hipStreamSynchronize(st);
}

hipError_t text_write(int kind, const TextArrays& in, int n, const long long* d_off, char* d_out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (kind == PMVS_TEXT_PLY)
    hipLaunchKernelGGL(rows_write_kernel<PMVS_TEXT_PLY>, dim3(text_grid(n, kTileRows)), dim3(kTileRows), 0, st, in.fields,
                       in.colors, n, d_off, d_out);
  else if (kind == PMVS_TEXT_PSET)
    hipLaunchKernelGGL(rows_write_kernel<PMVS_TEXT_PSET>, dim3(text_grid(n, kTileRows)), dim3(kTileRows), 0, st, in.fields,
                       (const int*)nullptr, n, d_off, d_out);
  else
    hipLaunchKernelGGL(patch_write_kernel, dim3(text_grid(n, 4)), dim3(256), 0, st, in.fields, in.image_off, in.image_ids,
                       in.vimage_off, in.vimage_ids, n, d_off, d_out);
  return hipGetLastError();
}

hipError_t launch_format_selftest(int precision, const float* d_in, int n, char* d_out, int* d_len, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(format_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, st, precision, d_in, n, d_out, d_len);
  return hipGetLastError();
}

}  // namespace pmvsdev
