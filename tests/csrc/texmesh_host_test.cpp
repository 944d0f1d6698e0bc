// tests/csrc/texmesh_host_test.cpp -- pmvs_texmesh.h on the host: the raster of already projected corners, with the
// header's own functions, for tests/test_texmesh_host.py to compare with the numpy restatement.  Stand-alone, built
// with -fsanitize=address,undefined.
//   texmesh_host_test IN OUT
// IN:  int32 W, H, nv, nf; float32 nv x 3 (x, y, z of a corner); int32 nf x 3 (corner ids)
// OUT: uint64 W x H keys ((depth_bits(d) << 32) | face, all ones = empty); then per face int32 drawn, boxed and
//      int64 box pixels; then float32 nv x 2 (tex_u(x, W), tex_v(y, H))
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pmvs_texmesh.h"

static uint32_t depth_bits(float d) {  // pmvs_device.h's, on the host
  uint32_t u;
  std::memcpy(&u, &d, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t head[4];
  if (std::fread(head, 4, 4, in) != 4) return 2;
  const int W = head[0], H = head[1], nv = head[2], nf = head[3];
  std::vector<float> vertex((size_t)nv * 3);
  std::vector<int32_t> face((size_t)nf * 3);
  if (std::fread(vertex.data(), 4, vertex.size(), in) != vertex.size()) return 2;
  if (std::fread(face.data(), 4, face.size(), in) != face.size()) return 2;
  std::fclose(in);
  std::vector<uint64_t> keys((size_t)W * H, ~0ull);
  std::vector<int32_t> flags((size_t)nf * 2);
  std::vector<int64_t> boxes((size_t)nf);
  for (int f = 0; f < nf; ++f) {
    pmvstex::Corner c[3];
    for (int k = 0; k < 3; ++k) {
      const float* v = &vertex[3 * (size_t)face[3 * f + k]];
      c[k].x = v[0], c[k].y = v[1], c[k].z = v[2];
    }
    double A = 0.0;
    pmvstex::Box b{};
    const bool drawn = pmvstex::face_drawn(c, &A);
    const bool boxed = drawn && pmvstex::face_box(c, W, H, &b);
    flags[2 * f] = drawn, flags[2 * f + 1] = boxed;
    boxes[f] = boxed ? pmvstex::box_pixels(b) : 0;
    if (!boxed) continue;
    for (int v = b.v0; v <= b.v1; ++v)
      for (int u = b.u0; u <= b.u1; ++u) {
        float d;
        if (!pmvstex::face_pixel_depth(c, A, u, v, &d)) continue;
        const uint64_t key = ((uint64_t)depth_bits(d) << 32) | (uint32_t)f;
        uint64_t& cell = keys[(size_t)v * W + u];
        if (key < cell) cell = key;
      }
  }
  std::vector<float> tex((size_t)nv * 2);
  for (int i = 0; i < nv; ++i) tex[2 * i] = pmvstex::tex_u(vertex[3 * i], W), tex[2 * i + 1] = pmvstex::tex_v(vertex[3 * i + 1], H);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(keys.data(), 8, keys.size(), out);
  std::fwrite(flags.data(), 4, flags.size(), out);
  std::fwrite(boxes.data(), 8, boxes.size(), out);
  std::fwrite(tex.data(), 4, tex.size(), out);
  return std::fclose(out) == 0 ? 0 : 2;
}
