// tests/csrc/atlas_host_test.cpp -- csrc/pmvs_atlas.h on the host (tests/test_atlas_host.py builds it with
// -fsanitize=address,undefined): for one class of `count` faces of side n in an atlas W texels wide, every
// texel of the class's band through texel_of, and every face's corners through face_corner.
//   atlas_host_test W n count y0 out.bin
// out.bin: per texel (row-major, rows * (n + 5) rows of W) the record {int32 ok, rank, half, pad; double l1, l2},
// then per rank and corner {int64 x, y}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pmvs_atlas.h"

struct Rec {
  int32_t ok, rank, half, pad;
  double l1, l2;
};

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int W = std::atoi(argv[1]), n = std::atoi(argv[2]), count = std::atoi(argv[3]), y0 = std::atoi(argv[4]);
  const int c = n + pmvsatlas::kGutter;
  const long long rows = pmvsatlas::class_rows(count, W, n) * c;
  std::vector<Rec> recs;
  for (int J = 0; J < rows; ++J)
    for (int I = 0; I < W; ++I) {
      pmvsatlas::Texel t{-1, -1, 0.0, 0.0};
      const bool ok = pmvsatlas::texel_of(W, n, count, I, J, &t);
      recs.push_back(ok ? Rec{1, t.rank, t.half, 0, t.l1, t.l2} : Rec{0, -1, -1, 0, 0.0, 0.0});
    }
  std::vector<int64_t> corners;
  for (int r = 0; r < count; ++r)
    for (int k = 0; k < 3; ++k) {
      long long x, y;
      pmvsatlas::face_corner(W, n, y0, r, k, &x, &y);
      corners.push_back(x), corners.push_back(y);
    }
  // the band table's search: every row of three bands finds its band
  const pmvsatlas::Band bands[3] = {{0, 9, 1, 0}, {14, 4, 1, 1}, {23, 1, 1, 2}};
  for (int J = 0; J < 29; ++J)
    if (pmvsatlas::band_of_row(bands, 3, J) != (J < 14 ? 0 : (J < 23 ? 1 : 2))) return 3;
  if (pmvsatlas::band_of_row(bands, 1, 5) != 0) return 3;
  FILE* f = std::fopen(argv[5], "wb");
  if (!f) return 4;
  std::fwrite(recs.data(), sizeof(Rec), recs.size(), f);
  std::fwrite(corners.data(), sizeof(int64_t), corners.size(), f);
  return std::fclose(f) == 0 ? 0 : 4;
}
