// oracle/ref_filter.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// Runs pieces of the reference's own CFilter and CExpand, compiled unmodified from
// $(REF)/source/pmvs/filter.cpp and expand.cpp (with findMatch.cpp, patchOrganizerS.cpp,
// photoSetS.cpp, camera.cpp and patch.cpp) by oracle/Makefile, so the restatements in
// oracle/filter_oracle.h and expand_oracle.h are pinned to reference object code
// (tests/test_filter_pinning.py):
//   op 1  CFilter::setDepthMapsVGridsVPGridsAddPatchV(0) at _depth == 0   filter.cpp:734-783
//         = collectPatches (patchOrganizerS.cpp:207-236), setDepthMaps (filter.cpp:667-732),
//           setVImagesVGrids (patchOrganizerS.cpp:420-450), addPatchVThread (filter.cpp:808-839)
//   op 2  a sequence of CExpand::checkCounts (expand.cpp:258-323) and updateCounts (:325-406) calls
//
// The recipe is ref_organizer.cpp's: the symbols of optim.cpp (nlopt), image.cpp (CImg) and
// mylapack.cpp (Eigen) stay unresolved (non-PIE, --unresolved-symbols=ignore-all) and are never
// called, no stand-in is written for any of them, and the objects the functions read are
// materialised in raw storage by their own reference constructors: CCamera + init per view,
// CPhotoSetS, and -- inside the raw CFindMatch, where CFilter and CExpand look for them --
// CPatchOrganizerS + init, CFilter and CExpand.  The thread members of CFindMatch (_lock, _count,
// _jobs, _imageLocks, _countLocks) are placement-constructed; _CPU is 1, because the *Thread bodies
// merge their results in lock order.  Every photo has _alloc = 2 and maxLevel empty _edges vectors,
// so CPhoto::getEdge answers 1 as it does for a scene without edge images.
//
// Patches enter the organizer through the reference's own addPatch at _depth == 0, in record order:
// the insertion order of every cell list is the row index, the convention the restatement and the
// device fix.  Results are mapped back to input rows through the patch pointers.
//
// Out of reach here: the three-argument CFindMatch::isNeighbor (findMatch.cpp:120-123)
// calls COptim::getUnit (optim.cpp), and computeGain, filterOutsideThread and filterSmallGroupsSub all
// call it on every cell entry they visit; isVisible at _depth > 0 calls getUnit too.
//
// stdin (little-endian int32 / float32):
//   num, tnum, level, csize, maxLevel, then per view: path length, path bytes (a CONTOUR camera
//   file), widths[maxLevel], heights[maxLevel];
//   n, then n x {coord[4], m, m x {image, ix, iy}}          the patch set, added in this order
//   then operations until EOF:
//   1:                                     -> per target cell: winner row (-1 empty); per target
//                                             cell: float32 OpticalAxis * winner coord (0 empty);
//                                             collected count, collected rows; per row: mv, then
//                                             mv x {image, ix, iy}; per target cell: k, k rows (_vpgrids)
//   2: depth, countThreshold1, minImageNum, k, then k x {kind (0 check, 1 update), m, m x {image, ix,
//      iy}, mv, mv x {image, ix, iy}}      -> k return values; per target cell: _counts
#include <cstdint>
#include <cstdio>
#include <list>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "pmvs/findMatch.hpp"

namespace {
struct FmProbe : public PMVS3::CFindMatch {
  using PMVS3::CFindMatch::_count;
  using PMVS3::CFindMatch::_countLocks;
  using PMVS3::CFindMatch::_imageLocks;
  using PMVS3::CFindMatch::_jobs;
  using PMVS3::CFindMatch::_lock;
  using PMVS3::CFindMatch::_num;
  using PMVS3::CFindMatch::_tnum;
};
struct ImgProbe : public Image::CImage {
  using Image::CImage::_alloc;
  using Image::CImage::_edges;
  using Image::CImage::_heights;
  using Image::CImage::_widths;
};
struct FilterProbe : public PMVS3::CFilter {
  using PMVS3::CFilter::setDepthMapsVGridsVPGridsAddPatchV;
};
struct ExpandProbe : public PMVS3::CExpand {
  using PMVS3::CExpand::checkCounts;
  using PMVS3::CExpand::updateCounts;
};

bool rd(void* p, size_t n) { return std::fread(p, 1, n, stdin) == n; }
int32_t ri() {
  int32_t v = 0;
  if (!rd(&v, 4)) throw 1;
  return v;
}
void wi(int32_t v) { std::fwrite(&v, 4, 1, stdout); }
void wf(float v) { std::fwrite(&v, 4, 1, stdout); }
void rlist(std::vector<int>& images, std::vector<TVec2<int>>& grids) {
  const int m = ri();
  for (int k = 0; k < m; ++k) {
    images.push_back(ri());
    const int ix = ri(), iy = ri();
    grids.push_back(TVec2<int>(ix, iy));
  }
}
}  // namespace

int main() {
  try {
    const int num = ri(), tnum = ri(), level = ri(), csize = ri(), maxLevel = ri();
    alignas(PMVS3::CFindMatch) static unsigned char raw[sizeof(PMVS3::CFindMatch)];
    PMVS3::CFindMatch& fm = *reinterpret_cast<PMVS3::CFindMatch*>(raw);
    fm._level = level;
    fm._csize = csize;
    fm._depth = 0;
    fm._CPU = 1;
    fm._neighborThreshold = 0.5f;  // findMatch.cpp:99 (isVisible0's strict; unread at depth 0)
    fm.*(&FmProbe::_tnum) = tnum;
    fm.*(&FmProbe::_num) = num;
    fm.*(&FmProbe::_count) = 0;
    new (&(fm.*(&FmProbe::_lock))) std::mutex();
    new (&(fm.*(&FmProbe::_jobs))) std::list<int>();
    new (&(fm.*(&FmProbe::_imageLocks))) std::vector<std::shared_mutex*>();
    new (&(fm.*(&FmProbe::_countLocks))) std::vector<std::shared_mutex*>();
    for (int i = 0; i < num; ++i) {
      (fm.*(&FmProbe::_imageLocks)).push_back(new std::shared_mutex());
      (fm.*(&FmProbe::_countLocks)).push_back(new std::shared_mutex());
    }
    new (&fm._pss) Image::CPhotoSetS();
    fm._pss._num = num;
    fm._pss._photos.reserve(num);  // storage only: a CPhoto cannot be constructed (ref_organizer.cpp)
    Image::CPhoto* photos = fm._pss._photos.data();
    for (int v = 0; v < num; ++v) {
      const int len = ri();
      std::string path((size_t)len, '\0');
      if (!rd(&path[0], (size_t)len)) return 2;
      Image::CCamera* cam = static_cast<Image::CCamera*>(&photos[v]);
      new (cam) Image::CCamera();
      cam->init(path, maxLevel);
      Image::CImage* im = static_cast<Image::CImage*>(&photos[v]);
      std::vector<int> w((size_t)maxLevel), h((size_t)maxLevel);
      for (int l = 0; l < maxLevel; ++l) w[l] = ri();
      for (int l = 0; l < maxLevel; ++l) h[l] = ri();
      new (&(im->*(&ImgProbe::_widths))) std::vector<int>(w);
      new (&(im->*(&ImgProbe::_heights))) std::vector<int>(h);
      new (&(im->*(&ImgProbe::_edges))) std::vector<std::vector<unsigned char>>((size_t)maxLevel);
      im->*(&ImgProbe::_alloc) = 2;
    }
    new (&fm._pos) PMVS3::CPatchOrganizerS(fm);
    fm._pos.init();
    new (&fm._filter) PMVS3::CFilter(fm);
    new (&fm._expand) PMVS3::CExpand(fm);

    const int n = ri();
    std::vector<Patch::PPatch> pp((size_t)n);
    std::unordered_map<const Patch::CPatch*, int32_t> row;
    for (int r = 0; r < n; ++r) {
      pp[r].reset(new Patch::CPatch());
      float c[4];
      if (!rd(c, 16)) return 2;
      pp[r]->_coord = Vec4f(c[0], c[1], c[2], c[3]);
      rlist(pp[r]->_images, pp[r]->_grids);
      row[pp[r].get()] = r;
      fm._pos.addPatch(pp[r]);
    }

    int32_t op = 0;
    while (rd(&op, 4)) {
      if (op == 1) {
        fm._depth = 0;
        (fm._filter.*(&FilterProbe::setDepthMapsVGridsVPGridsAddPatchV))(0);
        for (int t = 0; t < tnum; ++t)
          for (const Patch::PPatch& d : fm._pos._dpgrids[t])
            wi(d == PMVS3::CPatchOrganizerS::_MAXDEPTH ? -1 : row.at(d.get()));
        for (int t = 0; t < tnum; ++t)
          for (const Patch::PPatch& d : fm._pos._dpgrids[t])
            wf(d == PMVS3::CPatchOrganizerS::_MAXDEPTH ? 0.0f : photos[t].OpticalAxis() * d->_coord);
        wi((int32_t)fm._pos._ppatches.size());
        for (const Patch::PPatch& p : fm._pos._ppatches) wi(row.at(p.get()));
        for (int r = 0; r < n; ++r) {
          wi((int32_t)pp[r]->_vimages.size());
          for (size_t k = 0; k < pp[r]->_vimages.size(); ++k) {
            wi(pp[r]->_vimages[k]);
            wi(pp[r]->_vgrids[k][0]);
            wi(pp[r]->_vgrids[k][1]);
          }
        }
        for (int t = 0; t < tnum; ++t)
          for (const std::vector<Patch::PPatch>& cell : fm._pos._vpgrids[t]) {
            wi((int32_t)cell.size());
            for (const Patch::PPatch& p : cell) wi(row.at(p.get()));
          }
      } else if (op == 2) {
        fm._depth = ri();
        fm._countThreshold1 = ri();
        fm._minImageNumThreshold = ri();
        const int k = ri();
        fm._pos.clearCounts();
        for (int c = 0; c < k; ++c) {
          const int kind = ri();
          Patch::CPatch p;
          rlist(p._images, p._grids);
          rlist(p._vimages, p._vgrids);
          wi(kind == 0 ? (fm._expand.*(&ExpandProbe::checkCounts))(p) : (fm._expand.*(&ExpandProbe::updateCounts))(p));
        }
        for (int t = 0; t < tnum; ++t)
          for (unsigned char c : fm._pos._counts[t]) wi((int32_t)c);
      } else {
        return 2;
      }
    }
    std::fflush(stdout);
    std::_Exit(0);  // the raw-storage objects are never destroyed (their CImage / CFindMatch
                    // destructors live in the unbuilt TUs)
  } catch (int) {
    return 2;
  }
}
