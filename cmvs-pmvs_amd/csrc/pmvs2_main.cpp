// pmvs2_main.cpp -- the `pmvs2 prefix option_file [PATCH] [PSET] [DEPTH] [PIXDEPTH] [FUSE] [MESH] [FINEMESH] [TEXMESH]` executable (reference
// source/pmvs.cpp:7-63 with CFindMatch::init / run / write, findMatch.cpp:30-224), driving the
// MI355X-native core through its C-ABI (include/pmvs_amd.h).  A drop-in for the program
// genOption's pmvs.sh calls (genOption.cpp:73): same arguments, same input tree
// (prefix/visualize, prefix/txt, prefix/masks, prefix/edges, vis.dat, bimages.dat), same outputs
// (prefix/models/<option>.ply always, .patch / .pset on request).
//
// Pipeline: option file -> images (PPM / JPEG), masks, edges, cameras -> pmvs_scene_create (device
// pyramids) -> pmvs_detect_features (Harris + DoG on the device) -> pmvs_seed_run (seed phase) ->
// pmvs_run_loop (3 x expand / filter, model resident in HBM) -> pmvs_loop_export (writer order, fields,
// lists and colours on the device) -> writers.
//
// Multi-rank jobs (CMVS cluster per GPU): with WORLD_SIZE > 1 in the environment
// (torchrun-style: RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT; genOption --gpus N writes
// the script that sets them) the WORLD_SIZE pmvs2 processes of one job -- one cluster option file
// each -- find each other over TCP (pmvs_tcp), and their loops exchange the clusters' boundary
// patches after every iteration (pmvs_scene_set_cluster): device to device over RCCL on GPU LOCAL_RANK
// (the unique id travels on the TCP channel), or over the TCP channel itself with
// PMVS_EXCHANGE=tcp (several ranks on one GPU).  Each rank writes its own cluster's outputs.
//
// Expansion schedule: option `CPU 1` selects the reference's single-thread schedule exactly
// (wave = 1); any other value the production wave schedule (the reference's own
// multi-threaded schedule is nondeterministic).  PMVS_WAVE / PMVS_MIN_CANDIDATES override it.
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/pmvs_amd.h"

namespace {

bool exists(const std::string& p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0;
}

[[noreturn]] void die(const char* what, pmvs_status st) {
  std::cerr << "pmvs2: " << what << ": " << pmvs_last_error() << " (status " << (int)st << ")" << std::endl;
  std::exit(1);
}

#define CHECK(what, expr)                     \
  do {                                        \
    pmvs_status st_ = (expr);                 \
    if (st_ != PMVS_OK) die(what, st_);       \
  } while (0)

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}

const char* env_str(const char* name, const char* dflt) {
  const char* e = std::getenv(name);
  return (e && *e) ? e : dflt;
}

// The job's channels (WORLD_SIZE > 1): TCP between the processes, and RCCL unless PMVS_EXCHANGE=tcp.
struct Job {
  int rank = 0, world = 1, device = 0;
  bool rccl = true;
  pmvs_tcp* tcp = nullptr;
  pmvs_rccl* comm = nullptr;
  ~Job() {
    pmvs_rccl_destroy(comm);
    pmvs_tcp_destroy(tcp);
  }
  // every rank's `ok` flag; false when some rank failed (or has exited: its connection is closed)
  bool all_ok(bool ok) {
    if (world == 1) return ok;
    int32_t mine = ok ? 1 : 0;
    std::vector<int32_t> all(world, 0);
    if (pmvs_tcp_allgather(tcp, &mine, sizeof(mine), all.data()) != 0) return false;
    for (int32_t a : all)
      if (!a) return false;
    return true;
  }
};

// CImage::completeName (image.cpp:40-84): the first existing extension, else the bare name.
std::string complete_name(const std::string& base, bool color) {
  const char* ext_c[] = {".ppm", ".jpg"};
  const char* ext_m[] = {".pgm", ".pbm"};
  for (const char* e : (color ? ext_c : ext_m))
    if (exists(base + e)) return base + e;
  return base;
}

struct View {
  std::vector<uint8_t> rgb, mask, edge;
  int w = 0, h = 0;
  float proj[12];
};

void usage(const char* argv0) {
  std::cerr << "Usage: " << argv0 << " prefix option_file [Optional export]" << std::endl
            << std::endl
            << "--------------------------------------------------" << std::endl
            << "level       1    csize    2" << std::endl
            << "threshold   0.7  wsize    7" << std::endl
            << "minImageNum 3    CPU      4" << std::endl
            << "useVisData  0    sequence -1" << std::endl
            << "quad        2.5  maxAngle 10.0" << std::endl
            << "--------------------------------------------------" << std::endl
            << "2 ways to specify targetting images" << std::endl
            << "timages  5  1 3 5 7 9 (enumeration)" << std::endl
            << "        -1  0 24 (range specification)" << std::endl
            << "--------------------------------------------------" << std::endl
            << "4 ways to specify other images" << std::endl
            << "oimages  5  0 2 4 6 8 (enumeration)" << std::endl
            << "        -1  24 48 (range specification)" << std::endl
            << std::endl
            << "[Optional export] PATCH PSET DEPTH PIXDEPTH FUSE MESH FINEMESH TEXMESH ATLAS" << std::endl
            << " i.e export patch and pset: prefix option_file PATCH PSET"
            << " i.e export patch only: prefix option_file PATCH" << std::endl
            << " DEPTH: every target image's depth map, one value per csize x csize cell, as" << std::endl
            << "        models/option_file.depth.<8-digit image number>.pfm (0 = no patch)" << std::endl
            << " PIXDEPTH: every target image's depth map, one value per pixel at the option's level, every" << std::endl
            << "        patch rendered as a plane element of radius csize (at most " << PMVS_PIXEL_MAX_RADIUS
            << ") pixels, as" << std::endl
            << "        models/option_file.pixdepth.<8-digit image number>.pfm (0 = no patch)" << std::endl
            << " FUSE: the per-pixel maps of all target images (radius csize) fused into one point cloud: a pixel" << std::endl
            << "        whose surface point at least 2 other target images see at a depth within 1 % and with a" << std::endl
            << "        normal within 60 degrees gives one oriented, coloured point, once per surface point, as the" << std::endl
            << "        binary PLY models/option_file.fused.ply (x y z nx ny nz, colour, support)" << std::endl
            << " MESH: FUSE's maps integrated into a truncated signed distance volume (the fused cloud's bounding" << std::endl
            << "        box padded by 3 voxels, voxel = its longest extent / 256, truncation 3 voxels) and meshed by" << std::endl
            << "        naive surface nets, as the binary PLY models/option_file.mesh.ply (x y z nx ny nz, colour; faces)" << std::endl
            << " FINEMESH: the same mesh at image resolution, in a sparse volume of 8x8x8-voxel bricks that exists only" << std::endl
            << "        within 5 voxels of the fused points: voxel = the cloud's longest extent / min(4096, the largest" << std::endl
            << "        width or height of the target images at the level), truncation 3 voxels, as the binary PLY" << std::endl
            << "        models/option_file.finemesh.ply" << std::endl
            << " TEXMESH: MESH's mesh textured from the target images themselves (no atlas): every face gets the target" << std::endl
            << "        that sees it from the front with the largest projected area and whose view of its three corners" << std::endl
            << "        the mesh itself does not block (within 1 % of the depth), as the binary PLY" << std::endl
            << "        models/option_file.texmesh.ply with one `comment TextureFile ../visualize/<image>` per target" << std::endl
            << "        image, per-face texcoord (u, v in [0, 1], v up) and texnumber (-1 = no image sees the face)" << std::endl
            << " ATLAS: TEXMESH's mesh and views baked into one texture: every face's texels cut out of its image and" << std::endl
            << "        packed as right triangles of side 1 .. 64 texels (one texel per level-0 pixel of the face's" << std::endl
            << "        longest edge) into an atlas 8192 texels wide, as the binary PPM models/option_file.atlas.ppm and" << std::endl
            << "        the binary PLY models/option_file.atlas.ply with the single `comment TextureFile" << std::endl
            << "        option_file.atlas.ppm` (texnumber 0, or -1 for a face without texels)" << std::endl;
}

}  // namespace

int main(int argc, char* argv[]) {
  if (argc < 3) {
    usage(argv[0]);
    return 1;
  }
  for (int i = 0; i < argc; ++i) std::cout << std::endl << argv[i];
  std::cout << std::endl;
  const std::string prefix = argv[1], option = argv[2];
  bool export_patch = false, export_pset = false, export_depth = false, export_pixdepth = false, export_fuse = false, export_mesh = false,
       export_finemesh = false, export_texmesh = false, export_atlas = false;
  for (int i = 3; i < argc; ++i) {
    if (std::string(argv[i]) == "PATCH") export_patch = true;
    if (std::string(argv[i]) == "PSET") export_pset = true;
    if (std::string(argv[i]) == "DEPTH") export_depth = true;
    if (std::string(argv[i]) == "PIXDEPTH") export_pixdepth = true;
    if (std::string(argv[i]) == "FUSE") export_fuse = true;
    if (std::string(argv[i]) == "MESH") export_mesh = true;
    if (std::string(argv[i]) == "FINEMESH") export_finemesh = true;
    if (std::string(argv[i]) == "TEXMESH") export_texmesh = true;
    if (std::string(argv[i]) == "ATLAS") export_atlas = true;
  }
  const double t0 = now_s();

  // ---- the job (WORLD_SIZE > 1: one rank per cluster option file)
  Job job;
  job.world = env_int("WORLD_SIZE", 1);
  job.rank = env_int("RANK", 0);
  job.device = env_int("PMVS_DEVICE", env_int("LOCAL_RANK", 0));
  job.rccl = std::string(env_str("PMVS_EXCHANGE", "rccl")) != "tcp";
  if (job.world < 1 || job.rank < 0 || job.rank >= job.world) {
    std::cerr << "pmvs2: RANK " << job.rank << " / WORLD_SIZE " << job.world << " out of range" << std::endl;
    return 1;
  }
  if (job.world > 1) {
    CHECK("job", pmvs_tcp_create(job.rank, job.world, env_str("MASTER_ADDR", "127.0.0.1"), env_int("MASTER_PORT", 29533),
                                 env_int("PMVS_JOIN_TIMEOUT_MS", 600000), &job.tcp));
    std::cerr << "pmvs2: rank " << job.rank << " of " << job.world << ", GPU " << job.device << ", exchange "
              << (job.rccl ? "rccl" : "tcp") << std::endl;
  }

  // ---- SOption::init (option.cpp:30-160)
  pmvs_options* opt = nullptr;
  CHECK("option file", pmvs_options_load(prefix.c_str(), option.c_str(), &opt));
  std::vector<int> images(opt->timages, opt->timages + opt->num_timages);
  images.insert(images.end(), opt->oimages, opt->oimages + opt->num_oimages);
  const int num = (int)images.size(), tnum = opt->num_timages;
  if (tnum == 0) {
    std::cerr << "pmvs2: no target images" << std::endl;
    return 1;
  }

  // ---- CPhotoSetS::init (photoSetS.cpp:12-80): 8-digit names, else 4-digit.  The reference decodes
  // the views one after the other; here a pool of host threads decodes them (PMVS_IO_THREADS, default
  // min(16, cores)), and failures are reported in view order as the serial loop would.
  std::vector<View> views(num);
  std::vector<std::string> tex_names(num);  // the image files as models/ sees them (TEXMESH)
  std::vector<std::string> errors(num);
  std::vector<pmvs_status> status(num, PMVS_OK);
  std::cerr << "Reading images: " << std::flush;
  {
    std::atomic<int> next{0};
    auto load_one = [&](int index) -> pmvs_status {
      const int image = images[index];
      char b8[64], b4[64];
      std::snprintf(b8, sizeof(b8), "%08d", image);
      std::snprintf(b4, sizeof(b4), "%04d", image);
      const std::string v8 = prefix + "visualize/" + b8;
      const std::string id = (exists(v8 + ".ppm") || exists(v8 + ".jpg")) ? b8 : b4;
      View& v = views[index];
      const std::string name = complete_name(prefix + "visualize/" + id, true);
      tex_names[index] = "../visualize/" + name.substr(prefix.size() + std::strlen("visualize/"));
      pmvs_status st;
      errors[index] = "image";
      if ((st = pmvs_image_load(name.c_str(), &v.w, &v.h, nullptr))) return st;
      v.rgb.resize((size_t)v.w * v.h * 3);
      if ((st = pmvs_image_load(name.c_str(), &v.w, &v.h, v.rgb.data()))) return st;
      errors[index] = "camera";
      if ((st = pmvs_camera_load((prefix + "txt/" + id + ".txt").c_str(), v.proj))) return st;
      for (int k = 0; k < 2; ++k) {
        const std::string m = complete_name(prefix + (k == 0 ? "masks/" : "edges/") + id, false);
        if (m.size() < 4 || (m.compare(m.size() - 4, 4, ".pgm") && m.compare(m.size() - 4, 4, ".pbm"))) continue;
        int mw = 0, mh = 0;
        std::vector<uint8_t>& dst = k == 0 ? v.mask : v.edge;
        errors[index] = "mask/edge";
        if ((st = pmvs_pnm_mask_load(m.c_str(), &mw, &mh, nullptr))) return st;
        if (mw != v.w || mh != v.h) {
          errors[index] = m + " is " + std::to_string(mw) + "x" + std::to_string(mh) + ", image " + std::to_string(v.w) +
                          "x" + std::to_string(v.h);
          return PMVS_EINVAL;
        }
        dst.resize((size_t)mw * mh);
        if ((st = pmvs_pnm_mask_load(m.c_str(), &mw, &mh, dst.data()))) return st;
      }
      // CFindMatch::init: _pss.setEdge(_setEdge) replaces the edge maps (findMatch.cpp:74-76)
      if (opt->set_edge != 0.0f) {
        v.edge.resize((size_t)v.w * v.h);
        errors[index] = "setEdge";
        if ((st = pmvs_set_edge(v.rgb.data(), v.w, v.h, opt->set_edge, v.edge.data()))) return st;
      }
      return PMVS_OK;
    };
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    const int nthreads = std::max(1, std::min({num, env_int("PMVS_IO_THREADS", std::min(16, hw))}));
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t)
      pool.emplace_back([&]() {
        for (int index; (index = next.fetch_add(1)) < num;) {
          status[index] = load_one(index);
          if (status[index] != PMVS_OK && errors[index].find(' ') == std::string::npos)
            errors[index] += std::string(": ") + pmvs_last_error();  // the worker's own last error
        }
      });
    for (auto& t : pool) t.join();
  }
  for (int index = 0; index < num; ++index) {
    if (status[index] != PMVS_OK) {
      std::cerr << std::endl << "pmvs2: " << errors[index] << " (status " << (int)status[index] << ")" << std::endl;
      return 1;
    }
    std::cerr << '*';
  }
  std::cerr << std::endl;
  const double t_read = now_s();

  // ---- the device scene (CFindMatch::init, findMatch.cpp:30-107)
  std::vector<pmvs_view_desc> vd(num);
  for (int i = 0; i < num; ++i) {
    vd[i].width = views[i].w;
    vd[i].height = views[i].h;
    vd[i].rgb = views[i].rgb.data();
    vd[i].mask = views[i].mask.empty() ? nullptr : views[i].mask.data();
    vd[i].edge = views[i].edge.empty() ? nullptr : views[i].edge.data();
    std::memcpy(vd[i].projection, views[i].proj, sizeof(views[i].proj));
  }
  pmvs_scene_desc d{};
  d.num_views = num;
  d.num_targets = tnum;
  d.level = opt->level;
  d.csize = opt->csize;
  d.wsize = opt->wsize;
  d.min_image_num = opt->min_image_num;
  d.threshold = opt->threshold;
  d.max_angle = opt->max_angle;
  d.quad_threshold = opt->quad;
  d.sequence = opt->sequence;
  d.visdata2_offsets = opt->visdata2_offsets;
  d.visdata2 = opt->visdata2;
  d.num_bindexes = opt->num_bindexes;
  d.bindexes = opt->bindexes;
  d.views = vd.data();
  pmvs_scene* sc = nullptr;
  CHECK("scene", pmvs_scene_create(&d, job.device, &sc));
  // every rank has its scene before any collective (a rank that failed has exited, which its
  // peers see here instead of blocking in the RCCL bootstrap)
  if (!job.all_ok(true)) {
    std::cerr << "pmvs2: another rank of the job failed before the cluster exchange was set up" << std::endl;
    return 1;
  }
  if (job.world > 1) {
    if (job.rccl) {
      uint8_t id[128] = {0};
      if (job.rank == 0) CHECK("rccl", pmvs_rccl_unique_id(id));
      std::vector<uint8_t> ids((size_t)128 * job.world);
      if (pmvs_tcp_allgather(job.tcp, id, 128, ids.data()) != 0) {
        std::cerr << "pmvs2: the RCCL id exchange failed" << std::endl;
        return 1;
      }
      CHECK("rccl", pmvs_rccl_create(job.device, job.rank, job.world, ids.data(), &job.comm));
      CHECK("cluster", pmvs_scene_set_cluster_rccl(sc, job.rank, job.world, images.data(), job.comm));
    } else {
      CHECK("cluster", pmvs_scene_set_cluster(sc, job.rank, job.world, images.data(), &pmvs_tcp_allgather, job.tcp));
    }
  }
  std::vector<int32_t> tex_dims((size_t)tnum * 2);  // the level-0 sizes of the target images (TEXMESH)
  for (int t = 0; t < tnum; ++t) tex_dims[2 * t] = views[t].w, tex_dims[2 * t + 1] = views[t].h;
  std::vector<View>().swap(views);  // level-0 images live on the device now
  const double t_init = now_s();

  // ---- CDetectFeatures::run (detectFeatures.cpp:14-124, fcsize 16): skipped for an image whose
  // prefix/models/%08d.affin<level> exists, as the reference does
  std::vector<pmvs_point> points;
  std::vector<int32_t> npts(num, 0);
  for (int index = 0; index < num; ++index) {
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%08d.affin%d", images[index], opt->level);
    if (exists(prefix + "models/" + buf)) continue;
    int32_t n = 0;
    CHECK("features", pmvs_detect_features(sc, index, 16, nullptr, 0, &n));
    const size_t at = points.size();
    points.resize(at + n);
    CHECK("features", pmvs_detect_features(sc, index, 16, points.data() + at, n, &n));
    npts[index] = n;
  }
  const double t_feat = now_s();

  // ---- seed phase (CSeed::run, findMatch.cpp:193)
  int32_t nseeds = 0;
  pmvs_seed_stats sst{};
  CHECK("seeds", pmvs_seed_run(sc, points.data(), npts.data(), env_int("PMVS_SEED_BATCH", 0), nullptr, 0, &nseeds,
                               &sst));
  std::vector<pmvs_patch> seeds(std::max(nseeds, 1));
  CHECK("seeds", pmvs_seed_fetch(sc, seeds.data(), nseeds));
  seeds.resize(nseeds);
  std::cerr << "Total pass fail0 fail1 refinepatch: " << sst.trial << ' ' << sst.pass << ' ' << sst.fail0 << ' '
            << sst.fail1 << ' ' << sst.pass + sst.fail1 << std::endl;
  const double t_seed = now_s();

  // every rank reaches the loop (a rank whose features or seeds failed has exited, which its peers
  // see on the TCP channel here rather than inside an RCCL collective); failures inside the loop
  // reach every rank through the loop's error headers
  if (!job.all_ok(true)) {
    std::cerr << "pmvs2: another rank of the job failed before the loop" << std::endl;
    return 1;
  }

  // ---- expansion / filtering (findMatch.cpp:196-217)
  const int wave = env_int("PMVS_WAVE", opt->cpu == 1 ? 1 : 32768);
  const int min_cands = env_int("PMVS_MIN_CANDIDATES", wave == 1 ? 0 : 131072);
  const int iterations = 3;
  std::vector<pmvs_loop_iter> it(iterations);
  int32_t nmodel = 0;
  CHECK("expand/filter", pmvs_run_loop(sc, seeds.data(), nseeds, opt->threshold, iterations, wave, min_cands,
                                       PMVS_EXPAND_AFTER_SEEDS, INT_MAX / 2, &nmodel, it.data()));
  for (int t = 0; t < iterations; ++t)
    std::cerr << "depth " << it[t].depth << ": expanded " << it[t].expand.added << ", kept " << it[t].patches
              << (job.world > 1 ? ", boundary sent " + std::to_string(it[t].boundary_sent) + " received " +
                                      std::to_string(it[t].boundary_received) + " inserted " +
                                      std::to_string(it[t].boundary_inserted)
                                : std::string())
              << std::endl;
  const double t_loop = now_s();

  // ---- CPatchOrganizerS::writePatches2 (patchOrganizerS.cpp:89-132): collectPatches(1)
  // (patchOrganizerS.cpp:207-236) walks target images, their cells in raster order and each cell's
  // list in insertion (= model) order, taking every patch at its first registration: the key is
  // (lowest target image holding the patch, its cell there), ties in model order.  The order, the
  // writers' fields and lists (index2image applied) and writePLY's colours are produced on the
  // device (pmvs_loop_export): only these arrays cross PCIe, not the model's records.
  // The files' text is formatted on the device too (pmvs_loop_text): per file a size query, one buffer
  // and one write.  PMVS_HOST_WRITERS=1 keeps the export arrays and the host writers (the same bytes).
  const std::string out = prefix + "models/" + option;
  if (env_int("PMVS_HOST_WRITERS", 0) == 0) {
    const struct { int32_t kind; bool wanted; const char* ext; } files[] = {
        {PMVS_TEXT_PLY, true, ".ply"}, {PMVS_TEXT_PATCH, export_patch, ".patch"}, {PMVS_TEXT_PSET, export_pset, ".pset"}};
    std::vector<char> text;
    for (const auto& f : files) {
      if (!f.wanted) continue;
      int64_t size = 0;
      CHECK(f.ext, pmvs_loop_text(sc, f.kind, PMVS_EXPORT_WRITER_ORDER, images.data(), nullptr, 0, &size));
      if ((int64_t)text.size() < size) text.resize((size_t)size);
      CHECK(f.ext, pmvs_loop_text(sc, f.kind, PMVS_EXPORT_WRITER_ORDER, images.data(), text.data(), size, &size));
      std::ofstream os(out + f.ext, std::ios::binary);
      os.write(text.data(), (std::streamsize)size);
      os.close();
      if (!os) {
        std::cerr << "pmvs2: cannot write " << out << f.ext << std::endl;
        return 1;
      }
    }
  } else {
    pmvs_export_sizes xs{};
    CHECK("export", pmvs_loop_export_sizes(sc, &xs));
    std::vector<float> fields((size_t)std::max(nmodel, 1) * 11);
    std::vector<int32_t> colors((size_t)std::max(nmodel, 1) * 3);
    std::vector<int64_t> ioff, voff;  // the lists only for the .patch file
    std::vector<int32_t> ids, vids;
    pmvs_export_buffers xb{};
    xb.fields = fields.data();
    xb.colors = colors.data();
    if (export_patch) {
      ioff.resize((size_t)nmodel + 1);
      voff.resize((size_t)nmodel + 1);
      ids.resize((size_t)std::max<int64_t>(xs.image_entries, 1));
      vids.resize((size_t)std::max<int64_t>(xs.vimage_entries, 1));
      xb.image_off = ioff.data();
      xb.image_ids = ids.data();
      xb.vimage_off = voff.data();
      xb.vimage_ids = vids.data();
    }
    CHECK("export", pmvs_loop_export(sc, PMVS_EXPORT_WRITER_ORDER, images.data(), &xb));
    std::vector<int32_t> nimg(nmodel), nvimg(nmodel);
    for (int r = 0; r < nmodel && export_patch; ++r) {
      nimg[r] = (int32_t)(ioff[r + 1] - ioff[r]);
      nvimg[r] = (int32_t)(voff[r + 1] - voff[r]);
    }
    CHECK("ply", pmvs_write_ply((out + ".ply").c_str(), nmodel, fields.data(), colors.data()));
    if (export_patch)
      CHECK("patch", pmvs_write_patches((out + ".patch").c_str(), nmodel, fields.data(), nimg.data(), ids.data(),
                                        nvimg.data(), vids.data()));
    if (export_pset) CHECK("pset", pmvs_write_pset((out + ".pset").c_str(), nmodel, fields.data()));
  }
  if (export_depth) {
    // what each target image sees of the model just written (CFilter::setDepthMaps over it, on the
    // device): the depth of the nearest patch per cell, one PFM per target image
    std::vector<int32_t> dims((size_t)tnum * 2);
    std::vector<int64_t> doff((size_t)tnum + 1);
    CHECK("depth maps", pmvs_depth_map_layout(sc, dims.data(), doff.data()));
    std::vector<float> depth((size_t)std::max<int64_t>(doff[tnum], 1));
    pmvs_depthmap_buffers db{};
    db.depth = depth.data();
    CHECK("depth maps", pmvs_loop_depth_maps(sc, PMVS_EXPORT_WRITER_ORDER, &db));
    for (int t = 0; t < tnum; ++t) {
      char name[32];
      std::snprintf(name, sizeof(name), ".depth.%08d.pfm", images[t]);
      CHECK("pfm", pmvs_write_pfm((out + name).c_str(), dims[2 * t], dims[2 * t + 1], depth.data() + doff[t]));
    }
  }
  if (export_pixdepth) {
    // the model just written rendered into every target image (pmvs_loop_pixel_maps, writer order): one
    // call and one PFM per target, so the host holds one image at a time
    const int radius = std::min<int>(opt->csize, PMVS_PIXEL_MAX_RADIUS);
    for (int t = 0; t < tnum; ++t) {
      int32_t dims[2];
      int64_t poff[2];
      CHECK("pixel maps", pmvs_pixel_map_layout(sc, t, 1, dims, poff));
      std::vector<float> depth((size_t)std::max<int64_t>(poff[1], 1));
      pmvs_depthmap_buffers db{};
      db.depth = depth.data();
      CHECK("pixel maps", pmvs_loop_pixel_maps(sc, PMVS_EXPORT_WRITER_ORDER, t, 1, radius, &db));
      char name[32];
      std::snprintf(name, sizeof(name), ".pixdepth.%08d.pfm", images[t]);
      CHECK("pfm", pmvs_write_pfm((out + name).c_str(), dims[0], dims[1], depth.data()));
    }
  }
  if (export_fuse || export_mesh || export_finemesh || export_texmesh || export_atlas) {
    // the model just written fused over all target images (pmvs_loop_fuse, writer order): a counting
    // call sizes the host arrays
    pmvs_fuse_params fp{};
    fp.radius = std::min<int>(opt->csize, PMVS_PIXEL_MAX_RADIUS);
    fp.min_support = 2;
    fp.depth_rel = 0.01f;
    fp.normal_cos = 0.5f;
    pmvs_fuse_buffers fb{};
    int64_t npts = 0;
    CHECK("fuse", pmvs_loop_fuse(sc, PMVS_EXPORT_WRITER_ORDER, 0, tnum, &fp, 0, &fb, &npts));
    const size_t cap = (size_t)std::max<int64_t>(npts, 1);
    std::vector<float> coord(cap * 3), normal(cap * 3);
    std::vector<uint8_t> color(cap * 3), support(cap);
    fb.coord = coord.data();
    fb.normal = normal.data();
    fb.color = color.data();
    fb.support = support.data();
    int64_t written = 0;
    CHECK("fuse", pmvs_loop_fuse(sc, PMVS_EXPORT_WRITER_ORDER, 0, tnum, &fp, npts, &fb, &written));
    npts = std::min(npts, written);
    if (export_fuse)
      CHECK("fused ply", pmvs_write_ply_binary((out + ".fused.ply").c_str(), npts, coord.data(), normal.data(), color.data(),
                                               support.data()));
    if (export_mesh) {
      // the same maps meshed in the cloud's padded bounding box (pmvs_loop_mesh); a cloud with no extent
      // gives an empty mesh
      int64_t nv = 0, nf = 0;
      std::vector<float> vertex, vnormal;
      std::vector<uint8_t> vcolor;
      std::vector<int32_t> face;
      pmvs_volume vol{};
      if (npts > 0 && pmvs_volume_from_points(npts, coord.data(), 256, 3, &vol) == PMVS_OK) {
        pmvs_tsdf_params tp{};
        tp.fuse = fp;
        tp.trunc = 3.0f * vol.voxel;
        pmvs_mesh_buffers mb{};
        CHECK("mesh", pmvs_loop_mesh(sc, PMVS_EXPORT_WRITER_ORDER, 0, tnum, &tp, &vol, 1, 0, 0, &mb, &nv, &nf));
        vertex.resize((size_t)nv * 3), vnormal.resize((size_t)nv * 3), vcolor.resize((size_t)nv * 3), face.resize((size_t)nf * 3);
        mb.vertex = vertex.data(), mb.normal = vnormal.data(), mb.color = vcolor.data(), mb.face = face.data();
        int64_t wv = 0, wf = 0;
        CHECK("mesh", pmvs_loop_mesh(sc, PMVS_EXPORT_WRITER_ORDER, 0, tnum, &tp, &vol, 1, nv, nf, &mb, &wv, &wf));
        nv = std::min(nv, wv), nf = std::min(nf, wf);
      }
      CHECK("mesh ply", pmvs_write_ply_mesh_binary((out + ".mesh.ply").c_str(), nv, vertex.data(), vnormal.data(),
                                                   vcolor.data(), nf, face.data()));
    }
    if (export_finemesh) {
      // the same maps meshed in a sparse brick volume (pmvs_loop_brick_mesh) whose voxel follows the target
      // images' resolution; a cloud with no extent gives an empty mesh
      int64_t nv = 0, nf = 0;
      std::vector<float> vertex, vnormal;
      std::vector<uint8_t> vcolor;
      std::vector<int32_t> face;
      std::vector<int32_t> dims((size_t)tnum * 2);
      CHECK("pixel maps", pmvs_pixel_map_layout(sc, 0, tnum, dims.data(), nullptr));
      const int32_t cells = std::min<int32_t>(4096, *std::max_element(dims.begin(), dims.end()));
      pmvs_volume vol{};
      if (npts > 0 && pmvs_brick_volume_from_points(npts, coord.data(), cells, 3, &vol) == PMVS_OK) {
        pmvs_brick_params bp{};
        bp.tsdf.fuse = fp;
        bp.tsdf.trunc = 3.0f * vol.voxel;
        bp.margin = 5;  // ceil(trunc / voxel) + 2
        pmvs_mesh_buffers mb{};
        CHECK("fine mesh", pmvs_loop_brick_mesh(sc, PMVS_EXPORT_WRITER_ORDER, 0, tnum, &bp, &vol, 1, 0, 0, &mb, &nv, &nf));
        vertex.resize((size_t)nv * 3), vnormal.resize((size_t)nv * 3), vcolor.resize((size_t)nv * 3), face.resize((size_t)nf * 3);
        mb.vertex = vertex.data(), mb.normal = vnormal.data(), mb.color = vcolor.data(), mb.face = face.data();
        int64_t wv = 0, wf = 0;
        CHECK("fine mesh", pmvs_loop_brick_mesh(sc, PMVS_EXPORT_WRITER_ORDER, 0, tnum, &bp, &vol, 1, nv, nf, &mb, &wv, &wf));
        nv = std::min(nv, wv), nf = std::min(nf, wf);
      }
      CHECK("fine mesh ply", pmvs_write_ply_mesh_binary((out + ".finemesh.ply").c_str(), nv, vertex.data(), vnormal.data(),
                                                        vcolor.data(), nf, face.data()));
    }
    if (export_texmesh || export_atlas) {
      // MESH's mesh (the same volume and parameters) obtained in device mode and kept there, a target chosen
      // per face over all target images (pmvs_mesh_texture), then one fetch and one write.  ATLAS bakes the
      // same device arrays into one image (pmvs_mesh_atlas: a sizing call, then the render) before they are freed.
      int64_t nv = 0, nf = 0;
      std::vector<float> vertex, vnormal, uv;
      std::vector<uint8_t> vcolor;
      std::vector<int32_t> face, view;
      std::vector<float> atlas_uv;  // ATLAS: the atlas, its corners and which faces have texels
      std::vector<int32_t> atlas_view;
      std::vector<uint8_t> atlas_rgb;
      pmvs_atlas_params ap{};
      ap.width = 8192, ap.max_side = 64, ap.scale = 1.0f;
      pmvs_atlas_layout al{};
      al.width = ap.width;
      pmvs_volume vol{};
      if (npts > 0 && pmvs_volume_from_points(npts, coord.data(), 256, 3, &vol) == PMVS_OK) {
        const int32_t flags = PMVS_EXPORT_WRITER_ORDER | PMVS_EXPORT_DEVICE;
        pmvs_tsdf_params tp{};
        tp.fuse = fp;
        tp.trunc = 3.0f * vol.voxel;
        pmvs_mesh_buffers mb{};
        CHECK("textured mesh", pmvs_loop_mesh(sc, flags, 0, tnum, &tp, &vol, 1, 0, 0, &mb, &nv, &nf));
        const size_t vb = (size_t)std::max<int64_t>(nv, 1) * 3, fb3 = (size_t)std::max<int64_t>(nf, 1) * 3;
        // one device block: vertex, normal, uv (float), face, view (int32), colour (bytes)
        const size_t off_normal = vb * 4, off_uv = off_normal + vb * 4, off_face = off_uv + fb3 * 2 * 4, off_view = off_face + fb3 * 4,
                     off_color = off_view + fb3 / 3 * 4, bytes = off_color + vb;
        char* block = nullptr;
        if (hipSetDevice(job.device) != hipSuccess || hipMalloc((void**)&block, bytes) != hipSuccess) {
          std::cerr << "pmvs2: textured mesh: " << bytes << " bytes of device memory" << std::endl;
          return 1;
        }
        mb.vertex = (float*)block, mb.normal = (float*)(block + off_normal), mb.color = (uint8_t*)(block + off_color);
        mb.face = (int32_t*)(block + off_face);
        int64_t wv = 0, wf = 0;
        CHECK("textured mesh", pmvs_loop_mesh(sc, flags, 0, tnum, &tp, &vol, 1, nv, nf, &mb, &wv, &wf));
        nv = std::min(nv, wv), nf = std::min(nf, wf);
        pmvs_texture_params xp{};
        xp.depth_rel = fp.depth_rel;  // the fusion's 1 %
        xp.min_area = 0.0f;
        pmvs_texture_buffers tb{};
        tb.view = (int32_t*)(block + off_view), tb.uv = (float*)(block + off_uv);
        CHECK("texture", pmvs_mesh_texture(sc, PMVS_EXPORT_DEVICE, 0, tnum, &xp, nv, mb.vertex, nf, mb.face, &tb));
        std::vector<char> host(bytes);
        if (hipMemcpy(host.data(), block, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
          std::cerr << "pmvs2: textured mesh: the fetch failed" << std::endl;
          return 1;
        }
        if (export_atlas) {
          CHECK("atlas", pmvs_mesh_atlas(sc, PMVS_EXPORT_DEVICE, &ap, nv, mb.vertex, nf, mb.face, tb.view, 0, nullptr, &al));
          const size_t nfa = (size_t)std::max<int64_t>(nf, 1), texels = (size_t)al.height * (size_t)al.width;
          const size_t a_view = nfa * 6 * 4, a_rgb = a_view + nfa * 4, abytes = a_rgb + std::max<size_t>(texels * 3, 1);
          char* ablock = nullptr;  // uv (float), atlas_view (int32), rgb (bytes)
          if (hipMalloc((void**)&ablock, abytes) != hipSuccess) {
            std::cerr << "pmvs2: atlas: " << abytes << " bytes of device memory" << std::endl;
            return 1;
          }
          pmvs_atlas_buffers ab{};
          ab.uv = (float*)ablock, ab.atlas_view = (int32_t*)(ablock + a_view), ab.rgb = (uint8_t*)(ablock + a_rgb);
          CHECK("atlas", pmvs_mesh_atlas(sc, PMVS_EXPORT_DEVICE, &ap, nv, mb.vertex, nf, mb.face, tb.view, al.height, &ab, &al));
          atlas_uv.resize((size_t)nf * 6), atlas_view.resize((size_t)nf), atlas_rgb.resize(texels * 3);
          if ((nf && (hipMemcpy(atlas_uv.data(), ab.uv, atlas_uv.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(atlas_view.data(), ab.atlas_view, atlas_view.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)) ||
              (texels && hipMemcpy(atlas_rgb.data(), ab.rgb, atlas_rgb.size(), hipMemcpyDeviceToHost) != hipSuccess)) {
            std::cerr << "pmvs2: atlas: the fetch failed" << std::endl;
            return 1;
          }
          (void)hipFree(ablock);
        }
        (void)hipFree(block);
        vertex.resize((size_t)nv * 3), vnormal.resize((size_t)nv * 3), vcolor.resize((size_t)nv * 3);
        face.resize((size_t)nf * 3), view.resize((size_t)nf), uv.resize((size_t)nf * 6);
        std::memcpy(vertex.data(), host.data(), vertex.size() * 4);
        std::memcpy(vnormal.data(), host.data() + off_normal, vnormal.size() * 4);
        std::memcpy(vcolor.data(), host.data() + off_color, vcolor.size());
        std::memcpy(face.data(), host.data() + off_face, face.size() * 4);
        std::memcpy(view.data(), host.data() + off_view, view.size() * 4);
        std::memcpy(uv.data(), host.data() + off_uv, uv.size() * 4);
      }
      std::vector<const char*> names((size_t)tnum);
      for (int t = 0; t < tnum; ++t) names[t] = tex_names[t].c_str();
      if (export_texmesh)
        CHECK("textured mesh ply",
              pmvs_write_ply_texmesh_binary((out + ".texmesh.ply").c_str(), nv, vertex.data(), vnormal.data(), vcolor.data(), nf,
                                            face.data(), view.data(), uv.data(), tnum, names.data(), tex_dims.data()));
      if (export_atlas) {
        // an empty atlas (no face has texels) is written as one black texel, which no face refers to
        const std::string ppm = option + ".atlas.ppm";
        int32_t adims[2] = {(int32_t)al.width, (int32_t)al.height};
        if (al.height == 0) adims[0] = adims[1] = 1, atlas_rgb.assign(3, 0);
        atlas_view.resize((size_t)nf, -1), atlas_uv.resize((size_t)nf * 6, 0.0f);
        CHECK("atlas ppm", pmvs_write_ppm((prefix + "models/" + ppm).c_str(), adims[0], adims[1], atlas_rgb.data()));
        const char* aname = ppm.c_str();
        CHECK("atlas ply",
              pmvs_write_ply_texmesh_binary((out + ".atlas.ply").c_str(), nv, vertex.data(), vnormal.data(), vcolor.data(), nf,
                                            face.data(), atlas_view.data(), atlas_uv.data(), 1, &aname, adims));
      }
    }
  }
  pmvs_scene_destroy(sc);
  pmvs_options_free(opt);
  const double t_end = now_s();
  std::fprintf(stderr,
               "---- pmvs2: %d seeds, %d patches | init %.2f s, features %.2f s, seeds %.2f s, loop %.2f s, write %.2f s "
               "----\n",
               nseeds, nmodel, t_init - t0, t_feat - t_init, t_seed - t_feat, t_loop - t_seed, t_end - t_loop);
  return 0;
}
