#!/usr/bin/env python3
"""pmvs_mesh_raster and pmvs_mesh_texture over all targets of one loop result, timed with HIP events (and the host
clock) in device mode after one warm-up repetition.  Every call returns after its work has finished, so two events
recorded around it on an otherwise idle stream bracket exactly the call.  Three meshes of the same model, each
obtained in device mode and kept there:
  mesh      `pmvs2 ... MESH`'s: pmvs_loop_mesh in pmvs_volume_from_points(cloud, 256, 3)
  cube      tools/mesh_timing.py's cube of --voxels^3 around the fused cloud
  finemesh  `pmvs2 ... FINEMESH`'s: pmvs_loop_brick_mesh in pmvs_brick_volume_from_points(cloud, --cells, 3), margin 5
(trunc = 3 voxels, min_obs 1, writer order, the CLI's fuse parameters; texture: depth_rel 0.01, min_area 0).
Per mesh: the samples of both calls, the share of faces with a view, the histogram of views, and the peak of the
device memory in use during a call above what was in use before it (sampled from another thread: the scratch).
The per-kernel split needs the kernels' own times: run once under
`rocprofv3 --kernel-trace --stats -- python tools/texmesh_timing.py --reps 1 --only NAME`.
Prints one JSON line.

  python tools/texmesh_timing.py                  # the C3 model: 50 views, 3840x2160, level 0
  python tools/texmesh_timing.py --out FILE       # also write the JSON there
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmvs-pmvs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=5000)
    ap.add_argument("--wave", type=int, default=32768)
    ap.add_argument("--min-candidates", type=int, default=131072)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--voxels", type=int, default=512, help="the cube's edge in voxels")
    ap.add_argument("--cells", type=int, default=2048, help="the fine volume's longest side in cells")
    ap.add_argument("--only", nargs="*", default=["mesh", "cube", "finemesh"], help="the meshes to time")
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after one warm-up")
    ap.add_argument("--out", default=None, help="a file that receives the JSON line too")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[texmesh_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    dims, off = scene.pixel_map_layout()
    pixels, targets = int(off[-1]), len(dims)
    prm = dict(writer_order=True, radius=inp.csize, min_support=2, depth_rel=0.01, normal_cos=0.5)
    coord = scene.loop_fuse(arrays=("coord",), **prm)["coord"]
    log(f"{n} patches, digest {digest}, {targets} targets, {pixels} pixels, {len(coord)} fused points")
    dev = torch.device("cuda", scene.device)

    def timed(fn):
        """(event ms, host clock ms, the peak of the device memory in use above the level before the call)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info(dev)[0]
        low, stop = [before], threading.Event()

        def sample():
            while not stop.is_set():
                low[0] = min(low[0], torch.cuda.mem_get_info(dev)[0])
                time.sleep(0.0005)

        th = threading.Thread(target=sample)
        th.start()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        stop.set()
        th.join()
        return e0.elapsed_time(e1), wall, before - low[0]

    lo, hi = coord.min(0).astype(np.float64), coord.max(0).astype(np.float64)

    def make_mesh(name):
        if name == "mesh":
            vol = P.volume_from_points(coord, 256, 3)
            return vol, scene.loop_mesh(vol, float(np.float32(3.0) * np.float32(vol.voxel)), device=True, arrays=("vertex", "face"), **prm)
        if name == "cube":
            voxel = float((hi - lo).max() / (args.voxels - 6))
            vol = P.volume((lo + hi) / 2 - voxel * args.voxels / 2, voxel, (args.voxels,) * 3)
            return vol, scene.loop_mesh(vol, float(np.float32(3.0) * np.float32(vol.voxel)), device=True, arrays=("vertex", "face"), **prm)
        vol = P.brick_volume_from_points(coord, args.cells, 3)
        return vol, scene.loop_brick_mesh(vol, float(np.float32(3.0) * np.float32(vol.voxel)), 5, device=True,
                                          arrays=("vertex", "face"), **prm)

    result = {"workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                          f"{args.seeds} synthetic seed candidates",
              "patches": n, "model_digest": digest, "targets": targets, "pixels": pixels, "fused_points": int(len(coord)),
              "reps": args.reps, "meshes": {}}
    tp = P.TextureParams(0.01, 0.0)
    for name in args.only:
        vol, m = make_mesh(name)
        vertex, face = m["vertex"], m["face"]
        nv, nf = len(vertex), len(face)
        log(f"{name}: dims {list(vol.dims)}, {nv} vertices, {nf} faces")
        rface = torch.empty(pixels, dtype=torch.int32, device=dev)
        rdepth = torch.empty(pixels, dtype=torch.float32, device=dev)
        view = torch.empty(nf, dtype=torch.int32, device=dev)
        uv = torch.empty((nf, 6), dtype=torch.float32, device=dev)
        score = torch.empty(nf, dtype=torch.float32, device=dev)
        rb = P.RasterBuffers(rface.data_ptr(), rdepth.data_ptr())
        tb = P.TextureBuffers(view.data_ptr(), uv.data_ptr(), score.data_ptr())
        head = (scene.handle, P.EXPORT_DEVICE, 0, targets)
        mesh = (nv, vertex.data_ptr(), nf, face.data_ptr())
        calls = {"mesh_raster": lambda: P._check(scene.lib.pmvs_mesh_raster(*head, *mesh, C.byref(rb))),
                 "mesh_texture": lambda: P._check(scene.lib.pmvs_mesh_texture(*head, C.byref(tp), *mesh, C.byref(tb)))}
        samples, clock, peak = {k: [] for k in calls}, {k: [] for k in calls}, {k: 0 for k in calls}
        for rep in range(args.reps + 1):
            for k, fn in calls.items():
                ms, wall, scratch = timed(fn)
                peak[k] = max(peak[k], int(scratch))
                if rep > 0 or args.reps == 0:
                    samples[k].append(ms)
                    clock[k].append(wall)
            log(f"{name} rep {rep}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in samples.items() if v))
        hist = torch.bincount(view.long() + 1, minlength=targets + 1).cpu().numpy()
        result["meshes"][name] = {
            "dims": list(vol.dims), "voxel": float(vol.voxel), "vertices": nv, "faces": nf,
            "filled_pixels": int((rface >= 0).sum()), "faces_with_view": int(nf - hist[0]),
            "share_with_view": round(float(nf - hist[0]) / max(nf, 1), 4), "view_histogram": [int(x) for x in hist[1:]],
            "median_score": float(score[view >= 0].median()) if nf - hist[0] else 0.0,
            "event_median_ms": {k: round(statistics.median(v), 2) for k, v in samples.items()},
            "event_samples_ms": {k: [round(x, 2) for x in v] for k, v in samples.items()},
            "host_clock_median_ms": {k: round(statistics.median(v), 2) for k, v in clock.items()},
            "peak_scratch_bytes": peak}
        del m, vertex, face, rface, rdepth, view, uv, score
        torch.cuda.empty_cache()
    assert scene.loop_hash() == int(digest, 16)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    scene.close()


if __name__ == "__main__":
    main()
