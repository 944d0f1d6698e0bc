#!/usr/bin/env python3
"""pmvs_loop_mesh on one loop result, split into its stages, timed with HIP events (and the host clock) in
device mode, writer order, the CLI's fuse parameters, after one warm-up repetition.  Every call returns after
its work has finished, so two events recorded around it on an otherwise idle stream bracket exactly the call.
The volume is a cube of --voxels^3 around the fused cloud's bounding box (voxel = longest extent / (voxels -
6), trunc = 3 voxels, min_obs 1).  The stages, through the public calls:
  maps_pass     pmvs_loop_tsdf into a 1 x 1 x 1 volume: the maps, the support and pass flags, one voxel
  tsdf          pmvs_loop_tsdf into the cube: maps_pass + the integration kernel
  extract       pmvs_tsdf_mesh of that volume (the second, filling call; the counting call is timed as
                extract_count)
  loop_mesh     pmvs_loop_mesh, the filling call: everything above in one call
The integration's achieved bytes/s needs the kernel's own time: run once under
`rocprofv3 --kernel-trace --stats -- python tools/mesh_timing.py --reps 1` and divide `integration_bytes` of
the JSON line by tsdf_integrate_kernel's time.
Prints one JSON line: medians, every sample, the volume, the counts and the bytes.

  python tools/mesh_timing.py                  # the C3 model: 50 views, 3840x2160, level 0; 512^3
  python tools/mesh_timing.py --out FILE       # also write the JSON there
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
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
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after one warm-up")
    ap.add_argument("--out", default=None, help="a file that receives the JSON line too")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[mesh_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    dims, off = scene.pixel_map_layout()
    pixels = int(off[-1])
    fuse = dict(writer_order=True, radius=inp.csize, min_support=2, depth_rel=0.01, normal_cos=0.5)
    coord = scene.loop_fuse(arrays=("coord",), **fuse)["coord"]
    lo, hi = coord.min(0).astype(np.float64), coord.max(0).astype(np.float64)
    voxel = float((hi - lo).max() / (args.voxels - 6))
    cube = P.volume((lo + hi) / 2 - voxel * args.voxels / 2, voxel, (args.voxels,) * 3)
    one = P.volume((lo + hi) / 2, voxel, (1, 1, 1))
    trunc = float(np.float32(3.0) * np.float32(cube.voxel))
    log(f"{n} patches, digest {digest}, {len(dims)} targets, {pixels} pixels, {len(coord)} fused points, voxel {voxel:.6g}")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    dev = torch.device("cuda", scene.device)
    flags = P.EXPORT_WRITER_ORDER | P.EXPORT_DEVICE
    prm = P.TsdfParams(P.FuseParams(inp.csize, 2, 0.01, 0.5), trunc)
    nvox = args.voxels ** 3
    vol_arrays = {"tsdf": torch.empty(nvox, dtype=torch.float32, device=dev), "obs": torch.empty(nvox, dtype=torch.uint8, device=dev),
                  "color": torch.empty(nvox * 4, dtype=torch.uint8, device=dev)}
    state = {}

    def tsdf(v):
        b = P.TsdfBuffers(*[vol_arrays[k].data_ptr() for k in ("tsdf", "obs", "color")])
        P._check(scene.lib.pmvs_loop_tsdf(scene.handle, flags, 0, len(dims), C.byref(prm), C.byref(v), C.byref(b)))

    def mesh_call(call, count_only):
        nv, nf = C.c_int64(0), C.c_int64(0)
        if count_only:
            P._check(call(0, 0, C.byref(P.MeshBuffers()), C.byref(nv), C.byref(nf)))
            state["counts"] = (int(nv.value), int(nf.value))
            return
        v, f = state["counts"]
        if "mesh" not in state:
            state["mesh"] = {"vertex": torch.empty((v, 3), dtype=torch.float32, device=dev),
                             "normal": torch.empty((v, 3), dtype=torch.float32, device=dev),
                             "color": torch.empty((v, 3), dtype=torch.uint8, device=dev),
                             "face": torch.empty((f, 3), dtype=torch.int32, device=dev)}
        b = P.MeshBuffers(*[state["mesh"][k].data_ptr() if state["mesh"][k].numel() else None
                            for k in ("vertex", "normal", "color", "face")])
        P._check(call(v, f, C.byref(b), C.byref(nv), C.byref(nf)))
        assert (int(nv.value), int(nf.value)) == (v, f)

    def extract(*a):
        return scene.lib.pmvs_tsdf_mesh(scene.handle, P.EXPORT_DEVICE, C.byref(cube), 1, vol_arrays["tsdf"].data_ptr(),
                                        vol_arrays["obs"].data_ptr(), vol_arrays["color"].data_ptr(), *a)

    def whole(*a):
        return scene.lib.pmvs_loop_mesh(scene.handle, flags, 0, len(dims), C.byref(prm), C.byref(cube), 1, *a)

    calls = {"maps_pass": lambda: tsdf(one), "tsdf": lambda: tsdf(cube), "extract_count": lambda: mesh_call(extract, True),
             "extract": lambda: mesh_call(extract, False), "loop_mesh": lambda: mesh_call(whole, False)}
    samples, clock = {k: [] for k in calls}, {k: [] for k in calls}
    for rep in range(args.reps + 1):
        for k, fn in calls.items():
            _, ms, wall = timed(fn)
            if rep > 0 or args.reps == 0:
                samples[k].append(ms)
                clock[k].append(wall)
        log(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in samples.items() if v))
    assert scene.loop_hash() == int(digest, 16)
    obs = vol_arrays["obs"]
    med = {k: round(statistics.median(v), 2) for k, v in samples.items() if v}
    result = {
        "workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                    f"{args.seeds} synthetic seed candidates",
        "patches": n, "model_digest": digest, "targets": len(dims), "pixels": pixels, "fused_points": int(len(coord)),
        "volume": {"dims": [args.voxels] * 3, "voxel": voxel, "trunc": trunc, "min_obs": 1},
        "observed_voxels": int((obs > 0).sum().item()), "inside_voxels": int((vol_arrays["tsdf"] < 0).sum().item()),
        "vertices": state["counts"][0], "faces": state["counts"][1],
        # what the integration kernel must move: the volume's 9 bytes per voxel written once, and the depth map and
        # pass flags (5 bytes per pixel of the range) read at least once
        "integration_bytes": {"volume_written": 9 * nvox, "maps_read": 5 * pixels},
        "reps": args.reps, "event_median_ms": med,
        "integration_ms_by_difference": round(med["tsdf"] - med["maps_pass"], 2) if med else None,
        "event_samples_ms": {k: [round(x, 2) for x in v] for k, v in samples.items() if v},
        "host_clock_median_ms": {k: round(statistics.median(v), 2) for k, v in clock.items() if v},
    }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    scene.close()


if __name__ == "__main__":
    main()
