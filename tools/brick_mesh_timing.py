#!/usr/bin/env python3
"""pmvs_loop_brick_mesh against pmvs_loop_mesh on one loop result, timed with HIP events (and the host clock) in
device mode, writer order, the CLI's fuse parameters, after one warm-up repetition, the two alternating within
each repetition.  Every call returns after its work has finished, so two events recorded around it on an
otherwise idle stream bracket exactly the call.  Two parts:
  same volume   tools/mesh_timing.py's cube of --voxels^3 around the fused cloud (trunc = 3 voxels, min_obs 1):
                loop_mesh (dense) and loop_brick_mesh (margin --margin), the filling calls, and their counts;
                brick_tsdf is pmvs_loop_brick_tsdf's counting call (maps, mark, scan) and brick_count the brick
                mesh's counting call (those, the integration and the classification, no sort)
  fine volumes  for each of --cells: pmvs_brick_volume_from_points(cloud, cells, 3), the brick mesh alone: the
                bricks, the bytes they hold (8 + 512 * 9 each), the (voxel, target) pairs, vertices, faces, times;
                a volume that does not fit is reported as such (PMVS_ENOMEM), not retried
The per-kernel split needs the kernels' own times: run once under
`rocprofv3 --kernel-trace --stats -- python tools/brick_mesh_timing.py --reps 1`.
Prints one JSON line: medians, every sample, the volumes, the counts and the bytes.

  python tools/brick_mesh_timing.py                  # the C3 model: 50 views, 3840x2160, level 0; 512^3; 2048, 4096
  python tools/brick_mesh_timing.py --out FILE       # also write the JSON there
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
    ap.add_argument("--voxels", type=int, default=512, help="the shared cube's edge in voxels (0: skip that part)")
    ap.add_argument("--cells", type=int, nargs="*", default=[2048, 4096], help="the fine volumes' longest side in cells")
    ap.add_argument("--margin", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after one warm-up")
    ap.add_argument("--out", default=None, help="a file that receives the JSON line too")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[brick_mesh_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    dims, off = scene.pixel_map_layout()
    pixels, targets = int(off[-1]), len(dims)
    coord = scene.loop_fuse(arrays=("coord",), writer_order=True, radius=inp.csize, min_support=2, depth_rel=0.01,
                            normal_cos=0.5)["coord"]
    log(f"{n} patches, digest {digest}, {targets} targets, {pixels} pixels, {len(coord)} fused points")

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
    fuse = P.FuseParams(inp.csize, 2, 0.01, 0.5)

    def mesh_pair(call):
        """(count, fill): the counting call, which records the counts, and the filling call into device arrays."""
        state = {}

        def count():
            nv, nf = C.c_int64(0), C.c_int64(0)
            P._check(call(0, 0, C.byref(P.MeshBuffers()), C.byref(nv), C.byref(nf)))
            state["counts"] = (int(nv.value), int(nf.value))

        def fill():
            v, f = state["counts"]
            if "mesh" not in state:
                state["mesh"] = [torch.empty((v, 3), dtype=torch.float32, device=dev), torch.empty((v, 3), dtype=torch.float32, device=dev),
                                 torch.empty((v, 3), dtype=torch.uint8, device=dev), torch.empty((f, 3), dtype=torch.int32, device=dev)]
            b = P.MeshBuffers(*[t.data_ptr() if t.numel() else None for t in state["mesh"]])
            nv, nf = C.c_int64(0), C.c_int64(0)
            P._check(call(v, f, C.byref(b), C.byref(nv), C.byref(nf)))
            assert (int(nv.value), int(nf.value)) == (v, f)

        return state, count, fill

    def brick_calls(vol, trunc):
        bp = P.BrickParams(P.TsdfParams(fuse, trunc), args.margin)
        nb = C.c_int64(0)

        def select():
            P._check(scene.lib.pmvs_loop_brick_tsdf(scene.handle, flags, 0, targets, C.byref(bp), C.byref(vol), 0,
                                                    C.byref(P.BrickBuffers()), C.byref(nb)))

        state, count, fill = mesh_pair(lambda *a: scene.lib.pmvs_loop_brick_mesh(scene.handle, flags, 0, targets, C.byref(bp),
                                                                                 C.byref(vol), 1, *a))
        return nb, state, {"brick_tsdf": select, "brick_count": count, "loop_brick_mesh": fill}

    def run(calls):
        samples, clock = {k: [] for k in calls}, {k: [] for k in calls}
        for rep in range(args.reps + 1):
            for k, fn in calls.items():
                _, ms, wall = timed(fn)
                if rep > 0 or args.reps == 0:
                    samples[k].append(ms)
                    clock[k].append(wall)
            log(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in samples.items() if v))
        return {"event_median_ms": {k: round(statistics.median(v), 2) for k, v in samples.items() if v},
                "event_samples_ms": {k: [round(x, 2) for x in v] for k, v in samples.items() if v},
                "host_clock_median_ms": {k: round(statistics.median(v), 2) for k, v in clock.items() if v}}

    def brick_report(vol, nb, state):
        b = int(nb.value)
        return {"dims": list(vol.dims), "voxel": float(vol.voxel), "margin": args.margin,
                "grid_bricks": int(np.prod([(d + 7) // 8 for d in vol.dims])), "bricks": b, "stored_voxels": 512 * b,
                "brick_bytes": (8 + 512 * 9) * b, "voxel_target_pairs": 512 * b * targets,
                "vertices": state["counts"][0], "faces": state["counts"][1]}

    result = {"workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                          f"{args.seeds} synthetic seed candidates",
              "patches": n, "model_digest": digest, "targets": targets, "pixels": pixels, "fused_points": int(len(coord)),
              "reps": args.reps}
    lo, hi = coord.min(0).astype(np.float64), coord.max(0).astype(np.float64)
    if args.voxels:
        voxel = float((hi - lo).max() / (args.voxels - 6))
        cube = P.volume((lo + hi) / 2 - voxel * args.voxels / 2, voxel, (args.voxels,) * 3)
        trunc = float(np.float32(3.0) * np.float32(cube.voxel))
        tp = P.TsdfParams(fuse, trunc)
        dstate, dcount, dfill = mesh_pair(lambda *a: scene.lib.pmvs_loop_mesh(scene.handle, flags, 0, targets, C.byref(tp),
                                                                             C.byref(cube), 1, *a))
        nb, bstate, bcalls = brick_calls(cube, trunc)
        dcount()
        times = run({"loop_mesh": dfill, **bcalls})
        same = dstate["counts"] == bstate["counts"] and all(torch.equal(a, b) for a, b in zip(dstate["mesh"], bstate["mesh"]))
        result["same_volume"] = {"dense": {"voxels": args.voxels ** 3, "voxel_target_pairs": args.voxels ** 3 * targets,
                                           "vertices": dstate["counts"][0], "faces": dstate["counts"][1]},
                                 "brick": brick_report(cube, nb, bstate), "meshes_identical": bool(same), **times}
        del dstate, bstate
        torch.cuda.empty_cache()
    result["fine"] = []
    for cells in args.cells:
        vol = P.brick_volume_from_points(coord, cells, 3)
        nb, state, calls = brick_calls(vol, float(np.float32(3.0) * np.float32(vol.voxel)))
        try:
            times = run(calls)
            result["fine"].append({"cells": cells, "fits": True, **brick_report(vol, nb, state), **times})
        except P.PmvsError as e:
            result["fine"].append({"cells": cells, "fits": False, "dims": list(vol.dims), "bricks": int(nb.value), "error": str(e)[:200]})
        del state
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
