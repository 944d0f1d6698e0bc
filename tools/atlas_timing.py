#!/usr/bin/env python3
"""pmvs_mesh_atlas over one loop result, timed with HIP events (and the host clock) in device mode after one warm-up
repetition.  The call returns after its work has finished, so two events recorded around it on an otherwise idle
stream bracket exactly the call.  Two meshes of the same model, each obtained in device mode and kept there, with the
views pmvs_mesh_texture gives them (depth_rel 0.01, min_area 0) and the CLI's atlas defaults (width 8192, max_side
64, scale 1):
  mesh      `pmvs2 ... MESH`'s: pmvs_loop_mesh in pmvs_volume_from_points(cloud, 256, 3)
  finemesh  `pmvs2 ... FINEMESH`'s: pmvs_loop_brick_mesh in pmvs_brick_volume_from_points(cloud, --cells, 3), margin 5
Per mesh: the sizing call and the render call (rgb, uv and atlas_view; texel_face is not asked for, as the CLI), the
layout (H, the placed faces, the cells), the share of non-EMPTY texels (from one extra call that asks for
texel_face), the render's texels per second and the peak of the device memory in use during a call above what was in
use before it (sampled from another thread: the scratch).  The per-kernel split needs the kernels' own times: run
once under `rocprofv3 --kernel-trace --stats -- python tools/atlas_timing.py --reps 1 --only NAME`.
Prints one JSON line.

  python tools/atlas_timing.py                  # the C3 model: 50 views, 3840x2160, level 0
  python tools/atlas_timing.py --out FILE       # also write the JSON there
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
    ap.add_argument("--cells", type=int, default=2048, help="the fine volume's longest side in cells")
    ap.add_argument("--atlas-width", type=int, default=8192)
    ap.add_argument("--max-side", type=int, default=64)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", nargs="*", default=["mesh", "finemesh"], help="the meshes to time")
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after one warm-up")
    ap.add_argument("--out", default=None, help="a file that receives the JSON line too")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[atlas_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    prm = dict(writer_order=True, radius=inp.csize, min_support=2, depth_rel=0.01, normal_cos=0.5)
    coord = scene.loop_fuse(arrays=("coord",), **prm)["coord"]
    log(f"{n} patches, digest {digest}, {len(coord)} fused points")
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

    def make_mesh(name):
        if name == "mesh":
            vol = P.volume_from_points(coord, 256, 3)
            return vol, scene.loop_mesh(vol, float(np.float32(3.0) * np.float32(vol.voxel)), device=True, arrays=("vertex", "face"), **prm)
        vol = P.brick_volume_from_points(coord, args.cells, 3)
        return vol, scene.loop_brick_mesh(vol, float(np.float32(3.0) * np.float32(vol.voxel)), 5, device=True,
                                          arrays=("vertex", "face"), **prm)

    result = {"workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                          f"{args.seeds} synthetic seed candidates",
              "patches": n, "model_digest": digest, "fused_points": int(len(coord)), "reps": args.reps,
              "atlas": {"width": args.atlas_width, "max_side": args.max_side, "scale": args.scale}, "meshes": {}}
    ap_ = P.AtlasParams(args.atlas_width, args.max_side, args.scale)
    for name in args.only:
        vol, m = make_mesh(name)
        vertex, face = m["vertex"], m["face"]
        nv, nf = len(vertex), len(face)
        view = scene.mesh_texture(vertex, face, depth_rel=0.01, min_area=0.0, device=True, arrays=("view",))["view"]
        log(f"{name}: dims {list(vol.dims)}, {nv} vertices, {nf} faces, {int((view >= 0).sum())} with a view")
        layout = P.AtlasLayout()
        head = (scene.handle, P.EXPORT_DEVICE, C.byref(ap_), nv, vertex.data_ptr(), nf, face.data_ptr(), view.data_ptr())
        P._check(scene.lib.pmvs_mesh_atlas(*head, 0, None, C.byref(layout)))
        H, W = int(layout.height), args.atlas_width
        rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        uv = torch.empty((nf, 6), dtype=torch.float32, device=dev)
        av = torch.empty(nf, dtype=torch.int32, device=dev)
        buf = P.AtlasBuffers(rgb=rgb.data_ptr(), uv=uv.data_ptr(), atlas_view=av.data_ptr())
        calls = {"sizing": lambda: P._check(scene.lib.pmvs_mesh_atlas(*head, 0, None, C.byref(layout))),
                 "render": lambda: P._check(scene.lib.pmvs_mesh_atlas(*head, H, C.byref(buf), C.byref(layout)))}
        samples, clock, peak = {k: [] for k in calls}, {k: [] for k in calls}, {k: 0 for k in calls}
        for rep in range(args.reps + 1):
            for k, fn in calls.items():
                ms, wall, scratch = timed(fn)
                peak[k] = max(peak[k], int(scratch))
                if rep > 0 or args.reps == 0:
                    samples[k].append(ms)
                    clock[k].append(wall)
            log(f"{name} rep {rep}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in samples.items() if v))
        # the share of non-EMPTY texels, from one call that asks for texel_face alone (atlases of up to 2^31 texels)
        filled, slab = 0, max(1, (1 << 31) // W)
        tf = torch.empty((min(slab, max(H, 1)), W), dtype=torch.int32, device=dev)
        if H <= slab:
            P._check(scene.lib.pmvs_mesh_atlas(*head, H, C.byref(P.AtlasBuffers(texel_face=tf.data_ptr())), C.byref(layout)))
            filled = int((tf[:H] >= 0).sum())
        else:
            filled = None   # only the first min(H, cap) rows can be asked for: a taller atlas is not sampled
        texels = H * W
        med = statistics.median(samples["render"]) if samples["render"] else 0.0
        result["meshes"][name] = {
            "dims": list(vol.dims), "voxel": float(vol.voxel), "vertices": nv, "faces": nf, "faces_with_view": int((view >= 0).sum()),
            "layout": layout.as_dict(), "texels": texels, "non_empty_texels": filled,
            "non_empty_share": None if filled is None or not texels else round(filled / texels, 4),
            "rgb_bytes": texels * 3,
            "event_median_ms": {k: round(statistics.median(v), 2) for k, v in samples.items()},
            "event_samples_ms": {k: [round(x, 2) for x in v] for k, v in samples.items()},
            "host_clock_median_ms": {k: round(statistics.median(v), 2) for k, v in clock.items()},
            "render_call_gtexels_per_s": round(texels / med / 1e6, 3) if med else None,
            "peak_scratch_bytes": peak}
        del m, vertex, face, view, rgb, uv, av, tf
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
