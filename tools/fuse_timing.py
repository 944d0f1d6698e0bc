#!/usr/bin/env python3
"""pmvs_loop_fuse on one loop result: the call timed with HIP events (and the host clock) in device mode,
writer order, the CLI's parameters (radius csize, min_support 2, depth_rel 0.01, normal_cos 0.5); after one
warm-up repetition, which is also the counting call that sizes the point arrays.  The call returns after
its work has finished, so two events recorded around it on an otherwise idle stream bracket exactly the
call.  pmvs_loop_pixel_maps over the same ranges is timed in the same session as the scale.
Prints one JSON line: medians, every sample, the pixels, the points and the support histogram.

  python tools/fuse_timing.py                  # the C3 model: 50 views, 3840x2160, level 0
  python tools/fuse_timing.py --reps 1         # under rocprofv3 --kernel-trace --stats
  python tools/fuse_timing.py --out FILE       # also write the JSON there
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after one warm-up")
    ap.add_argument("--out", default=None, help="a file that receives the JSON line too")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[fuse_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    dims, off = scene.pixel_map_layout()
    tnum, mid = len(dims), len(dims) // 2
    log(f"{n} patches, digest {digest}, {tnum} targets, {int(off[-1])} pixels, radius {inp.csize}")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    flags = P.EXPORT_WRITER_ORDER | P.EXPORT_DEVICE
    prm = P.FuseParams(inp.csize, 2, 0.01, 0.5)
    ranges = {"all_targets": (0, tnum), "one_target": (mid, 1)}
    bufs, counts = {}, {}

    def fuse(name):
        first, num = ranges[name]
        pixels = int(off[first + num] - off[first])
        cnt = C.c_int64(0)
        if name not in bufs:  # the counting call, then every array of the call
            P._check(scene.lib.pmvs_loop_fuse(scene.handle, flags, first, num, C.byref(prm), 0, C.byref(P.FuseBuffers()),
                                              C.byref(cnt)))
            counts[name] = int(cnt.value)
            bufs[name] = scene._new_arrays(P.FuseBuffers, scene.FUSE_ARRAYS, None, True, px=pixels, n=counts[name])
        out, b = bufs[name]
        P._check(scene.lib.pmvs_loop_fuse(scene.handle, flags, first, num, C.byref(prm), counts[name], C.byref(b), C.byref(cnt)))
        assert int(cnt.value) == counts[name]
        return out

    calls = {"fuse_one_target": lambda: fuse("one_target"),
             "pixel_maps_one_target": lambda: scene.loop_pixel_maps(writer_order=True, device=True, first_target=mid, num_targets=1),
             "fuse_all_targets": lambda: fuse("all_targets"),
             "pixel_maps_all_targets": lambda: scene.loop_pixel_maps(writer_order=True, device=True)}
    samples = {k: [] for k in calls}
    clock = {k: [] for k in calls}
    info = {}
    for rep in range(args.reps + 1):
        for k, fn in calls.items():
            out, ms, wall = timed(fn)
            if rep > 0 or args.reps == 0:
                samples[k].append(ms)
                clock[k].append(wall)
            if rep == 0 and k.startswith("fuse_"):
                name = k[len("fuse_"):]
                sm = out["support_map"]
                hist = torch.bincount(sm.to(torch.int64), minlength=4).cpu().tolist()
                info[name] = {"pixels": int(sm.numel()), "points": counts[name], "support_histogram_all_pixels": hist,
                              "point_support_histogram": torch.bincount(out["support"].to(torch.int64), minlength=4).cpu().tolist(),
                              "checksum": {a: int(t.reshape(-1).to(torch.float64).nan_to_num(0.0, 0.0, 0.0).sum().item())
                                           for a, t in out.items() if a in ("support_map", "pixel", "patch", "color")}}
            if rep == 0 and k == "pixel_maps_all_targets":
                info["filled_pixels"] = int((out["patch"] >= 0).sum().item())
            del out
        log(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in samples.items() if v))
    assert scene.loop_hash() == int(digest, 16)
    result = {
        "workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                    f"{args.seeds} synthetic seed candidates",
        "patches": n, "model_digest": digest, "targets": int(tnum),
        "params": {"radius": int(inp.csize), "min_support": 2, "depth_rel": 0.01, "normal_cos": 0.5}, **info,
        "reps": args.reps,
        "event_median_ms": {k: round(statistics.median(v), 2) for k, v in samples.items() if v},
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
