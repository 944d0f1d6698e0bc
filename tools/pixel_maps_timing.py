#!/usr/bin/env python3
"""pmvs_loop_pixel_maps on one loop result: the call timed with HIP events (and the host clock) in
device mode, writer order, radius csize; after one warm-up repetition.  The call returns after its work
has finished, so two events recorded around it on an otherwise idle stream bracket exactly the call.
Prints one JSON line: medians, every sample, the pixels, the filled share and the bytes returned.

  python tools/pixel_maps_timing.py                  # the C3 model: 50 views, 3840x2160, level 0
  python tools/pixel_maps_timing.py --reps 1         # under rocprofv3 --kernel-trace --stats
  python tools/pixel_maps_timing.py --lib PATH       # another build of the library (an A/B form)
"""
import argparse
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
    ap.add_argument("--radius", type=int, default=None, help="default: csize")
    ap.add_argument("--lib", default=None, help="the library to load (default: the tree's)")
    args = ap.parse_args()
    import pmvs_amd as P
    if args.lib:
        P.load_library(os.path.abspath(args.lib))

    def log(msg):
        print(f"[pixel_maps_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    radius = inp.csize if args.radius is None else args.radius
    dims, off = scene.pixel_map_layout()
    pixels, one = int(off[-1]), int(off[1])
    log(f"{n} patches, digest {digest}, {len(dims)} targets, {pixels} pixels, radius {radius}")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    kw = dict(writer_order=True, device=True, radius=radius)
    mid = len(dims) // 2
    calls = {"one_target_depth_only": lambda: scene.loop_pixel_maps(first_target=mid, num_targets=1, arrays=("depth",), **kw),
             "one_target_all_arrays": lambda: scene.loop_pixel_maps(first_target=mid, num_targets=1, **kw),
             "all_targets_all_arrays": lambda: scene.loop_pixel_maps(**kw)}
    samples = {k: [] for k in calls}
    clock = {k: [] for k in calls}
    info = {}
    for rep in range(args.reps + 1):
        for k, fn in calls.items():
            out, ms, wall = timed(fn)
            if rep > 0 or args.reps == 0:
                samples[k].append(ms)
                clock[k].append(wall)
            if rep == 0 and k == "one_target_all_arrays":
                keep = {a: t.cpu().numpy() for a, t in out.items()}
                info["one_target_filled_share"] = round(float((keep["patch"] >= 0).mean()), 4)
            if rep == 0 and k == "all_targets_all_arrays":
                info["filled_pixels"] = int((out["patch"] >= 0).sum().item())
                info["filled_share"] = round(info["filled_pixels"] / pixels, 4)
                # a range is its targets' part of the whole
                lo = int(off[mid])
                info["range_equals_part"] = all(
                    out[a][lo:lo + len(keep[a])].cpu().numpy().tobytes() == keep[a].tobytes() for a in keep)
                info["checksum"] = {a: int(out[a].view(torch.int32).to(torch.int64).sum().item()) for a in out}
                del keep
            del out
        log(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in samples.items() if v))
    assert scene.loop_hash() == int(digest, 16)
    result = {
        "workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                    f"{args.seeds} synthetic seed candidates",
        "library": args.lib or "cmvs-pmvs_amd/libpmvs_amd.so",
        "patches": n, "model_digest": digest, "targets": int(len(dims)), "pixels": pixels, "pixels_one_target": one,
        "radius": radius, **info, "reps": args.reps,
        "event_median_ms": {k: round(statistics.median(v), 2) for k, v in samples.items() if v},
        "event_samples_ms": {k: [round(x, 2) for x in v] for k, v in samples.items() if v},
        "host_clock_median_ms": {k: round(statistics.median(v), 2) for k, v in clock.items() if v},
        # patch, depth, ncc 4 bytes and normal 12 bytes per pixel
        "bytes_returned": {"all_targets_all_arrays": pixels * 24, "one_target_all_arrays": one * 24,
                           "one_target_depth_only": one * 4},
    }
    print(json.dumps(result), flush=True)
    scene.close()
    if info.get("range_equals_part") is False:
        sys.exit("pixel_maps_timing.py: a target range differs from its part of the whole")


if __name__ == "__main__":
    main()
