#!/usr/bin/env python3
"""pmvs_loop_depth_maps on one loop result: the call timed with HIP events (and the host clock) in
host mode and in device mode, all four arrays, writer order; after one warm-up repetition.  The call
returns after its work has finished, so two events recorded around it on an otherwise idle stream
bracket exactly the call.  Prints one JSON line: medians, every sample, the cells, the filled cells and
the bytes returned.

  python tools/depth_maps_timing.py                  # the C3 model: 50 views, 3840x2160, level 0
  python tools/depth_maps_timing.py --reps 1         # under rocprofv3 --kernel-trace --stats
"""
import argparse
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
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after one warm-up")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[depth_maps_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    dims, off = scene.depth_map_layout()
    cells = int(off[-1])
    log(f"{n} patches, digest {digest}, {cells} cells")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    calls = {"host": lambda: scene.loop_depth_maps(writer_order=True),
             "device": lambda: scene.loop_depth_maps(writer_order=True, device=True),
             "device_model_order": lambda: scene.loop_depth_maps(writer_order=False, device=True),
             "device_depth_only": lambda: scene.loop_depth_maps(writer_order=True, device=True, arrays=("depth",))}
    samples = {k: [] for k in calls}
    clock = {k: [] for k in calls}
    info = {}
    for rep in range(args.reps + 1):
        for k, fn in calls.items():
            out, ms, wall = timed(fn)
            if rep > 0 or args.reps == 0:
                samples[k].append(ms)
                clock[k].append(wall)
            if rep == 0 and k == "host":
                info["filled_cells"] = int((out["patch"] >= 0).sum())
                keep = out
            if rep == 0 and k == "device":
                info["device_equals_host"] = all(out[a].cpu().numpy().tobytes() == keep[a].tobytes() for a in keep)
                del keep
            del out
        log(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in samples.items() if v))
    assert scene.loop_hash() == int(digest, 16)
    result = {
        "workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                    f"{args.seeds} synthetic seed candidates",
        "patches": n, "model_digest": digest, "targets": int(len(dims)), "cells": cells, **info,
        "reps": args.reps,
        "event_median_ms": {k: round(statistics.median(v), 2) for k, v in samples.items() if v},
        "event_samples_ms": {k: [round(x, 2) for x in v] for k, v in samples.items() if v},
        "host_clock_median_ms": {k: round(statistics.median(v), 2) for k, v in clock.items() if v},
        # patch, depth, ncc 4 bytes and normal 12 bytes per cell
        "bytes_returned": {"all_arrays": cells * 24, "depth_only": cells * 4},
    }
    print(json.dumps(result), flush=True)
    scene.close()
    if info.get("device_equals_host") is False:
        sys.exit("depth_maps_timing.py: device mode differs from host mode")


if __name__ == "__main__":
    main()
