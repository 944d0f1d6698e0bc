#!/usr/bin/env python3
"""From "loop finished" to "writer-ready arrays on the host", two ways, on one loop result:
  (a) host: pmvs_loop_fetch of the 1608-byte records, pmvs2's former host ordering and gather, and
      pmvs_patch_colors (tools/export_timing_host.cpp, built here with g++ -O2);
  (b) device: pmvs_loop_export_sizes + pmvs_loop_export in writer order (the arrays pmvs2 ... PATCH asks for).
Both run in one process on the same model, (b) first (the fetch consumes the result), after one
warm-up repetition; the arrays of the two are compared once.  Prints one JSON line: the medians, every
sample, the bytes each path moves over PCIe and the gather kernel's algorithmic bytes.

  python tools/export_timing.py                      # the C3 model: 50 views, 3840x2160, level 0
  python tools/export_timing.py --reps 1 --no-host   # under rocprofv3 --kernel-trace --stats
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmvs-pmvs_amd"))


def build_host_path(tmp):
    so = os.path.join(tmp, "export_timing_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "export_timing_host.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    lib.host_path.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.host_path_take.argtypes = [C.c_void_p] * 6
    lib.host_path_take.restype = None
    return lib


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
    ap.add_argument("--no-host", action="store_true", help="time only the device export (profiler runs)")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[export_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    lib = scene.lib
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    log(f"scene ready, {len(seeds)} seed patches")
    tnum, num = inp.num_targets, len(inp.images)
    gwidth = np.array([((img.shape[1] >> inp.level) + inp.csize - 1) // inp.csize for img in inp.images], np.int32)
    index2image = np.arange(num, dtype=np.int32)
    tmp = tempfile.TemporaryDirectory()
    host = None if args.no_host else build_host_path(tmp.name)
    names = ("fields", "colors", "image_off", "image_ids", "vimage_off", "vimage_ids")

    samples = {"device": [], "device_sizes": [], "host": [], "host_fetch": [], "host_order_gather": [], "host_colors": []}
    info = {}
    for rep in range(args.reps + 1):
        n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                              min_candidates=args.min_candidates, fetch=False)
        digest = f"{scene.loop_hash():016x}"
        # (b) sizes, the caller's arrays, the export
        t0 = time.perf_counter()
        sz = P.ExportSizes()
        P._check(lib.pmvs_loop_export_sizes(scene.handle, C.byref(sz)))
        t1 = time.perf_counter()
        out, buf = scene._new_arrays(P.ExportBuffers, scene.EXPORT_ARRAYS, names, False, n=sz.patches, n1=sz.patches + 1,
                                     e=sz.image_entries, v=sz.vimage_entries)
        P._check(lib.pmvs_loop_export(scene.handle, P.EXPORT_WRITER_ORDER, P._ptr(index2image), C.byref(buf)))
        t2 = time.perf_counter()
        e, ve = int(sz.image_entries), int(sz.vimage_entries)
        rec = {"device": t2 - t0, "device_sizes": t1 - t0}
        if host is not None:
            # (a) fetch, host ordering and gather, colours
            secs, ent = (C.c_double * 3)(), (C.c_longlong * 2)()
            t0 = time.perf_counter()
            st = host.host_path(scene.handle, n, tnum, P._ptr(gwidth), P._ptr(index2image),
                                C.cast(lib.pmvs_loop_fetch, C.c_void_p), C.cast(lib.pmvs_patch_colors, C.c_void_p),
                                secs, ent)
            t1 = time.perf_counter()
            P._check(st)
            rec.update(host=t1 - t0, host_fetch=secs[0], host_order_gather=secs[1], host_colors=secs[2])
            want = {"fields": np.empty((n, 11), np.float32), "colors": np.empty((n, 3), np.int32),
                    "nimg": np.empty(n, np.int32), "ids": np.empty(ent[0], np.int32), "nvimg": np.empty(n, np.int32),
                    "vids": np.empty(ent[1], np.int32)}
            host.host_path_take(*[P._ptr(want[k]) for k in ("fields", "colors", "nimg", "ids", "nvimg", "vids")])
            if rep == 0:  # the two paths give the same arrays
                same = (ent[0] == e and ent[1] == ve
                        and out["fields"].tobytes() == want["fields"].tobytes()
                        and out["colors"].tobytes() == want["colors"].tobytes()
                        and np.array_equal(np.diff(out["image_off"]), want["nimg"])
                        and np.array_equal(np.diff(out["vimage_off"]), want["nvimg"])
                        and np.array_equal(out["image_ids"], want["ids"]) and np.array_equal(out["vimage_ids"], want["vids"]))
                info["arrays_identical"] = bool(same)
            del want
        log(f"rep {rep}: {n} patches, digest {digest}, " + ", ".join(f"{k} {v * 1e3:.1f} ms" for k, v in rec.items()))
        info.update(patches=n, image_entries=e, vimage_entries=ve, model_digest=digest)
        if rep > 0 or args.reps == 0:
            for k, v in rec.items():
                samples[k].append(v)
        del out

    n, e, ve = info["patches"], info["image_entries"], info["vimage_entries"]
    result = {
        "workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} iterations, "
                    f"{args.seeds} synthetic seed candidates",
        **info,
        "reps": args.reps,
        "median_ms": {k: round(statistics.median(v) * 1e3, 2) for k, v in samples.items() if v},
        "samples_ms": {k: [round(x * 1e3, 2) for x in v] for k, v in samples.items() if v},
        # bytes over PCIe: (a) every record down, then coordinates, offsets and lists up and the colours down;
        # (b) fields, colours, two offset arrays and two id lists down (the index2image table up)
        "pcie_bytes": {"host": n * 1608 + n * 16 + (n + 1) * 4 + e * 4 + n * 12,
                       "device": n * (44 + 12) + 2 * 8 * (n + 1) + 4 * (e + ve) + 4 * num},
        # export_gather_kernel's algorithmic bytes for these arrays: read the 72-byte header, the int16 lists,
        # the row's source index and offsets and 4 texels of 4 bytes per image entry; written 56 bytes per
        # patch and 4 per list entry
        "gather_bytes": {"read": n * (72 + 4 + 2 * 2 * 8) + 2 * (e + ve) + 16 * e, "written": n * 56 + 4 * (e + ve)},
    }
    if samples["host"]:
        result["device_not_slower"] = result["median_ms"]["device"] <= result["median_ms"]["host"]
    print(json.dumps(result), flush=True)
    scene.close()
    if info.get("arrays_identical") is False:
        sys.exit("export_timing.py: the device export differs from the host path")


if __name__ == "__main__":
    main()
