#!/usr/bin/env python3
"""From "loop finished" to "the .ply / .patch / .pset file written", two ways, on one loop result:
  (a) baseline: pmvs_loop_export of the arrays the file needs to the host, then the host writer
      (pmvs_write_ply / _patches / _pset: ostream formatting) to a file;
  (b) text: pmvs_loop_text to the host (a size query, one buffer, the call), then one write of the buffer
      to a file in the same directory;
and (c) pmvs_loop_text in device mode, the call alone (size query included, the buffer allocated once).
All run in one process on the same model (none of them consumes it); per kind one warm-up of each path,
then `reps` timed repetitions, (a) and (b) alternating.  The files of (a) and (b) are compared once.
Prints one JSON line: per kind the file's size, the medians, the ranges, every sample, and whether (b)'s
slowest repetition is faster than (a)'s fastest.

  python tools/text_export_timing.py                    # the C3 model: 50 views, 3840x2160, level 0
  python tools/text_export_timing.py --reps 1 --only-text   # under rocprofv3 --kernel-trace --stats
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

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
    ap.add_argument("--only-text", action="store_true", help="time only pmvs_loop_text (profiler runs)")
    ap.add_argument("--kinds", default="ply,patch,pset", help="the kinds to time, comma separated")
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    args = ap.parse_args()
    import pmvs_amd as P

    def log(msg):
        print(f"[text_export_timing] {msg}", file=sys.stderr, flush=True)

    inp, sp = P.synth_scene(args.views, args.width, args.height, level=args.level, supersample=2, nthreads=16)
    scene = P.Scene(inp)
    lib = scene.lib
    cands = P.synth_candidates(sp, inp.projections, args.seeds, seed=0x5EED)  # bench.py's synthetic seed model
    seeds = P.patches_from_refined(scene.refine_batch(cands)[0])
    log(f"scene ready, {len(seeds)} seed patches")
    index2image = np.arange(len(inp.images), dtype=np.int32)
    n, _ = scene.run_loop(seeds, inp.threshold, iterations=args.iterations, wave=args.wave,
                          min_candidates=args.min_candidates, fetch=False)
    digest = f"{scene.loop_hash():016x}"
    log(f"loop finished: {n} patches, digest {digest}")
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    kinds = (("ply", P.TEXT_PLY, ("fields", "colors")),
             ("patch", P.TEXT_PATCH, ("fields", "image_off", "image_ids", "vimage_off", "vimage_ids")),
             ("pset", P.TEXT_PSET, ("fields",)))
    kinds = [k for k in kinds if k[0] in args.kinds.split(",")]

    def baseline(name, arrays, path):
        t0 = time.perf_counter()
        a = scene.loop_export(writer_order=True, index2image=index2image, arrays=arrays)
        t1 = time.perf_counter()
        f = a["fields"]
        if name == "ply":
            st = lib.pmvs_write_ply(path.encode(), n, P._ptr(f), P._ptr(a["colors"]))
        elif name == "pset":
            st = lib.pmvs_write_pset(path.encode(), n, P._ptr(f))
        else:
            nimg = np.diff(a["image_off"]).astype(np.int32)
            nvimg = np.diff(a["vimage_off"]).astype(np.int32)
            st = lib.pmvs_write_patches(path.encode(), n, P._ptr(f), P._ptr(nimg), P._ptr(a["image_ids"]), P._ptr(nvimg),
                                        P._ptr(a["vimage_ids"]))
        P._check(st)
        t2 = time.perf_counter()
        return {"baseline": t2 - t0, "baseline_export": t1 - t0, "baseline_writer": t2 - t1}

    def text(kind, path):
        t0 = time.perf_counter()
        buf = scene.loop_text(kind, writer_order=True, index2image=index2image)
        t1 = time.perf_counter()
        with open(path, "wb") as fh:
            fh.write(memoryview(buf))
        t2 = time.perf_counter()
        return {"text": t2 - t0, "text_call": t1 - t0, "text_write": t2 - t1}

    def device(kind, out):
        t0 = time.perf_counter()
        scene.loop_text(kind, writer_order=True, index2image=index2image, device=True, out=out)
        return {"device_call": time.perf_counter() - t0}

    result = {"workload": f"{args.views} views {args.width}x{args.height} level {args.level}, {args.iterations} "
                          f"iterations, {args.seeds} synthetic seed candidates",
              "patches": n, "model_digest": digest, "reps": args.reps, "kinds": {}}
    identical = True
    for name, kind, arrays in kinds:
        pa, pb = os.path.join(tmp.name, "a." + name), os.path.join(tmp.name, "b." + name)
        samples = {}
        out = None
        for rep in range(args.reps + 1):
            rec = {}
            if not args.only_text:
                rec.update(baseline(name, arrays, pa))
            rec.update(text(kind, pb))
            if out is None:
                out = torch.empty(os.path.getsize(pb), dtype=torch.uint8, device=torch.device("cuda", scene.device))
            rec.update(device(kind, out))
            if rep == 0 and not args.only_text:
                with open(pa, "rb") as fa, open(pb, "rb") as fb:
                    same = True
                    while same:
                        x, y = fa.read(1 << 26), fb.read(1 << 26)
                        same = x == y
                        if not x:
                            break
                identical = identical and same
                log(f"{name}: files identical: {same}")
            log(f"{name} rep {rep}: " + ", ".join(f"{k} {v * 1e3:.1f} ms" for k, v in rec.items()))
            if rep > 0 or args.reps == 0:
                for k, v in rec.items():
                    samples.setdefault(k, []).append(v)
        entry = {"file_bytes": os.path.getsize(pb),
                 "median_ms": {k: round(statistics.median(v) * 1e3, 2) for k, v in samples.items()},
                 "range_ms": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in samples.items()},
                 "samples_ms": {k: [round(x * 1e3, 2) for x in v] for k, v in samples.items()}}
        if "baseline" in samples:
            entry["text_faster_beyond_ranges"] = max(samples["text"]) < min(samples["baseline"])
        result["kinds"][name] = entry
        del out
        for p in (pa, pb):
            if os.path.exists(p):
                os.remove(p)
    if not args.only_text:
        result["files_identical"] = identical
    result["model_digest_after"] = f"{scene.loop_hash():016x}"
    print(json.dumps(result), flush=True)
    scene.close()
    if not identical:
        sys.exit("text_export_timing.py: the device text differs from the host writers' file")


if __name__ == "__main__":
    main()
