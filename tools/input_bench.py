#!/usr/bin/env python3
"""The input formats (ugsm_set_input_format, UGSM_INPUT_*) on the device: what reading bgr8, rgba8, bgra8 or mono8 in place costs or saves
against rgb8, and what the float formats rgb32f and mono32f (four times the input bytes) cost.

    python tools/input_bench.py [--rounds 2] [--pairs 32] [--reps 8] [--out profiles/input_format_bench.json]
    python tools/input_bench.py --formats rgb8 rgb32f mono32f --out profiles/input_format_float_bench.json

For 16 MP (4928 x 3264) and 1080p, per format, in child processes that take turns format by format (the order reversed every round, as
tools/ab.py alternates its configurations; every child under `timeout -k 10`), one context per process:
  - pyr_base_tiled_us / pyr_base_stream_us: K-pyr-base per image, from the library's in-dispatch events (profile_events 2, the
    "k_pyr_base" statistic: its total over its launches, two per call) -- full calls run the LDS-tiled k_pyr_base, foveated calls the
    streaming k_pyr_base_march; median over --reps calls;
  - device_pairs_s: --pairs full-mode pairs through the queue (ugsm_enqueue_full, four slots, device-resident images), after a warm-up burst;
  - managed_pairs_s / host_pairs_s: the same from host memory -- ugsm_enqueue_full_managed (any memory: copied into the library's staging)
    and ugsm_enqueue_full_host (page-locked images and result planes);
  - service_ms: the node's service call, ugsm_match_full from pageable memory into pageable planes, median of --reps wall-clock calls.
Rates and times are the median over the rounds; min, max and every child's value are kept.  Prints one JSON line per row and writes them all to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"16mp": (4928, 3264), "1080p": (1920, 1080)}
NAMES = ["rgb8", "bgr8", "rgba8", "bgra8", "mono8"]  # the default run: the 8-bit formats, name -> UGSM_INPUT_* by position
FLOAT = {"rgb32f": 8, "mono32f": 9}                   # integer-valued float images of the same pair: the same match, four times the input bytes


def child(args):
    import encode_np as en
    import float_np as fl
    from ug_stereomatcher_amd import _lib, synth
    W, H = SIZES[args.size]
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 3)
    if args.fmt in FLOAT:
        fmt = FLOAT[args.fmt]
        a, b = fl.encode(L, fmt), fl.encode(R, fmt)
    else:
        fmt = NAMES.index(args.fmt)
        a, b = en.encode(L, fmt), en.encode(R, fmt)
    row = a[0].nbytes
    out = dict(size=args.size, W=W, H=H, format=args.fmt, bytes_per_pixel=_lib.input_bytes_per_pixel(fmt), image_MB=row * H / 1e6)

    # K-pyr-base per image, both forms (slot 0 carries the events)
    with _lib.Context(levels=14, fovea_levels=7, slots=1, profile_events=2) as c:
        c.set_input_format(fmt)
        dl, dr = c.to_device(a), c.to_device(b)
        fw, fh = _lib.fovea_dims(W, H, 14, 7)
        do, ds = c.alloc(3 * W * H * 4), c.alloc(3 * 7 * fw * fh * 4)

        def pyr_us(call):
            vals = []
            for k in range(args.reps + 2):
                c.reset_kernel_stats()
                call()
                c.check(c.lib.ugsm_wait(c.handle, 0))
                st = [s for s in c.kernel_stats() if s["name"] == "k_pyr_base"]
                if k >= 2:
                    vals.append(1000.0 * sum(s["total_ms"] for s in st) / sum(s["launches"] for s in st))
            return float(np.median(vals))
        out["pyr_base_tiled_us"] = pyr_us(lambda: c.check(c.lib.ugsm_submit_full(c.handle, 0, dl, dr, W, H, row, do)))
        out["pyr_base_stream_us"] = pyr_us(lambda: c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dl, dr, W, H, row, 0, 0, ds, None, None)))
        for p in (dl, dr, do, ds):
            c.free(p)

    # the queue: device-resident, managed and page-locked host memory
    with _lib.Context(levels=14, slots=4, batch=1) as c:
        c.set_input_format(fmt)
        dl, dr = c.to_device(a), c.to_device(b)
        douts = [c.alloc(3 * W * H * 4) for _ in range(5)]
        hl, hr = c.host_array(a.shape, a.dtype), c.host_array(b.shape, b.dtype)
        hl[...], hr[...] = a, b
        houts = [c.host_array((3, H, W), np.float32) for _ in range(5)]

        def burst(enqueue, n):  # (completions fetched as they come: at most (slots + 1) x batch pairs may be outstanding)
            for k in range(n):
                enqueue(k)
                while c.next_done(False) is not None:
                    pass
            c.drain()

        def rate(enqueue):
            burst(enqueue, 8)
            t0 = time.perf_counter()
            burst(enqueue, args.pairs)
            return args.pairs / (time.perf_counter() - t0)
        out["device_pairs_s"] = rate(lambda k: c.enqueue_full(dl, dr, W, H, row, douts[k % 5], k))
        out["managed_pairs_s"] = rate(lambda k: c.enqueue_full_managed(a, b, k))
        out["host_pairs_s"] = rate(lambda k: c.enqueue_full_host(hl, hr, houts[k % 5], k))
        for p in [dl, dr] + douts:
            c.free(p)

    # the service call from pageable memory
    with _lib.Context(levels=14, slots=1) as c:
        c.set_input_format(fmt)
        res = np.empty((3, H, W), np.float32)
        ms = []
        for k in range(args.reps + 2):
            t0 = time.perf_counter()
            c.check(c.lib.ugsm_match_full(c.handle, a.ctypes.data, b.ctypes.data, W, H, row, res[0].ctypes.data, res[1].ctypes.data,
                                          res[2].ctypes.data))
            if k >= 2:
                ms.append(1000.0 * (time.perf_counter() - t0))
        out["service_ms"] = float(np.median(ms))
    print("ROW " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--sizes", nargs="*", default=list(SIZES))
    ap.add_argument("--formats", nargs="*", default=NAMES, choices=NAMES + list(FLOAT))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_format_bench.json"))
    ap.add_argument("--child", action="store_true", help="(internal) measure one size and format, print one ROW line")
    ap.add_argument("--size", default="16mp")
    ap.add_argument("--fmt", default="rgb8")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {}
    for r in range(args.rounds):
        for size in args.sizes:
            order = args.formats if r % 2 == 0 else args.formats[::-1]
            for f in order:
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--size", size, "--fmt", f,
                       "--pairs", str(args.pairs), "--reps", str(args.reps)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
                if p.returncode != 0 or not rows:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                    raise SystemExit(f"child {size} {f} failed with status {p.returncode}; stopping")
                runs.setdefault((size, f), []).append(json.loads(rows[0]))
                sys.stderr.write(f"[input_bench] round {r + 1} of {args.rounds}: {size} {f} done\n")
                sys.stderr.flush()
    keys = ["pyr_base_tiled_us", "pyr_base_stream_us", "device_pairs_s", "managed_pairs_s", "host_pairs_s", "service_ms"]
    table = []
    for (size, f), rs in runs.items():
        row = {k: rs[0][k] for k in ("size", "W", "H", "format", "bytes_per_pixel", "image_MB")}
        row["rounds"], row["pairs"], row["reps"] = len(rs), args.pairs, args.reps
        for k in keys:
            v = [x[k] for x in rs]
            row[k] = round(statistics.median(v), 3)
            row[k + "_min"], row[k + "_max"] = round(min(v), 3), round(max(v), 3)
            row[k + "_runs"] = [round(x, 3) for x in v]  # (one value per child process, in round order)
        print(json.dumps(row), flush=True)
        table.append(row)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/input_bench.py", "rounds": args.rounds, "pairs": args.pairs, "reps": args.reps, "rows": table}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
