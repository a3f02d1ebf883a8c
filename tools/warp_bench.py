#!/usr/bin/env python3
"""What the warped right image and the photometric residual cost (ugsm_warp_right, ugsm_photometric_residual and the two fovea forms) --
on ONE box, in one session.

    python tools/warp_bench.py [--rounds 3] [--out profiles/warp_bench.json]

At 16 MP (4928 x 3264) and 1080p, 14 / 7 levels, everything resident on the device, events off.  Every measurement is a child process of
its own (one context per process, as tools/lr_bench.py); a child measures the four calls of one size one after the other, and the rounds
repeat the children.  A call is asynchronous, so a child times a REGION: `reps` calls enqueued back to back on the slot's stream and one
ugsm_wait behind them, host clock around both, after a warm-up region of the same shape; reps is chosen per call so that the region lasts
about --region seconds.  The full-resolution forms run on the synthetic pair's images and its true (smooth) field with a confidence plane;
the fovea forms on the stacks and pyramid stacks a foveated call of the same pair wrote on the device.

Per call the file holds the time per call (the median over the children, every child's value kept, and the spread max - min), the
algorithmic bytes -- what the definition has to move, computed from the shapes by algorithmic_bytes() below -- the achieved bytes per
second, and that rate as a share of the HBM peak (MI355X: 8.0 TB/s by the specification; 6.29 TB/s measured with a float4 copy) and as a
multiple of the host-link copy rate of profiles/r06_pcie_probe.txt (one hipMemcpyAsync, the way the reference's form moves every plane).
No threshold: neither the reference nor the parent commit has a device form to compare with."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"16mp": (4928, 3264), "1080p": (1920, 1080)}
LEVELS, F = 14, 7
CALLS = ["warp_right", "photometric_residual", "warp_right_fovea", "photometric_residual_fovea"]
HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12   # bytes / s

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--region", type=float, default=0.4, help="seconds a timed region should last")
ap.add_argument("--sizes", nargs="*", default=list(SIZES))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.json"))
ap.add_argument("--child", action="store_true", help="(internal) measure in this process, print one JSON line")
ap.add_argument("--size", default="16mp", help="(internal)")
args = ap.parse_args()


def algorithmic_bytes(call, W, H, fw, fh):
    """Bytes the definition moves, rgb8 images: a pixel's (dx, dy) once, the gathered right pixel once, what is written once."""
    px, fpx = W * H, F * fw * fh
    return {
        "warp_right": px * (8 + 3 + 12),                    # (dx, dy), one rgb8 pixel, three floats out
        "photometric_residual": px * (8 + 4 + 3 + 3) + 2 * 32 * H,   # (dx, dy), conf, a left and a right pixel; the row sums out and in
        "warp_right_fovea": fpx * (8 + 12 + 12),            # (dx, dy), three gathered floats, three floats out, per pixel of a level
        "photometric_residual_fovea": fpx * (8 + 4 + 12 + 12) + 2 * 32 * F * fh,
    }[call]


def link_copy_rate():
    """bytes / s of one hipMemcpyAsync over the host link, from profiles/r06_pcie_probe.txt"""
    for line in open(os.path.join(ROOT, "profiles", "r06_pcie_probe.txt")):
        m = re.match(r"^down, .*one hipMemcpyAsync\s+[\d.]+ ms\s+([\d.]+) GB/s", line)
        if m:
            return float(m.group(1)) * 1e9
    raise SystemExit("profiles/r06_pcie_probe.txt: no 'down ... one hipMemcpyAsync' line")


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    from ug_stereomatcher_amd import _lib, synth
    W, H = SIZES[args.size]
    fw, fh = _lib.fovea_dims(W, H, LEVELS, F)
    n, fn = W * H, fw * fh
    L, R, dx, dy = synth.make_pair(W, H, synth.BASE_SEED + 2)
    out = {}
    with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dF = c.to_device(np.stack([dx, dy, np.full((H, W), 0.75, np.float32)]).astype(np.float32))
        dW, dSums = c.alloc(3 * n * 4), c.alloc(F * 4 * 8)
        dS, dPL, dPR, dFW = (c.alloc(3 * F * fn * 4) for _ in range(4))
        c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dL, dR, W, H, 3 * W, 0, 0, dS, dPL, dPR))
        c.check(c.lib.ugsm_wait(c.handle, 0))
        so, h = c.lib, c.handle
        calls = {
            "warp_right": lambda: so.ugsm_warp_right(h, 0, dR, W, H, 3 * W, dF, dF + 4 * n, dW),
            "photometric_residual": lambda: so.ugsm_photometric_residual(h, 0, dL, dR, W, H, 3 * W, dF, dF + 4 * n, dF + 8 * n, dSums),
            "warp_right_fovea": lambda: so.ugsm_warp_right_fovea(h, 0, dPR, dS, dS + 4 * F * fn, fw, fh, dFW),
            "photometric_residual_fovea": lambda: so.ugsm_photometric_residual_fovea(h, 0, dPL, dPR, dS, dS + 4 * F * fn, dS + 8 * F * fn, fw, fh,
                                                                                     dSums),
        }

        def region(f, reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                st = f()
                if st:
                    c.check(st)
            c.check(so.ugsm_wait(h, 0))
            return time.perf_counter() - t0

        for name in CALLS:
            f = calls[name]
            region(f, 20)                                            # first launches: code objects, the scratch
            reps = int(min(max(args.region / (region(f, 50) / 50), 50), 20000))
            region(f, reps)                                          # warm-up of the timed shape
            dt = region(f, reps)
            out[name] = dict(us_per_call=dt / reps * 1e6, reps=reps, region_s=dt)
    print("WARPBENCH " + json.dumps(out), flush=True)


def measure(size):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", size, "--region", str(args.region)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("WARPBENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][10:])


def main():
    sys.path.insert(0, ROOT)
    from ug_stereomatcher_amd import _lib
    link = link_copy_rate()
    result = dict(tool="tools/warp_bench.py", levels=LEVELS, fovea_levels=F, rounds=args.rounds, region_s=args.region,
                  hbm_peak_spec_bytes_per_s=HBM_PEAK_SPEC, hbm_peak_measured_bytes_per_s=HBM_PEAK_MEASURED, link_copy_bytes_per_s=link,
                  timing="host clock around `reps` calls enqueued back to back and one ugsm_wait; per call = region / reps", sizes={})
    for size in args.sizes:
        W, H = SIZES[size]
        fw, fh = _lib.fovea_dims(W, H, LEVELS, F)
        kept = []
        for rnd in range(args.rounds):
            kept.append(measure(size))
            print(size, rnd, {k: round(v["us_per_call"], 2) for k, v in kept[-1].items()}, flush=True)
        row = dict(W=W, H=H, fovW=fw, fovH=fh, calls={})
        for name in CALLS:
            us = [k[name]["us_per_call"] for k in kept]
            med = statistics.median(us)
            nbytes = algorithmic_bytes(name, W, H, fw, fh)
            rate = nbytes / (med * 1e-6)
            row["calls"][name] = dict(us_per_call=med, us_per_call_children=us, spread_us=max(us) - min(us), reps=[k[name]["reps"] for k in kept],
                                      algorithmic_bytes=nbytes, bytes_per_s=rate, share_of_hbm_peak_spec=rate / HBM_PEAK_SPEC,
                                      share_of_hbm_peak_measured=rate / HBM_PEAK_MEASURED, times_link_copy_rate=rate / link)
        result["sizes"][size] = row
        print(json.dumps(row["calls"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    child() if args.child else main()
