#!/usr/bin/env python3
"""What the seeded full-mode call saves (ugsm_submit_full_seeded) -- on ONE box, in one session.

    python tools/seeded_bench.py [--rounds 3] [--out profiles/seeded_bench.json]

At 16 MP (4928 x 3264) and 1080p, 14 levels, images and priors resident on the device, events off, every measurement a child process of its
own (one context per measurement, as tools/lr_bench.py), the configurations of a size taking turns round by round, every child's value kept:
  plain      ugsm_submit_full_batch of one pair -- the cold call of the same build (tools/isa_dump.py --diff against the parent reports every
             existing function identical, so it is the parent's call);
  s9 .. s3   ugsm_submit_full_seeded from start level 9, 7, 5 and 3, the prior a cold result of the same pair.
Each child measures (a) the blocking call -- submit + ugsm_wait on a one-slot context, the median wall-clock time of --reps calls after
--warmup -- and (b) a burst of --burst calls dealt round-robin onto a four-slot context, in pairs per second.
`kernel`: the restriction's own time per start level, from the kernel statistics (profile_events = 2) of one more child per size.
`accuracy`: a synthetic sequence from synth.make_pair at 1080p -- the same scene (seed) in every frame, the truth field's amplitude raised by
--drift pixels per frame -- matched cold, and seeded frame after frame from the previous frame's own seeded result (frame 0: its cold
result); the RMSE of dx and dy against the truth, inside a border of 16 pixels, per start level.
Nothing is gated here: the table says what came out (DESIGN.md section 8 quotes it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"16mp": (4928, 3264), "1080p": (1920, 1080)}
LEVELS = 14
STARTS = (9, 7, 5, 3)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--burst", type=int, default=64)
ap.add_argument("--frames", type=int, default=5)
ap.add_argument("--drift", type=float, default=3.0, help="pixels the truth field's amplitude grows by per frame of the accuracy sequence")
ap.add_argument("--sizes", nargs="*", default=list(SIZES))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_bench.json"))
ap.add_argument("--child", choices=["time", "kernel", "accuracy"], help="(internal) measure in this process, print one JSON line")
ap.add_argument("--size", default="16mp", help="(internal)")
ap.add_argument("--start", type=int, default=-1, help="(internal) start level; -1: the plain call")
args = ap.parse_args()


def _setup():
    sys.path.insert(0, ROOT)
    from ug_stereomatcher_amd import _lib, synth
    return _lib, synth


def _call(c, slot, dL, dR, W, H, dP, start, dO):
    if start < 0:
        c.submit_full_batch(slot, [dL], [dR], W, H, 3 * W, [dO])
    else:
        c.submit_full_seeded(slot, [dL], [dR], W, H, 3 * W, [dP], start, [dO])


def time_child():
    _lib, synth = _setup()
    W, H = SIZES[args.size]
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    nbytes = 3 * W * H * 4
    with _lib.Context(levels=LEVELS, slots=1) as c:
        dL, dR, dP, dO = c.to_device(L), c.to_device(R), c.alloc(nbytes), c.alloc(nbytes)
        _call(c, 0, dL, dR, W, H, None, -1, dP)                    # the prior: the pair's cold result
        c.check(c.lib.ugsm_wait(c.handle, 0))
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            _call(c, 0, dL, dR, W, H, dP, args.start, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[args.warmup:]
        out = dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), device_bytes=c.device_bytes())
    slots = 4
    with _lib.Context(levels=LEVELS, slots=slots) as c:
        dL, dR, dP = c.to_device(L), c.to_device(R), c.alloc(nbytes)
        dO = [c.alloc(nbytes) for _ in range(slots)]
        _call(c, 0, dL, dR, W, H, None, -1, dP)
        c.check(c.lib.ugsm_wait(c.handle, 0))

        def run(m):
            for k in range(m):
                if k >= slots:
                    c.check(c.lib.ugsm_wait(c.handle, k % slots))
                _call(c, k % slots, dL, dR, W, H, dP, args.start, dO[k % slots])
            c.check(c.lib.ugsm_wait_all(c.handle))
        run(2 * slots)
        t0 = time.perf_counter()
        run(args.burst)
        out["burst_pairs_per_s"] = args.burst / (time.perf_counter() - t0)
    print("SEEDEDBENCH " + json.dumps(out), flush=True)


def kernel_child():
    _lib, synth = _setup()
    W, H = SIZES[args.size]
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    nbytes = 3 * W * H * 4
    w, h = _lib.level_dims(W, H, LEVELS)
    rows = {}
    with _lib.Context(levels=LEVELS, slots=1, profile_events=2) as c:
        dL, dR, dP, dO = c.to_device(L), c.to_device(R), c.alloc(nbytes), c.alloc(nbytes)
        _call(c, 0, dL, dR, W, H, None, -1, dP)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        for s in STARTS:
            c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
            for _ in range(8):
                _call(c, 0, dL, dR, W, H, dP, s, dO)
                c.check(c.lib.ugsm_wait(c.handle, 0))
            st = c.kernel_stats()
            r = [x for x in st if x["name"] == "k_restrict"]
            assert len(r) == 1 and r[0]["level"] == s and r[0]["launches"] == 8, r
            rows[f"s{s}"] = dict(w=w[s], h=h[s], us_per_launch=1e3 * r[0]["total_ms"] / r[0]["launches"],
                                 all_kernels_ms_per_call=sum(x["total_ms"] for x in st) / 8,
                                 launches_per_call=sum(x["launches"] for x in st) / 8)
        c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
        for _ in range(8):
            _call(c, 0, dL, dR, W, H, None, -1, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
        st = c.kernel_stats()
        rows["plain"] = dict(all_kernels_ms_per_call=sum(x["total_ms"] for x in st) / 8, launches_per_call=sum(x["launches"] for x in st) / 8)
    print("SEEDEDBENCH " + json.dumps(rows), flush=True)


def accuracy_child():
    _lib, synth = _setup()
    import numpy as np
    W, H = SIZES["1080p"]
    b = 16

    def rmse(f, dx, dy):
        e = np.stack([f[0] - dx, f[1] - dy])[:, b:-b, b:-b].astype(np.float64)
        return float(np.sqrt(np.nanmean(e * e)))

    frames = [synth.make_pair(W, H, synth.BASE_SEED + 2, a=0.01 + t * args.drift / W) for t in range(args.frames)]
    out = dict(W=W, H=H, frames=args.frames, drift_px_per_frame=args.drift, border=b, cold=[], seeded={f"s{s}": [] for s in STARTS})
    with _lib.Context(levels=LEVELS, slots=1) as c:
        nbytes = 3 * W * H * 4
        dO = c.alloc(nbytes)
        dev = [(c.to_device(L), c.to_device(R)) for L, R, _, _ in frames]
        for t, (L, R, dx, dy) in enumerate(frames):
            _call(c, 0, dev[t][0], dev[t][1], W, H, None, -1, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            out["cold"].append(rmse(c.to_host(dO, (3, H, W)), dx, dy))
        for s in STARTS:
            dF = c.alloc(nbytes)
            _call(c, 0, dev[0][0], dev[0][1], W, H, None, -1, dF)  # frame 0: cold
            c.check(c.lib.ugsm_wait(c.handle, 0))
            for t in range(1, args.frames):                        # every later frame from the previous one's field, in place
                _call(c, 0, dev[t][0], dev[t][1], W, H, dF, s, dF)
                c.check(c.lib.ugsm_wait(c.handle, 0))
                out["seeded"][f"s{s}"].append(rmse(c.to_host(dF, (3, H, W)), frames[t][2], frames[t][3]))
            c.free(dF)
    out["cold_mean_after_frame_0"] = statistics.mean(out["cold"][1:])
    out["seeded_mean"] = {k: statistics.mean(v) for k, v in out["seeded"].items()}
    print("SEEDEDBENCH " + json.dumps(out), flush=True)


def measure(kind, size="1080p", start=-1):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--size", size, "--start", str(start), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--burst", str(args.burst), "--frames", str(args.frames), "--drift", str(args.drift)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SEEDEDBENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("SEEDEDBENCH "):])


def main():
    sys.path.insert(0, ROOT)
    from ug_stereomatcher_amd import _lib
    result = dict(tool="tools/seeded_bench.py", levels=LEVELS, rounds=args.rounds, reps=args.reps, burst=args.burst, sizes={})
    for size in args.sizes:
        W, H = SIZES[size]
        configs = {"plain": -1, **{f"s{s}": s for s in STARTS}}
        kept = {k: [] for k in configs}
        for rnd in range(args.rounds):
            names = list(configs)
            for name in (names if rnd % 2 == 0 else names[::-1]):     # alternating order
                kept[name].append(measure("time", size, configs[name]))
                print(size, name, kept[name][-1], flush=True)
        med = {k: statistics.median(v["ms"] for v in kept[k]) for k in configs}
        rng = {k: max(v["ms"] for v in kept[k]) - min(v["ms"] for v in kept[k]) for k in configs}
        rate = {k: statistics.median(v["burst_pairs_per_s"] for v in kept[k]) for k in configs}
        row = dict(W=W, H=H, children=kept, median_ms=med, range_ms=rng, burst_pairs_per_s=rate,
                   ms_over_plain={k: med[k] / med["plain"] for k in configs}, burst_over_plain={k: rate[k] / rate["plain"] for k in configs},
                   pixel_iterations_over_plain={k: (_lib.seeded_pixel_iterations(W, H, LEVELS, s) if s >= 0 else _lib.pixel_iterations(W, H, LEVELS, 0))
                                                / _lib.pixel_iterations(W, H, LEVELS, 0) for k, s in configs.items()},
                   kernel=measure("kernel", size))
        result["sizes"][size] = row
        print(json.dumps({k: v for k, v in row.items() if k != "children"}), flush=True)
    result["accuracy"] = measure("accuracy")
    print(json.dumps(result["accuracy"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    {"time": time_child, "kernel": kernel_child, "accuracy": accuracy_child, None: main}[args.child]()
