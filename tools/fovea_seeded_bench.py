#!/usr/bin/env python3
"""What the seeded (warm) foveated call saves (ugsm_submit_foveated_warm) -- on ONE box, in one session.

    python tools/fovea_seeded_bench.py [--rounds 3] [--out profiles/fovea_seeded_bench.json]

At 16 MP (4928 x 3264) and 1080p, 14 levels, 7 fovea levels, images and priors resident on the device, events off, every measurement a child
process of its own (one context per measurement, as tools/seeded_bench.py), the configurations of a size taking turns round by round, every
child's value kept:
  plain      ugsm_submit_foveated of the pair, centred -- the cold call of the same build;
  s6 .. s1   ugsm_submit_foveated_warm from start level 6, 5, 3 and 1, the prior the pair's cold stack, the window moved by (12, -8) pixels.
Each child measures (a) the blocking call -- submit + ugsm_wait on a one-slot context, the median wall-clock time of --reps calls after
--warmup -- and (b) a burst of --burst calls dealt round-robin onto a four-slot context, in pairs per second.
`kernel`: per start level, from the kernel statistics (profile_events = 2) of one more child per size: the starting-field launch's own
duration and the call's launches; and what that launch replaces, timed on the same stack: ugsm_reconstruct_full, then ugsm_stage_restrict
for the levels s .. 6 -- the duration of the reconstruction's kernels from the statistics, and the wall-clock time of the whole composition
against that of ugsm_stage_warm_stack (both include their waits).
`accuracy`: a synthetic sequence from synth.make_pair at 1080p -- the same scene (seed) in every frame, the truth field's amplitude raised by
--drift pixels per frame, the window moving by --step pixels per frame -- matched cold, and warm frame after frame from the previous frame's
own warm stack (frame 0: its cold stack); the RMSE of level 0's dx and dy against the truth inside the window, per start level.
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
LEVELS, F = 14, 7
STARTS = (6, 5, 3, 1)
MOVED = (12, -8)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--burst", type=int, default=64)
ap.add_argument("--frames", type=int, default=5)
ap.add_argument("--drift", type=float, default=3.0, help="pixels the truth field's amplitude grows by per frame of the accuracy sequence")
ap.add_argument("--step", type=int, default=5, help="pixels the window moves per frame of the accuracy sequence, in x and in y")
ap.add_argument("--sizes", nargs="*", default=list(SIZES))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fovea_seeded_bench.json"))
ap.add_argument("--child", choices=["time", "kernel", "accuracy"], help="(internal) measure in this process, print one JSON line")
ap.add_argument("--size", default="16mp", help="(internal)")
ap.add_argument("--start", type=int, default=-1, help="(internal) start level; -1: the plain call")
args = ap.parse_args()
TAG = "FOVEASEEDEDBENCH "


def _setup():
    sys.path.insert(0, ROOT)
    from ug_stereomatcher_amd import _lib, synth
    return _lib, synth


def _call(c, slot, dL, dR, W, H, off, dP, poff, start, dO):
    if start < 0:
        c.check(c.lib.ugsm_submit_foveated(c.handle, slot, dL, dR, W, H, 3 * W, off[0], off[1], dO, None, None))
    else:
        c.submit_foveated_warm(slot, [dL], [dR], W, H, 3 * W, [off], [dP], [poff], start, [dO])


def _stack_bytes(_lib, W, H):
    fw, fh = _lib.fovea_dims(W, H, LEVELS, F)
    return 4 * 3 * F * fw * fh, fw, fh


def time_child():
    _lib, synth = _setup()
    W, H = SIZES[args.size]
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    nbytes = _stack_bytes(_lib, W, H)[0]
    off = (0, 0) if args.start < 0 else MOVED
    with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1) as c:
        dL, dR, dP, dO = c.to_device(L), c.to_device(R), c.alloc(nbytes), c.alloc(nbytes)
        _call(c, 0, dL, dR, W, H, (0, 0), None, None, -1, dP)      # the prior: the pair's cold stack, centred
        c.check(c.lib.ugsm_wait(c.handle, 0))
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            _call(c, 0, dL, dR, W, H, off, dP, (0, 0), args.start, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[args.warmup:]
        out = dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), device_bytes=c.device_bytes())
    slots = 4
    with _lib.Context(levels=LEVELS, fovea_levels=F, slots=slots) as c:
        dL, dR, dP = c.to_device(L), c.to_device(R), c.alloc(nbytes)
        dO = [c.alloc(nbytes) for _ in range(slots)]
        _call(c, 0, dL, dR, W, H, (0, 0), None, None, -1, dP)
        c.check(c.lib.ugsm_wait(c.handle, 0))

        def run(m):
            for k in range(m):
                if k >= slots:
                    c.check(c.lib.ugsm_wait(c.handle, k % slots))
                _call(c, k % slots, dL, dR, W, H, off, dP, (0, 0), args.start, dO[k % slots])
            c.check(c.lib.ugsm_wait_all(c.handle))
        run(2 * slots)
        t0 = time.perf_counter()
        run(args.burst)
        out["burst_pairs_per_s"] = args.burst / (time.perf_counter() - t0)
    print(TAG + json.dumps(out), flush=True)


def kernel_child():
    _lib, synth = _setup()
    W, H = SIZES[args.size]
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    nbytes, fw, fh = _stack_bytes(_lib, W, H)
    sn = F * fw * fh * 4                                           # bytes of one plane of a stack
    rows, reps = {}, 8
    with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1, profile_events=2) as c:
        dL, dR, dP, dO = c.to_device(L), c.to_device(R), c.alloc(nbytes), c.alloc(nbytes)
        full, lvl = c.alloc(4 * 3 * W * H), c.alloc(4 * 3 * W * H)
        _call(c, 0, dL, dR, W, H, (0, 0), None, None, -1, dP)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        for s in STARTS:
            c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
            for _ in range(reps):
                _call(c, 0, dL, dR, W, H, MOVED, dP, (0, 0), s, dO)
                c.check(c.lib.ugsm_wait(c.handle, 0))
            st = c.kernel_stats()
            r = [x for x in st if x["name"] == "k_restrict_stack"]
            assert len(r) == 1 and r[0]["level"] == s and r[0]["launches"] == reps, r
            row = dict(levels=F - s, us_per_launch=1e3 * r[0]["total_ms"] / reps, all_kernels_ms_per_call=sum(x["total_ms"] for x in st) / reps,
                       launches_per_call=sum(x["launches"] for x in st) / reps)
            # what the launch replaces, on the same stack: reconstruct -> restrict the levels s .. F-1 (the crop would follow on the host)
            c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
            wall = []
            for _ in range(reps):
                t0 = time.perf_counter()
                c.reconstruct_full(dP, dP + sn, dP + 2 * sn, W, H, full, 0, 0)
                for k in range(s, F):
                    c.stage_restrict(full, W, H, k, lvl)
                wall.append((time.perf_counter() - t0) * 1e6)
            row["reconstruct_kernels_us"] = 1e3 * sum(x["total_ms"] for x in c.kernel_stats()) / reps
            row["composition_wall_us"] = statistics.median(wall)
            wall = []
            for _ in range(reps):
                t0 = time.perf_counter()
                c.stage_warm_stack(dP, W, H, (0, 0), MOVED, s, dO)
                wall.append((time.perf_counter() - t0) * 1e6)
            row["stage_warm_wall_us"] = statistics.median(wall)
            rows[f"s{s}"] = row
        c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
        for _ in range(reps):
            _call(c, 0, dL, dR, W, H, (0, 0), None, None, -1, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
        st = c.kernel_stats()
        rows["plain"] = dict(all_kernels_ms_per_call=sum(x["total_ms"] for x in st) / reps, launches_per_call=sum(x["launches"] for x in st) / reps)
        rows["fovea"] = [fw, fh]
    print(TAG + json.dumps(rows), flush=True)


def accuracy_child():
    _lib, synth = _setup()
    import numpy as np
    W, H = SIZES["1080p"]
    nbytes, fw, fh = _stack_bytes(_lib, W, H)
    shape = (3, F, fh, fw)

    def rmse(stack, dx, dy, off):
        x0, y0, _ = _lib.fovea_level_mapping(W, H, LEVELS, F, 0, off)          # level 0's window in the frame
        e = np.stack([stack[0, 0] - dx[y0:y0 + fh, x0:x0 + fw], stack[1, 0] - dy[y0:y0 + fh, x0:x0 + fw]]).astype(np.float64)
        return float(np.sqrt(np.nanmean(e * e)))

    frames = [synth.make_pair(W, H, synth.BASE_SEED + 2, a=0.01 + t * args.drift / W) for t in range(args.frames)]
    offs = [(t * args.step, -t * args.step) for t in range(args.frames)]
    out = dict(W=W, H=H, frames=args.frames, drift_px_per_frame=args.drift, window_step_px=args.step, offsets=offs, cold=[],
               warm={f"s{s}": [] for s in STARTS})
    with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1) as c:
        dev = [(c.to_device(L), c.to_device(R)) for L, R, _, _ in frames]
        dO = c.alloc(nbytes)
        for t, (L, R, dx, dy) in enumerate(frames):
            _call(c, 0, dev[t][0], dev[t][1], W, H, offs[t], None, None, -1, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            out["cold"].append(rmse(c.to_host(dO, shape), dx, dy, offs[t]))
        for s in STARTS:
            two = [c.alloc(nbytes), c.alloc(nbytes)]               # the call is not in place: two stacks take turns
            _call(c, 0, dev[0][0], dev[0][1], W, H, offs[0], None, None, -1, two[0])     # frame 0: cold
            c.check(c.lib.ugsm_wait(c.handle, 0))
            for t in range(1, args.frames):                        # every later frame from the previous one's stack, the window moved
                _call(c, 0, dev[t][0], dev[t][1], W, H, offs[t], two[(t - 1) % 2], offs[t - 1], s, two[t % 2])
                c.check(c.lib.ugsm_wait(c.handle, 0))
                out["warm"][f"s{s}"].append(rmse(c.to_host(two[t % 2], shape), frames[t][2], frames[t][3], offs[t]))
            for p in two:
                c.free(p)
    out["cold_mean_after_frame_0"] = statistics.mean(out["cold"][1:])
    out["warm_mean"] = {k: statistics.mean(v) for k, v in out["warm"].items()}
    print(TAG + json.dumps(out), flush=True)


def measure(kind, size="1080p", start=-1):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--size", size, "--start", str(start), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--burst", str(args.burst), "--frames", str(args.frames), "--drift", str(args.drift), "--step", str(args.step)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len(TAG):])


def main():
    sys.path.insert(0, ROOT)
    from ug_stereomatcher_amd import _lib
    result = dict(tool="tools/fovea_seeded_bench.py", levels=LEVELS, fovea_levels=F, rounds=args.rounds, reps=args.reps, burst=args.burst, moved=MOVED, sizes={})
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
        plain_pi = _lib.pixel_iterations(W, H, LEVELS, F)
        row = dict(W=W, H=H, children=kept, median_ms=med, range_ms=rng, burst_pairs_per_s=rate,
                   ms_over_plain={k: med[k] / med["plain"] for k in configs}, burst_over_plain={k: rate[k] / rate["plain"] for k in configs},
                   pixel_iterations_over_plain={k: (_lib.fovea_warm_pixel_iterations(W, H, LEVELS, F, s) if s >= 0 else plain_pi) / plain_pi
                                                for k, s in configs.items()},
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
