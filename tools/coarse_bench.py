#!/usr/bin/env python3
"""What the two halves of a full-mode call cost (ugsm_submit_full_coarse, ugsm_submit_full_fine) -- on ONE box, in one session.

    python tools/coarse_bench.py [--parent-tree DIR] [--rounds 3] [--out profiles/coarse_bench.json]

At 16 MP (4928 x 3264) and 1080p, 14 levels, images resident on the device, events off, every measurement a child process of its own (one
context per measurement, as tools/seeded_bench.py), the configurations of a size taking turns round by round in alternating order, every
child's value kept:
  plain        ugsm_submit_full_batch of one pair on this build;
  parent       the same call on a build of the parent commit, where --parent-tree names a tree that holds one (DIR/ug_stereomatcher_amd with
               its libraries): tools/isa_dump.py --diff reports every existing function identical, so the two must agree within the spread;
  c1 .. c5     ugsm_submit_full_coarse, stop level 1 .. 5, no d_full;
  cf1 .. cf5   the same with a d_full entry: the prolongation launch runs;
  both2, both5 ugsm_submit_full_coarse + ugsm_submit_full_fine on one slot, no wait in between: the plain call plus the second pyramid build.
Each child measures (a) the blocking call -- submit + ugsm_wait on a one-slot context, the median wall-clock time of --reps calls after
--warmup -- and (b) a burst of --burst calls dealt round-robin onto a four-slot context, in pairs per second.
`kernel` (one more child per size, profile_events = 2): k_prolong's own duration at stop level 1 .. 5 from the kernel statistics of
ugsm_stage_prolong, and the summed k_seed durations of the same prolongation done as e ugsm_stage_seed launches through intermediates -- the
parent's kernel, bit-equal output (asserted here) --, each the median of --kreps runs; the bytes the single launch writes per second, and
the bytes it writes plus the state read once.
`pixel_iterations`: the shares of ugsm_coarse_pixel_iterations beside the times.  Nothing is gated here: the table says what came out
(DESIGN.md section 8 quotes it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"16mp": (4928, 3264), "1080p": (1920, 1080)}
LEVELS = 14
STOPS = (1, 2, 3, 4, 5)
BOTH = (2, 5)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--burst", type=int, default=64)
ap.add_argument("--kreps", type=int, default=9)
ap.add_argument("--sizes", nargs="*", default=list(SIZES))
ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libraries built")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_bench.json"))
ap.add_argument("--child", choices=["time", "kernel"], help="(internal) measure in this process, print one JSON line")
ap.add_argument("--size", default="16mp", help="(internal)")
ap.add_argument("--case", default="plain", help="(internal)")
ap.add_argument("--tree", default=ROOT, help="(internal) the tree whose package the child loads")
ap.add_argument("--images", default=None, help="(internal) an .npz with the pair")
args = ap.parse_args()


def _setup():
    sys.path.insert(0, args.tree)
    from ug_stereomatcher_amd import _lib
    import numpy as np
    z = np.load(args.images)
    return _lib, np, np.ascontiguousarray(z["L"]), np.ascontiguousarray(z["R"])


def time_child():
    _lib, np, L, R = _setup()
    W, H = SIZES[args.size]
    case = args.case
    e = int(case.lstrip("cfboth")) if case not in ("plain", "parent") else 0
    nbytes = 3 * W * H * 4
    if e:
        w, h = _lib.level_dims(W, H, LEVELS)
        sbytes = 3 * w[e] * h[e] * 4

    def buffers(c, slots):
        dS = [c.alloc(sbytes) for _ in range(slots)] if e else None
        dO = [c.alloc(nbytes) for _ in range(slots)] if (not e or case.startswith(("cf", "both"))) else None
        return dS, dO

    def call(c, slot, dL, dR, dS, dO):
        if not e:
            c.submit_full_batch(slot, [dL], [dR], W, H, 3 * W, [dO[slot]])
        elif case.startswith("both"):
            c.submit_full_coarse(slot, [dL], [dR], W, H, 3 * W, e, [dS[slot]], None)
            c.submit_full_fine(slot, [dL], [dR], W, H, 3 * W, [dS[slot]], e, [dO[slot]])
        else:
            c.submit_full_coarse(slot, [dL], [dR], W, H, 3 * W, e, [dS[slot]], [dO[slot]] if dO else None)

    with _lib.Context(levels=LEVELS, slots=1) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dS, dO = buffers(c, 1)
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            call(c, 0, dL, dR, dS, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[args.warmup:]
        out = dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), device_bytes=c.device_bytes())
    slots = 4
    with _lib.Context(levels=LEVELS, slots=slots) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dS, dO = buffers(c, slots)

        def run(m):
            for k in range(m):
                if k >= slots:
                    c.check(c.lib.ugsm_wait(c.handle, k % slots))
                call(c, k % slots, dL, dR, dS, dO)
            c.check(c.lib.ugsm_wait_all(c.handle))
        run(2 * slots)
        t0 = time.perf_counter()
        run(args.burst)
        out["burst_pairs_per_s"] = args.burst / (time.perf_counter() - t0)
    print("COARSEBENCH " + json.dumps(out), flush=True)


def kernel_child():
    _lib, np, L, R = _setup()
    W, H = SIZES[args.size]
    w, h = _lib.level_dims(W, H, LEVELS)
    nbytes = 3 * W * H * 4
    rows = {}

    def stat(c, name):
        st = [x for x in c.kernel_stats() if x["name"] == name and x["launches"] > 0]
        return sum(x["total_ms"] for x in st) * 1e3, sum(x["launches"] for x in st)

    with _lib.Context(levels=LEVELS, slots=1, profile_events=2) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dA, dB = c.alloc(nbytes), c.alloc(nbytes)            # the chain's two intermediates / its result
        dF = c.alloc(nbytes)
        for e in STOPS:
            dS = c.alloc(3 * w[e] * h[e] * 4)
            c.submit_full_coarse(0, [dL], [dR], W, H, 3 * W, e, [dS], None)   # a real state of level e
            c.check(c.lib.ugsm_wait(c.handle, 0))
            one, chain = [], []
            for _ in range(args.kreps):
                c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
                c.stage_prolong(dS, W, H, e, dF)
                us, n = stat(c, "k_prolong")
                assert n == 1, n
                one.append(us)
                c.check(c.lib.ugsm_reset_kernel_stats(c.handle))
                src, dst = dS, dA
                for l in range(e - 1, -1, -1):
                    c.check(c.lib.ugsm_stage_seed(c.handle, src, w[l + 1], h[l + 1], dst, w[l], h[l], 0, 0, 0, 0))
                    src, dst = dst, (dB if dst == dA else dA)
                us, n = stat(c, "k_seed")
                assert n == e, (n, e)
                chain.append(us)
            same = bool(np.array_equal(c.to_host(dF, (3 * H * W,)).view(np.uint32), c.to_host(src, (3 * H * W,)).view(np.uint32)))
            assert same, f"level {e}: the single launch and the chain of k_seed launches differ"
            us = statistics.median(one)
            rows[f"e{e}"] = dict(w=w[e], h=h[e], k_prolong_us=us, k_prolong_us_min=min(one), k_prolong_us_max=max(one),
                                 k_seed_chain_us=statistics.median(chain), k_seed_chain_us_min=min(chain), k_seed_chain_us_max=max(chain),
                                 chain_bytes_written=sum(3 * w[l] * h[l] * 4 for l in range(e)), bytes_written=nbytes,
                                 written_GB_per_s=nbytes / us / 1e3, state_bytes=3 * w[e] * h[e] * 4,
                                 GB_per_s=(nbytes + 3 * w[e] * h[e] * 4) / us / 1e3, bit_equal=same)
            c.free(dS)
    print("COARSEBENCH " + json.dumps(rows), flush=True)


def measure(kind, size, case, images, tree=ROOT):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--size", size, "--case", case, "--reps", str(args.reps), "--warmup", str(args.warmup),
           "--burst", str(args.burst), "--kreps", str(args.kreps), "--tree", tree, "--images", images]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("COARSEBENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("COARSEBENCH "):])


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    from ug_stereomatcher_amd import _lib, synth
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit(f"{parent}: no built ug_stereomatcher_amd/libugsm.so")
    result = dict(tool="tools/coarse_bench.py", levels=LEVELS, rounds=args.rounds, reps=args.reps, burst=args.burst, kreps=args.kreps,
                  parent_measured=bool(parent), sizes={})
    with tempfile.TemporaryDirectory() as tmp:
        for size in args.sizes:
            W, H = SIZES[size]
            L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
            images = os.path.join(tmp, size + ".npz")
            np.savez(images, L=L, R=R)                                  # (made once: the children only load it)
            configs = ["plain"] + (["parent"] if parent else []) + [f"c{e}" for e in STOPS] + [f"cf{e}" for e in STOPS] + [f"both{e}" for e in BOTH]
            kept = {k: [] for k in configs}
            for rnd in range(args.rounds):
                for name in (configs if rnd % 2 == 0 else configs[::-1]):   # alternating order
                    kept[name].append(measure("time", size, name, images, parent if name == "parent" else ROOT))
                    print(size, name, kept[name][-1], flush=True)
            med = {k: statistics.median(v["ms"] for v in kept[k]) for k in configs}
            rng = {k: max(v["ms"] for v in kept[k]) - min(v["ms"] for v in kept[k]) for k in configs}
            rate = {k: statistics.median(v["burst_pairs_per_s"] for v in kept[k]) for k in configs}
            whole = _lib.pixel_iterations(W, H, LEVELS, 0)
            row = dict(W=W, H=H, children=kept, median_ms=med, range_ms=rng, burst_pairs_per_s=rate,
                       ms_over_plain={k: med[k] / med["plain"] for k in configs}, burst_over_plain={k: rate[k] / rate["plain"] for k in configs},
                       both_minus_plain_ms={f"both{e}": med[f"both{e}"] - med["plain"] for e in BOTH},
                       full_minus_none_ms={f"e{e}": med[f"cf{e}"] - med[f"c{e}"] for e in STOPS},
                       pixel_iterations_over_plain={f"e{e}": _lib.coarse_pixel_iterations(W, H, LEVELS, e) / whole for e in STOPS},
                       kernel=measure("kernel", size, "plain", images))
            if parent:
                row["plain_minus_parent_ms"] = med["plain"] - med["parent"]
            result["sizes"][size] = row
            print(json.dumps({k: v for k, v in row.items() if k != "children"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    {"time": time_child, "kernel": kernel_child, None: main}[args.child]()
