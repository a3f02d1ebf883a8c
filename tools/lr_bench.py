#!/usr/bin/env python3
"""What the LR check of the foveated calls costs (ugsm_set_lr_check, UGSM_LR_FOVEATED) -- on ONE box, in one session.

    python tools/lr_bench.py [--parent-tree DIR] [--rounds 3] [--out profiles/lr_fovea_bench.json]
    python tools/lr_bench.py --full [--parent-tree DIR] [--rounds 3]      # the full-mode calls: full_main below, profiles/lr_full_bench.json
    python tools/lr_bench.py --queue [--parent-tree DIR] [--rounds 3]     # checked full-mode pairs through the queue: queue_main below,
                                                                          # profiles/lr_queue_bench.json

At 16 MP (4928 x 3264) and 1080p, 14 / 7 levels, images resident on the device, events off, every measurement a child process of its own
(one context per process, as tools/ab.py), the configurations of a group taking turns round by round, every child's value kept:
  (a) one blocking plain foveated call: ugsm_submit_foveated + ugsm_wait on a one-slot context, the median wall-clock time of --reps calls
      after --warmup -- on this build, and on a build of the parent commit when --parent-tree names a tree that holds one
      (DIR/ug_stereomatcher_amd with its libugsm.so; the child then imports that package instead of this one);
  (b) the same call with the check on;
  (c) a queue burst of --burst foveated pairs on four slots with batches of eight, as bench.py --workload fovea16mp forms it
      (ugsm_enqueue_foveated, polling, drain), plain and checked, in pairs per second.
`spread` is the range (max - min) of the (a) children of this build; the acceptance of the change that added the check is written beside
the numbers: (a) on this build within the spread of (a) on the parent, and (b) below 2 x (a) by more than the spread -- two plain calls
are what running the second direction after the first would cost before the check itself.
"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libraries built")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--burst", type=int, default=96)
ap.add_argument("--tau", type=float, default=1.0)
ap.add_argument("--sizes", nargs="*", default=list(SIZES))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_fovea_bench.json"))
ap.add_argument("--out-partial", default=None, help="--queue: also write what has been measured so far to this file after every child")
ap.add_argument("--full", action="store_true", help="the full-mode table (full_main below) instead of the foveated one; writes profiles/lr_full_bench.json")
ap.add_argument("--queue", action="store_true", help="checked full-mode pairs through the queue (queue_main below); writes profiles/lr_queue_bench.json")
ap.add_argument("--arm", choices=["plain", "ctx", "checked", "checked_back", "managed", "managed_back"], default="plain", help="(internal, --child queue)")
ap.add_argument("--form", choices=["plain", "seq", "new"], default="plain", help="(internal, --child full)")
ap.add_argument("--n", type=int, default=1, help="(internal, --child full) pairs per call")
ap.add_argument("--child", choices=["call", "burst", "full", "queue"], help="(internal) measure in this process, print one JSON line")
ap.add_argument("--tree", default=ROOT, help="(internal) the tree whose package the child loads")
ap.add_argument("--checked", type=int, default=0, help="(internal)")
ap.add_argument("--size", default="16mp", help="(internal)")
args = ap.parse_args()


def child():
    sys.path.insert(0, args.tree)
    import numpy as np
    from ug_stereomatcher_amd import _lib, synth
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(args.tree), "ug_stereomatcher_amd")
    W, H = SIZES[args.size]
    fw, fh = _lib.fovea_dims(W, H, LEVELS, F)
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    nbytes = 3 * F * fh * fw * 4
    if args.child == "call":
        with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1) as c:
            if args.checked:
                c.set_lr_check(args.tau, _lib.UGSM_LR_FOVEATED)
            dL, dR, dS = c.to_device(L), c.to_device(R), c.alloc(nbytes)
            ts = []
            for k in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dL, dR, W, H, 3 * W, 0, 0, dS, None, None))
                c.check(c.lib.ugsm_wait(c.handle, 0))
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = ts[args.warmup:]
            marked = int(c.lib.ugsm_last_lr_marked(c.handle, 0))
            out = dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), marked=marked, device_bytes=c.device_bytes())
    else:
        slots, B = 4, 8
        with _lib.Context(levels=LEVELS, fovea_levels=F, slots=slots, batch=B) as c:
            if args.checked:
                c.set_lr_check(args.tau, _lib.UGSM_LR_FOVEATED)
            dL, dR = c.to_device(L), c.to_device(R)
            cap = (slots + 1) * B
            ring = [c.alloc(nbytes) for _ in range(cap)]

            def run(m):
                sizes, last = [], None
                for k in range(m):
                    c.enqueue_foveated(dL, dR, W, H, 3 * W, (0, 0), ring[k % cap], k)
                    while True:
                        d = c.next_done(False)
                        if d is None:
                            break
                        if d.call_index != last:
                            sizes.append(d.call_pairs)
                            last = d.call_index
                for d in c.drain():
                    if d.call_index != last:
                        sizes.append(d.call_pairs)
                        last = d.call_index
                return sizes
            run(2 * slots * B)
            t0 = time.perf_counter()
            sizes = run(args.burst)
            dt = time.perf_counter() - t0
            out = dict(pairs_per_s=args.burst / dt, calls=sizes, device_bytes=c.device_bytes())
    print("LRBENCH " + json.dumps(out), flush=True)


def full_child():
    """One blocking full-mode call of --n pairs (submit + ugsm_wait on a one-slot context; every pair the same two device images, its own outputs):
    plain -- ugsm_submit_full / ugsm_submit_full_batch; seq -- the same on a context with lr_check_threshold = tau (the second direction after
    the first, batches pair by pair); new -- ugsm_submit_full_checked, the right-to-left fields left in the slot as the context's check leaves them."""
    sys.path.insert(0, args.tree)
    from ug_stereomatcher_amd import _lib, synth
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(args.tree), "ug_stereomatcher_amd")
    W, H = SIZES[args.size]
    n = args.n
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    with _lib.Context(levels=LEVELS, slots=1, batch=n, lr_check_threshold=args.tau if args.form == "seq" else 0.0) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dO = [c.alloc(3 * W * H * 4) for _ in range(n)]
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            if args.form == "new":
                c.submit_full_checked(0, [dL] * n, [dR] * n, W, H, 3 * W, dO, None, args.tau)
            elif n == 1:
                c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, dO[0]))
            else:
                c.submit_full_batch(0, [dL] * n, [dR] * n, W, H, 3 * W, dO)
            c.check(c.lib.ugsm_wait(c.handle, 0))
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[args.warmup:]
        out = dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), marked=int(c.lib.ugsm_last_lr_marked(c.handle, 0)), device_bytes=c.device_bytes())
    print("LRBENCH " + json.dumps(out), flush=True)


def full_main():
    """--full: what the LR check of a full-mode call costs, at 16 MP and 1080p, 14 levels, every measurement a child process, the configurations
    taking turns round by round:
      a_plain    the plain blocking call, n = 1 (this build);
      b_seq      the checked ugsm_submit_full of the PARENT build (--parent-tree; this build's where none is given: the same code), n = 1: the
                 sequential form;  b_seq_this: the same on this build, where a parent was measured;
      c_new_1    ugsm_submit_full_checked, n = 1;  c_new_8: n = 8, against  b_seq_8: the parent's checked ugsm_submit_full_batch of 8.
    `b_spread_ms` is the range of the b_seq children; no ratio is fixed in advance (DESIGN.md section 8 quotes the table)."""
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit(f"{parent}: no built ug_stereomatcher_amd/libugsm.so")
    old = parent or ROOT
    result = dict(tool="tools/lr_bench.py --full", levels=LEVELS, tau=args.tau, rounds=args.rounds, reps=args.reps, parent_measured=bool(parent), sizes={})
    for size in args.sizes:
        configs = {"a_plain": (ROOT, "plain", 1), "b_seq": (old, "seq", 1), "c_new_1": (ROOT, "new", 1), "b_seq_8": (old, "seq", 8), "c_new_8": (ROOT, "new", 8)}
        if parent:
            configs["b_seq_this"] = (ROOT, "seq", 1)
        kept = {k: [] for k in configs}
        for rnd in range(args.rounds):
            names = list(configs)
            for name in (names if rnd % 2 == 0 else names[::-1]):     # alternating order
                tree, form, n = configs[name]
                kept[name].append(measure("full", size, tree, 0, form, n))
                print(size, name, kept[name][-1], flush=True)
        med = {k: statistics.median(v["ms"] for v in kept[k]) for k in configs}
        rng = {k: max(v["ms"] for v in kept[k]) - min(v["ms"] for v in kept[k]) for k in configs}
        row = dict(W=SIZES[size][0], H=SIZES[size][1], children=kept, median_ms=med, range_ms=rng, b_spread_ms=rng["b_seq"],
                   b_over_a=med["b_seq"] / med["a_plain"], c1_over_a=med["c_new_1"] / med["a_plain"], c1_over_b=med["c_new_1"] / med["b_seq"],
                   c8_over_b8=med["c_new_8"] / med["b_seq_8"], c8_ms_per_pair=med["c_new_8"] / 8, b8_ms_per_pair=med["b_seq_8"] / 8,
                   c1_slower_than_b_by_more_than_spread=bool(med["c_new_1"] - med["b_seq"] > rng["b_seq"]))
        result["sizes"][size] = row
        print(json.dumps({k: v for k, v in row.items() if k != "children"}), flush=True)
    out = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "lr_full_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(result, open(out, "w"), indent=1, sort_keys=True)
    print(f"wrote {out}")


def queue_child():
    """A queue burst of --burst full-mode pairs on four slots with batches of eight (every pair the same two images, a ring of (slots + 1) x batch
    outputs), completions polled after every enqueue and drained at the end, in pairs per second after a warm-up burst of 2 x slots x batch.  The arms:
    plain -- ugsm_enqueue_full; ctx -- the same on a context with ugsm_set_lr_check(tau, UGSM_LR_FULL): the context's own check, pair by pair;
    checked, checked_back -- ugsm_enqueue_full_checked without and with d_back; managed, managed_back -- ugsm_enqueue_full_checked_managed from
    pageable host images, without and with want_back."""
    sys.path.insert(0, args.tree)
    from ug_stereomatcher_amd import _lib, synth
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(args.tree), "ug_stereomatcher_amd")
    W, H = SIZES[args.size]
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    slots, B, arm = 4, 8, args.arm
    with _lib.Context(levels=LEVELS, slots=slots, batch=B) as c:
        if arm == "ctx":
            c.set_lr_check(args.tau, _lib.UGSM_LR_FULL)
        cap = (slots + 1) * B
        device = not arm.startswith("managed")
        dL, dR = (c.to_device(L), c.to_device(R)) if device else (None, None)
        ring = [c.alloc(3 * W * H * 4) for _ in range(cap)] if device else []
        back = [c.alloc(3 * W * H * 4) for _ in range(cap)] if arm == "checked_back" else [None] * cap

        def enqueue(k):
            if arm in ("plain", "ctx"):
                c.enqueue_full(dL, dR, W, H, 3 * W, ring[k % cap], k)
            elif device:
                c.enqueue_full_checked(dL, dR, W, H, 3 * W, ring[k % cap], back[k % cap], args.tau, k)
            else:
                c.enqueue_full_checked_managed(L, R, args.tau, arm == "managed_back", k)

        def run(m):
            sizes, last = [], None
            for k in range(m):
                enqueue(k)
                while True:
                    d = c.next_done(False)
                    if d is None:
                        break
                    if d.call_index != last:
                        sizes.append(d.call_pairs)
                        last = d.call_index
            for d in c.drain():
                if d.call_index != last:
                    sizes.append(d.call_pairs)
                    last = d.call_index
            return sizes
        run(2 * slots * B)
        t0 = time.perf_counter()
        sizes = run(args.burst)
        dt = time.perf_counter() - t0
        out = dict(pairs_per_s=args.burst / dt, calls=sizes, device_bytes=c.device_bytes())
    print("LRBENCH " + json.dumps(out), flush=True)


def queue_main():
    """--queue: what a checked full-mode pair costs through the queue, at 16 MP and 1080p, 14 levels, four slots, batch 8, a burst of --burst
    (128) pairs, every measurement a child process, the arms taking turns round by round:
      a         plain pairs;
      b         the parent commit's only way (--parent-tree; this build's where none is given): ugsm_enqueue_full on a context with
                ugsm_set_lr_check(tau, UGSM_LR_FULL);  b_this: the same on this build, where a parent was measured;
      c, c_back ugsm_enqueue_full_checked without / with d_back;
      d, d_back ugsm_enqueue_full_checked_managed from host memory, without / with want_back.
    Medians and ranges of pairs/s are kept; no ratio is fixed in advance (DESIGN.md section 8 quotes the table)."""
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit(f"{parent}: no built ug_stereomatcher_amd/libugsm.so")
    old = parent or ROOT
    burst = args.burst if args.burst != ap.get_default("burst") else 128
    result = dict(tool="tools/lr_bench.py --queue", levels=LEVELS, tau=args.tau, rounds=args.rounds, burst=burst, slots=4, batch=8,
                  parent_measured=bool(parent), sizes={})
    for size in args.sizes:
        arms = {"a": (ROOT, "plain"), "b": (old, "ctx"), "c": (ROOT, "checked"), "c_back": (ROOT, "checked_back"), "d": (ROOT, "managed"),
                "d_back": (ROOT, "managed_back")}
        if parent:
            arms["b_this"] = (ROOT, "ctx")
        kept = {k: [] for k in arms}
        for rnd in range(args.rounds):
            names = list(arms)
            for name in (names if rnd % 2 == 0 else names[::-1]):     # alternating order
                tree, arm = arms[name]
                kept[name].append(measure("queue", size, tree, 0, arm=arm, burst=burst))
                print(size, name, kept[name][-1], flush=True)
                if args.out_partial:                                  # (every child's value is on disk as soon as it exists)
                    json.dump(dict(result, sizes=dict(result["sizes"], **{size: dict(children=kept)})), open(args.out_partial, "w"), indent=1, sort_keys=True)
        med = {k: statistics.median(v["pairs_per_s"] for v in kept[k]) for k in arms}
        rng = {k: max(v["pairs_per_s"] for v in kept[k]) - min(v["pairs_per_s"] for v in kept[k]) for k in arms}
        row = dict(W=SIZES[size][0], H=SIZES[size][1], children=kept, median_pairs_per_s=med, range_pairs_per_s=rng, b_range_pairs_per_s=rng["b"],
                   c_over_b=med["c"] / med["b"], a_over_c=med["a"] / med["c"], a_over_b=med["a"] / med["b"], c_back_over_c=med["c_back"] / med["c"],
                   d_over_c=med["d"] / med["c"], c_beats_b_by_more_than_b_range=bool(med["c"] - med["b"] > rng["b"]))
        result["sizes"][size] = row
        print(json.dumps({k: v for k, v in row.items() if k != "children"}), flush=True)
    out = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "lr_queue_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(result, open(out, "w"), indent=1, sort_keys=True)
    print(f"wrote {out}")


def measure(kind, size, tree, checked, form="plain", n=1, arm="plain", burst=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--size", size, "--tree", tree, "--checked", str(int(checked)),
           "--reps", str(args.reps), "--warmup", str(args.warmup), "--burst", str(burst or args.burst), "--tau", str(args.tau), "--form", form, "--n", str(n),
           "--arm", arm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LRBENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][8:])


def main():
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit(f"{parent}: no built ug_stereomatcher_amd/libugsm.so")
    result = dict(tool="tools/lr_bench.py", levels=LEVELS, fovea_levels=F, tau=args.tau, rounds=args.rounds, reps=args.reps, burst=args.burst,
                  parent_measured=bool(parent), sizes={})
    for size in args.sizes:
        calls = {"a_this": (ROOT, 0), "b_checked": (ROOT, 1)}
        if parent:
            calls["a_parent"] = (parent, 0)
        bursts = {"c_plain": 0, "c_checked": 1}
        kept = {k: [] for k in list(calls) + list(bursts)}
        for rnd in range(args.rounds):
            names = list(calls)
            for name in (names if rnd % 2 == 0 else names[::-1]):     # alternating order
                tree, checked = calls[name]
                kept[name].append(measure("call", size, tree, checked))
                print(size, name, kept[name][-1], flush=True)
            names = list(bursts)
            for name in (names if rnd % 2 == 0 else names[::-1]):
                kept[name].append(measure("burst", size, ROOT, bursts[name]))
                print(size, name, kept[name][-1], flush=True)
        med = {k: statistics.median(v["ms"] for v in kept[k]) for k in calls}
        a_vals = [v["ms"] for v in kept["a_this"]]
        spread = max(a_vals) - min(a_vals)
        rate = {k: statistics.median(v["pairs_per_s"] for v in kept[k]) for k in bursts}
        row = dict(W=SIZES[size][0], H=SIZES[size][1], children=kept, a_ms=med["a_this"], b_ms=med["b_checked"], spread_ms=spread,
                   b_over_a=med["b_checked"] / med["a_this"], c_plain_pairs_per_s=rate["c_plain"], c_checked_pairs_per_s=rate["c_checked"],
                   c_plain_over_checked=rate["c_plain"] / rate["c_checked"],
                   b_below_two_a_by_more_than_spread=bool(2 * med["a_this"] - med["b_checked"] > spread))
        if parent:
            pv = [v["ms"] for v in kept["a_parent"]]
            row.update(a_parent_ms=med["a_parent"], a_parent_spread_ms=max(pv) - min(pv),
                       a_equals_parent_within_spread=bool(abs(med["a_this"] - med["a_parent"]) <= max(spread, max(pv) - min(pv))))
        result["sizes"][size] = row
        print(json.dumps({k: v for k, v in row.items() if k != "children"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    if args.child == "full":
        full_child()
    elif args.child == "queue":
        queue_child()
    elif args.child:
        child()
    elif args.queue:
        queue_main()
    else:
        full_main() if args.full else main()
