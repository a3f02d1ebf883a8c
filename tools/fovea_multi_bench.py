#!/usr/bin/env python3
"""What n fovea windows on one pair cost (ugsm_submit_foveated_multi) against the three ways a host had before -- on ONE box, in one session.

    python tools/fovea_multi_bench.py [--parent-tree DIR] [--rounds 3] [--out profiles/fovea_multi_bench.json]

At 16 MP (4928 x 3264) and 1920 x 1080, 14 / 7 levels, images resident on the device, events off, n in {1, 2, 4, 8, 16} windows at scattered
offsets.  Every call is blocking and lone (submit + ugsm_wait on a one-slot context; the batch on a context created for n pairs); a value is
the median wall-clock time of --reps calls after --warmup.  The candidates:
  (a) n sequential ugsm_submit_foveated calls on one slot;
  (b) ugsm_submit_foveated_batch with the pair given n times (left out where its n x slot memory cannot be had);
  (c) ugsm_submit_pyramids + ugsm_submit_fovea_coarse + n x ugsm_submit_fovea_fine;
  (d) ugsm_submit_foveated_multi.
(a), (b) and (c) run on a build of the parent commit when --parent-tree names a tree that holds one (DIR/ug_stereomatcher_amd with its
libugsm.so; the child then imports that package instead of this one), else on this build.  A child is a fresh process that measures one tree
at one size -- every n, every candidate of that tree -- under a time limit of its own; the children of the two trees take turns round by
round, every child's value is kept, and the figure of a configuration is the median over its children.  `spread` is the range (max - min)
over the children of one configuration: what two runs of the same code differ by on the box.
Also timed at 16 MP: ugsm_reconstruct_full_multi for n = 1 against ugsm_reconstruct_full, and for n = 8.
Reported beside the numbers: (d) at n = 1 against one ugsm_submit_foveated on the parent (within the spread?), and (d) against the best of
(a), (b), (c) for every n >= 2 (faster by more than the spread?).

    python tools/fovea_multi_bench.py --checked [--parent-tree DIR] [--out profiles/fovea_multi_checked_bench.json]

The same protocol for the CHECKED multi-window call (ugsm_submit_foveated_multi_checked, tau = 1):
  (a)  n sequential checked ugsm_submit_foveated calls (ugsm_set_lr_check(1, UGSM_LR_FOVEATED));     on the parent
  (b)  a checked ugsm_submit_foveated_batch with the pair given n times;                             on the parent
  (c)  the plain ugsm_submit_foveated_multi;                                                         on the parent
  (d)  ugsm_submit_foveated_multi_checked;                                                           on this build
  (c') the plain ugsm_submit_foveated_multi.                                                         on this build
Reported: whether (d) takes no longer than the better of (a) and (b) beyond the spread (the larger range between the children of (d) and of
that candidate), whether (c') equals (c) within the spread of the two, the ratio (d) / (c'), and the memory of (d) against (b).
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
NS = (1, 2, 4, 8, 16)
# scattered window offsets as fractions of the frame (fixed: every run measures the same windows)
FRAC = [(0.0, 0.0), (-0.31, 0.22), (0.27, -0.18), (0.12, 0.30), (-0.22, -0.27), (0.33, 0.09), (-0.08, 0.15), (0.19, -0.33),
        (-0.35, -0.05), (0.05, -0.12), (0.24, 0.26), (-0.15, 0.34), (0.31, -0.29), (-0.27, 0.07), (0.09, 0.21), (-0.03, -0.35)]

ap = argparse.ArgumentParser()
ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libraries built")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--sizes", nargs="*", default=list(SIZES))
ap.add_argument("--child-timeout", type=int, default=240, help="seconds a child may take (timeout -k 10)")
ap.add_argument("--checked", action="store_true", help="measure the checked multi-window call (tau = 1) against its alternatives")
ap.add_argument("--out", default=None, help="default: profiles/fovea_multi_bench.json, with --checked profiles/fovea_multi_checked_bench.json")
ap.add_argument("--child", choices=["old", "new"], help="(internal) measure in this process, print one JSON line")
ap.add_argument("--tree", default=ROOT, help="(internal) the tree whose package the child loads")
ap.add_argument("--size", default="16mp", help="(internal)")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "fovea_multi_checked_bench.json" if args.checked else "fovea_multi_bench.json")
TAU = 1.0


def offsets(W, H, n):
    return [(int(fx * W), int(fy * H)) for fx, fy in FRAC[:n]]


def timed(fn):
    ts = []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[args.warmup:])


def child_checked():
    """The --checked child: (a), (b), (c) on the tree of `old`; (d), (c') on the tree of `new`."""
    sys.path.insert(0, args.tree)
    from ug_stereomatcher_amd import _lib, synth
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(args.tree), "ug_stereomatcher_amd")
    W, H = SIZES[args.size]
    fw, fh = _lib.fovea_dims(W, H, LEVELS, F)
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    nbytes = 3 * F * fh * fw * 4
    out = {}
    with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dS = [c.alloc(nbytes) for _ in range(max(NS))]
        wait = lambda: c.check(c.lib.ugsm_wait(c.handle, 0))
        for n in NS:
            offs = offsets(W, H, n)

            def plain():
                c.submit_foveated_multi(0, dL, dR, W, H, 3 * W, offs, dS[:n])
                wait()
            if args.child == "old":
                def a():
                    for k, (ox, oy) in enumerate(offs):
                        c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dL, dR, W, H, 3 * W, ox, oy, dS[k], None, None))
                        wait()
                out[f"c_{n}"] = timed(plain)
                c.set_lr_check(TAU, _lib.UGSM_LR_FOVEATED)
                out[f"a_{n}"] = timed(a)
                c.set_lr_check(0.0, 0)
            else:
                def d():
                    c.submit_foveated_multi_checked(0, dL, dR, W, H, 3 * W, offs, dS[:n], TAU)
                    wait()
                out[f"cp_{n}"] = timed(plain)
                out[f"d_{n}"] = timed(d)
                out[f"device_bytes_d_{n}"] = c.device_bytes()
    if args.child == "old":     # (b): a context created for n pairs holds n slots' worth of memory
        for n in NS:
            try:
                with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1, batch=n) as c:
                    c.set_lr_check(TAU, _lib.UGSM_LR_FOVEATED)
                    dL, dR = c.to_device(L), c.to_device(R)
                    dS = [c.alloc(nbytes) for _ in range(n)]
                    offs = offsets(W, H, n)

                    def b():
                        c.submit_foveated_batch(0, [dL] * n, [dR] * n, W, H, 3 * W, offs, dS)
                        c.check(c.lib.ugsm_wait(c.handle, 0))
                    out[f"b_{n}"] = timed(b)
                    out[f"device_bytes_b_{n}"] = c.device_bytes()
            except _lib.UgsmError as e:
                if e.status != _lib.UGSM_ERR_NOMEM:
                    raise
                out[f"b_{n}"] = None
    print("MULTIBENCH " + json.dumps(out), flush=True)


def child():
    if args.checked:
        return child_checked()
    sys.path.insert(0, args.tree)
    from ug_stereomatcher_amd import _lib, synth
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(args.tree), "ug_stereomatcher_amd")
    W, H = SIZES[args.size]
    fw, fh = _lib.fovea_dims(W, H, LEVELS, F)
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
    nbytes = 3 * F * fh * fw * 4
    out = {}
    with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dS = [c.alloc(nbytes) for _ in range(max(NS))]
        dT = c.alloc(3 * fh * fw * 4)
        wait = lambda: c.check(c.lib.ugsm_wait(c.handle, 0))
        if args.child == "old":
            for n in NS:
                offs = offsets(W, H, n)

                def a():
                    for k, (ox, oy) in enumerate(offs):
                        c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dL, dR, W, H, 3 * W, ox, oy, dS[k], None, None))
                        wait()

                def cc():
                    c.check(c.lib.ugsm_submit_pyramids(c.handle, 0, dL, dR, W, H, 3 * W))
                    c.check(c.lib.ugsm_submit_fovea_coarse(c.handle, 0, dT))
                    for k, (ox, oy) in enumerate(offs):
                        c.check(c.lib.ugsm_submit_fovea_fine(c.handle, 0, dT, ox, oy, dS[k]))
                    wait()
                out[f"a_{n}"] = timed(a)
                out[f"c_{n}"] = timed(cc)
            out["device_bytes_a_c"] = c.device_bytes()
        else:
            for n in NS:
                offs = offsets(W, H, n)

                def d():
                    c.submit_foveated_multi(0, dL, dR, W, H, 3 * W, offs, dS[:n])
                    wait()
                out[f"d_{n}"] = timed(d)
                out[f"device_bytes_d_{n}"] = c.device_bytes()
            if args.size == "16mp":     # the reconstruction over the stacks the last call left (n = 16): one window, old and new entry point; eight windows
                dO = c.alloc(3 * W * H * 4)
                pl = F * fh * fw * 4
                offs = offsets(W, H, 8)

                def r_old():
                    c.check(c.lib.ugsm_reconstruct_full(c.handle, 0, dS[0], dS[0] + pl, dS[0] + 2 * pl, W, H, 0, 0, dO))
                    wait()
                out["reconstruct_full"] = timed(r_old)
                out["reconstruct_multi_1"] = timed(lambda: c.reconstruct_full_multi(dS[:1], W, H, dO, offs[:1]))
                out["reconstruct_multi_8"] = timed(lambda: c.reconstruct_full_multi(dS[:8], W, H, dO, offs))
                c.free(dO)
    if args.child == "old":     # (b): a context created for n pairs holds n slots' worth of memory
        for n in NS:
            try:
                with _lib.Context(levels=LEVELS, fovea_levels=F, slots=1, batch=n) as c:
                    dL, dR = c.to_device(L), c.to_device(R)
                    dS = [c.alloc(nbytes) for _ in range(n)]
                    offs = offsets(W, H, n)

                    def b():
                        c.submit_foveated_batch(0, [dL] * n, [dR] * n, W, H, 3 * W, offs, dS)
                        c.check(c.lib.ugsm_wait(c.handle, 0))
                    out[f"b_{n}"] = timed(b)
                    out[f"device_bytes_b_{n}"] = c.device_bytes()
            except _lib.UgsmError as e:
                if e.status != _lib.UGSM_ERR_NOMEM:
                    raise
                out[f"b_{n}"] = None
    print("MULTIBENCH " + json.dumps(out), flush=True)


def measure(kind, size, tree):
    cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", kind, "--size", size, "--tree", tree,
           "--reps", str(args.reps), "--warmup", str(args.warmup)] + (["--checked"] if args.checked else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("MULTIBENCH ")]
    if r.returncode != 0 or not lines:     # (a child that failed, faulted or ran into its limit: nothing more is started)
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("MULTIBENCH "):])


def main():
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit(f"{parent}: no built ug_stereomatcher_amd/libugsm.so")
    result = dict(tool="tools/fovea_multi_bench.py" + (" --checked" if args.checked else ""), levels=LEVELS, fovea_levels=F, rounds=args.rounds,
                  reps=args.reps, warmup=args.warmup, parent_measured=bool(parent), windows=NS, sizes={})
    if args.checked:
        result["tau"] = TAU
    for size in args.sizes:
        W, H = SIZES[size]
        turns = [("old", parent or ROOT), ("new", ROOT)]
        kept = {"old": [], "new": []}
        for rnd in range(args.rounds):
            for kind, tree in (turns if rnd % 2 == 0 else turns[::-1]):     # alternating order
                kept[kind].append(measure(kind, size, tree))
                print(size, kind, kept[kind][-1], flush=True)

        def stat(kind, key):
            vals = [v[key] for v in kept[kind] if v.get(key) is not None]
            return (statistics.median(vals), max(vals) - min(vals)) if vals else (None, None)
        row = dict(W=W, H=H, offsets=offsets(W, H, max(NS)), children=kept, n={})
        if args.checked:
            for n in NS:
                cell = {}
                for kind, cand in (("old", "a"), ("old", "b"), ("old", "c"), ("new", "d"), ("new", "cp")):
                    cell[f"{cand}_ms"], cell[f"{cand}_spread_ms"] = stat(kind, f"{cand}_{n}")
                others = {k: cell[f"{k}_ms"] for k in "ab" if cell[f"{k}_ms"] is not None}
                best = min(others, key=others.get)
                spread = max(cell["d_spread_ms"], cell[f"{best}_spread_ms"])
                cell.update(best_other=best, best_other_ms=others[best], d_over_best=cell["d_ms"] / others[best], spread_ms=spread,
                            d_over_cp=cell["d_ms"] / cell["cp_ms"],
                            d_no_slower_than_best_beyond_spread=bool(cell["d_ms"] - others[best] <= spread),
                            d_faster_than_best_by_more_than_spread=bool(others[best] - cell["d_ms"] > spread),
                            cp_equals_c_within_spread=bool(abs(cell["cp_ms"] - cell["c_ms"]) <= max(cell["cp_spread_ms"], cell["c_spread_ms"])),
                            device_bytes_d=stat("new", f"device_bytes_d_{n}")[0], device_bytes_b=stat("old", f"device_bytes_b_{n}")[0])
                row["n"][str(n)] = cell
            result["sizes"][size] = row
            print(json.dumps({k: v for k, v in row.items() if k != "children"}), flush=True)
            continue
        single, single_spread = stat("old", "a_1")
        for n in NS:
            cell = {}
            for kind, cand in (("old", "a"), ("old", "b"), ("old", "c"), ("new", "d")):
                cell[f"{cand}_ms"], cell[f"{cand}_spread_ms"] = stat(kind, f"{cand}_{n}")
            others = {k: cell[f"{k}_ms"] for k in "abc" if cell[f"{k}_ms"] is not None}
            best = min(others, key=others.get)
            spread = max(cell["d_spread_ms"], cell[f"{best}_spread_ms"])
            cell.update(best_other=best, best_other_ms=others[best], d_over_best=cell["d_ms"] / others[best], spread_ms=spread)
            if n == 1:
                cell["d_equals_single_call_within_spread"] = bool(abs(cell["d_ms"] - single) <= max(cell["d_spread_ms"], single_spread))
            else:
                cell["d_faster_than_best_by_more_than_spread"] = bool(others[best] - cell["d_ms"] > spread)
            row["n"][str(n)] = cell
        for key in ("reconstruct_full", "reconstruct_multi_1", "reconstruct_multi_8"):
            if any(key in v for v in kept["new"]):
                row[key + "_ms"], row[key + "_spread_ms"] = stat("new", key)
        result["sizes"][size] = row
        print(json.dumps({k: v for k, v in row.items() if k != "children"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    child() if args.child else main()
