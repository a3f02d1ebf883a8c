#!/usr/bin/env python3
"""What the depth image costs (ugsm_depth_image, ugsm_match_full_depth), and what a host could do without it -- on ONE box, in one session.

    python tools/depth_bench.py --parent-tree DIR [--rounds 3] [--out profiles/depth_bench.json]

At 16 MP (4928 x 3264) and 1080p, 14 levels, events off.  Every measurement is a fresh child process (one context per process); the children
of the parent build (DIR: a checkout of the parent commit with its libraries built) and of this build alternate, and the rounds repeat them.

  a_parent / a_this   what a host can do on the parent commit: ugsm_triangulate on resident planes, the download of the Z plane, the 16UC1
                      conversion in numpy (the rule of include/ugsm.h).  a_this is the same on this build: the X, Y, Z instruction streams
                      did not move (tools/isa_dump.py --diff), so the two must agree within the spread.
  b                   ugsm_depth_image 16U on the same planes plus the download of the image.
  c_parent / c_this   ugsm_match_full from pageable memory: the blocking call, three planes down.
  d                   ugsm_match_full_depth 16U with no planes: only the image crosses the bus.
  kernel              the depth launches alone, a REGION as tools/warp_bench.py times it (`reps` calls of ugsm_depth_image through ctypes,
                      enqueued back to back, and one ugsm_wait): 16U without a confidence plane (8 + 2 bytes a pixel) and 32F with one
                      (12 + 4), each without d_valid and with it (`_count`: one hipMemsetAsync more per call, and the launch's one integer
                      atomic per wave on one word), beside the HBM bound W * H * bytes / peak.

    python tools/depth_bench.py --lens [--calibration tests/golden/lens_cal.json] [--rig rig16mp] [--rounds 3] [--out profiles/lens_bench.json]

What honouring the lens costs (ugsm_set_lens): the `kernel` regions alone, with the calibration's K, D and P, in children without a lens
(`kernel`) and with it (`kernel_lens`) that take turns round by round; the result goes under "depth" of --out, beside what
tools/cloud_bench.py --lens put there.

    python tools/depth_bench.py --frame --parent-tree DIR [--rounds 3] [--out profiles/depth_frame_bench.json]

The depth image of the whole frame from a fovea stack: (a) the composition ugsm_reconstruct_full[_multi] + ugsm_depth_image on a build of the
parent commit against (b) the fused call ugsm_depth_image_fovea_full / _multi on this build.  4928 x 3264 (14 levels, 7 fovea levels) and
1920 x 1080 (the same), 32F and 16U, factor 1 and 0.2, one window and four scattered windows; device-resident synthetic stacks, events off.
A child is one (size, windows, build): it times every form as a region (calls enqueued back to back, one ugsm_wait) and reports what
the context's slot memory grew by (ugsm_context_device_bytes).  The children of the two builds take turns, `rounds` children each.

Every child's value is kept; a row gives the median and the spread (max - min) of its children.  No number is fixed here: a ratio counts
as a difference only where it exceeds the spread between children of one configuration."""
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
CONFIGS = ["a_parent", "a_this", "b", "c_parent", "c_this", "d", "kernel"]
HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12   # bytes / s (tools/warp_bench.py)
UNIT = 0.01                                          # a unit that puts the synthetic pair's depths inside the 16UC1 range

ap = argparse.ArgumentParser()
ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libraries built")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--region", type=float, default=0.3, help="seconds a timed kernel region should last")
ap.add_argument("--sizes", nargs="*", default=list(SIZES))
ap.add_argument("--configs", nargs="*", default=None, help="the configurations to measure (default: all)")
ap.add_argument("--lens", action="store_true", help="the kernel regions without a lens and with it instead")
ap.add_argument("--frame", action="store_true", help="the whole frame's image from a fovea stack: the parent's composition against the fused call")
ap.add_argument("--windows", type=int, default=1, help="(internal) --frame: the windows of the child's stacks")
ap.add_argument("--calibration", default=os.path.join(ROOT, "tests", "golden", "lens_cal.json"), help="--lens: K, D, P of the two cameras")
ap.add_argument("--rig", default="rig16mp", help="--lens: the rig of the calibration file")
ap.add_argument("--iterations", type=int, default=5, help="--lens: ugsm_set_lens's iterations")
ap.add_argument("--out", default=None, help="default: profiles/depth_bench.json (--lens: profiles/lens_bench.json)")
ap.add_argument("--child", default=None, help="(internal) the configuration to measure in this process")
ap.add_argument("--size", default="16mp", help="(internal)")
ap.add_argument("--tree", default=ROOT, help="(internal)")
ap.add_argument("--images", default=None, help="(internal)")
args = ap.parse_args()


def rig():
    import numpy as np
    P1 = np.array([[7.3230899280915291e+03, 0., 2.4836974544986647e+03, 0.], [0., 7.3035803715514758e+03, 1.7170248033347561e+03, 0.],
                   [0., 0., 1., 0.]])
    P2 = P1.copy()
    P2[0, 3] = 7.3230899280915291e+03 * 0.12      # (the baseline on the side of the synthetic pairs' positive disparities)
    return P1, P2


def to_16u(np, z, unit):
    """The 16UC1 rule of include/ugsm.h on a host Z plane."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = (z * np.float32(unit)) * np.float32(1000.0) + np.float32(0.5)
        valid = np.isfinite(z) & (u >= np.float32(1.0)) & (u < np.float32(65536.0))
        return np.where(valid, u, np.float32(0)).astype(np.uint16)


FRAME_LEVELS, FRAME_FOVEA = 14, 7
FRAME_OFFSETS = {1: [(150, -90)], 4: [(-700, -400), (650, -350), (-600, 420), (720, 380)]}   # (level-0 pixels; clamped to the frame where they leave it)
FRAME_FORMS = [("32f", 0, 1.0), ("16u", 1, 1.0), ("32f_0.2", 0, 0.2), ("16u_0.2", 1, 0.2)]


def frame_child():
    """One (size, windows, build): `fused` on this build, `composed` on whichever tree args.tree names (only calls the parent has)."""
    sys.path.insert(0, args.tree)
    import ctypes as C
    import numpy as np
    from ug_stereomatcher_amd import _lib
    W, H = SIZES[args.size]
    n, nw, fused = W * H, args.windows, args.child == "fused"
    P1, P2 = rig()
    q = [(C.c_double * 12)(*np.asarray(p, np.float64).reshape(12)) for p in (P1, P2)]
    offs = FRAME_OFFSETS[nw]
    out = {}
    with _lib.Context(levels=FRAME_LEVELS, fovea_levels=FRAME_FOVEA, slots=1) as c:
        fw, fh = _lib.fovea_dims(W, H, FRAME_LEVELS, FRAME_FOVEA)
        plane = FRAME_FOVEA * fw * fh
        rng = np.random.Generator(np.random.PCG64(17))
        stacks = []
        for _ in range(nw):
            st = np.empty((3, FRAME_FOVEA, fh, fw), np.float32)
            for l in range(FRAME_FOVEA):
                k = np.float32(1.41421356) ** np.float32(l)
                st[0, l] = rng.normal(40, 12, (fh, fw)).astype(np.float32) / k
                st[1, l] = rng.normal(0, 2, (fh, fw)).astype(np.float32) / k
                st[2, l] = rng.uniform(0, 1, (fh, fw)).astype(np.float32) / k
            stacks.append(c.to_device(st))
        arr = (C.c_void_p * nw)(*stacks)
        ox, oy = (C.c_int * nw)(*[o[0] for o in offs]), (C.c_int * nw)(*[o[1] for o in offs])
        dF = None if fused else c.alloc(3 * n * 4)
        dD, dV = c.alloc(4 * n), c.alloc(8)
        bytes0 = c.device_bytes()

        def region(f, reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            c.check(c.lib.ugsm_wait(c.handle, 0))
            return time.perf_counter() - t0
        lib, h, s0 = c.lib, c.handle, stacks[0]
        for name, fmt, factor in FRAME_FORMS:
            prm = _lib.depth_params(format=fmt, unit=UNIT, min_conf=0.25, factor=factor)
            ref = C.byref(prm)
            if fused and nw == 1:
                f = lambda: c.check(lib.ugsm_depth_image_fovea_full(h, 0, s0, s0 + 4 * plane, s0 + 8 * plane, W, H, offs[0][0], offs[0][1], q[0], q[1], ref, dD, dV))   # noqa: E731
            elif fused:
                f = lambda: c.check(lib.ugsm_depth_image_fovea_multi(h, 0, nw, arr, W, H, ox, oy, q[0], q[1], ref, dD, dV))   # noqa: E731
            elif nw == 1:
                def f():
                    c.check(lib.ugsm_reconstruct_full(h, 0, s0, s0 + 4 * plane, s0 + 8 * plane, W, H, offs[0][0], offs[0][1], dF))
                    c.check(lib.ugsm_depth_image(h, 0, dF, dF + 4 * n, dF + 8 * n, W, H, q[0], q[1], ref, dD, dV))
            else:
                def f():
                    c.check(lib.ugsm_reconstruct_full_multi(h, 0, nw, arr, W, H, ox, oy, dF))
                    c.check(lib.ugsm_depth_image(h, 0, dF, dF + 4 * n, dF + 8 * n, W, H, q[0], q[1], ref, dD, dV))
            region(f, 5)
            reps = int(min(max(args.region / (region(f, 10) / 10), 10), 2000))
            region(f, reps)
            dt = region(f, reps)
            out[name] = dict(us_per_call=dt / reps * 1e6, reps=reps, valid=int(c.to_host(dV, (1,), np.uint64)[0]))
        # the slot's growth, and what the caller must hold besides the stacks and the image
        out["slot_bytes"] = c.device_bytes() - bytes0
        out["caller_field_bytes"] = 0 if fused else 3 * n * 4
    print("DEPTHBENCH " + json.dumps(out), flush=True)


def frame_main():
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if not parent or not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit("--frame needs --parent-tree DIR, a checkout of the parent commit with its libraries built")
    result = dict(tool="tools/depth_bench.py --frame", levels=FRAME_LEVELS, fovea_levels=FRAME_FOVEA, rounds=args.rounds, unit=UNIT, offsets=FRAME_OFFSETS,
                  timing="region / reps: calls enqueued back to back and one ugsm_wait; a: ugsm_reconstruct_full[_multi] + ugsm_depth_image on the parent "
                         "build, b: the fused call on this build; min_conf 0.25 and d_valid in every call", rows=[])
    for size in args.sizes:
        for nw in (1, 4):
            kept = {"composed": [], "fused": []}
            for rnd in range(args.rounds):
                for k in (("composed", "fused") if rnd % 2 == 0 else ("fused", "composed")):     # (the two builds' children take turns)
                    cmd = [sys.executable, os.path.abspath(__file__), "--frame", "--child", k, "--size", size, "--windows", str(nw), "--tree",
                           parent if k == "composed" else ROOT, "--region", str(args.region)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DEPTHBENCH ")]
                    if r.returncode != 0 or not lines:
                        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                    kept[k].append(json.loads(lines[-1][len("DEPTHBENCH "):]))
            for name, _, _ in FRAME_FORMS:
                a = [x[name]["us_per_call"] for x in kept["composed"]]
                b = [x[name]["us_per_call"] for x in kept["fused"]]
                ma, mb = statistics.median(a), statistics.median(b)
                spread = max(max(a) - min(a), max(b) - min(b))
                assert kept["composed"][0][name]["valid"] == kept["fused"][0][name]["valid"], (size, nw, name)
                row = dict(size=size, W=SIZES[size][0], H=SIZES[size][1], windows=nw, form=name, a_us=ma, a_us_children=a, b_us=mb, b_us_children=b,
                           b_over_a=mb / ma, spread_us=spread, spread_over_a=spread / ma, b_beats_a_by_more_than_the_spread=bool(ma - mb > spread),
                           valid=kept["fused"][0][name]["valid"],
                           a_slot_bytes=kept["composed"][0]["slot_bytes"], a_caller_field_bytes=kept["composed"][0]["caller_field_bytes"],
                           b_slot_bytes=kept["fused"][0]["slot_bytes"], b_caller_field_bytes=0)
                result["rows"].append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith("_children")}), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "depth_frame_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(result, open(out, "w"), indent=1, sort_keys=True)
    print(f"wrote {out}")


def child():
    sys.path.insert(0, args.tree)
    import ctypes as C
    import numpy as np
    from ug_stereomatcher_amd import _lib
    W, H = SIZES[args.size]
    n = W * H
    z = np.load(args.images)
    L, R, field = np.ascontiguousarray(z["L"]), np.ascontiguousarray(z["R"]), np.ascontiguousarray(z["field"])
    P1, P2 = rig()
    cal = None
    if args.lens:   # the calibration's projections; its right camera lies on the side of negative disparities
        cal = {k: np.array(v, np.float64) for k, v in json.load(open(args.calibration))[args.rig].items() if isinstance(v, list)}
        P1, P2 = cal["P1"].reshape(3, 4), cal["P2"].reshape(3, 4)
        field[0] = -field[0]
    case = args.child[0]
    out = {}

    def timed(f):
        ts = []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[args.warmup:]
        return dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts))

    with _lib.Context(levels=LEVELS, slots=1) as c:
        if args.child.endswith("_lens"):
            c.set_lens(cal["K1"], cal["D1"], cal["K2"], cal["D2"], args.iterations)
        if case == "a":
            dF, dX = c.to_device(field), c.alloc(3 * n * 4)

            def f():
                c.triangulate(dF, dF + 4 * n, W, H, P1, P2, dX)
                return to_16u(np, c.to_host(dX + 8 * n, (H, W)), UNIT)
            out = timed(f)
            out["valid_share"] = float((f() > 0).mean())
        elif case == "b":
            dF, dD, dV = c.to_device(field), c.alloc(2 * n), c.alloc(8)
            prm = _lib.depth_params(format=_lib.UGSM_DEPTH_16U, unit=UNIT)

            def f():
                c.depth_image(dF, dF + 4 * n, None, W, H, P1, P2, prm, dD, dV)
                return c.to_host(dD, (H, W), np.uint16)
            out = timed(f)
            out["valid_share"] = float((f() > 0).mean())
        elif case == "c":
            planes = np.empty((3, H, W), np.float32)
            ptr = [planes[k].ctypes.data for k in range(3)]
            out = timed(lambda: c.check(c.lib.ugsm_match_full(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], *ptr)))
        elif case == "d":
            prm = _lib.depth_params(format=_lib.UGSM_DEPTH_16U, unit=UNIT)
            depth = np.empty((H, W), np.uint16)
            q = [(C.c_double * 12)(*np.asarray(p, np.float64).reshape(12)) for p in (P1, P2)]
            out = timed(lambda: c.check(c.lib.ugsm_match_full_depth(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], q[0], q[1], C.byref(prm),
                                                                    depth.ctypes.data, None, None, None)))
            out["valid_share"] = float((depth > 0).mean())
        else:   # the kernel alone
            dF, dD, dV = c.to_device(field), c.alloc(4 * n), c.alloc(8)

            def region(f, reps):
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                c.check(c.lib.ugsm_wait(c.handle, 0))
                return time.perf_counter() - t0
            # (name: parameters, confidence plane, d_valid, bytes a pixel) -- `_count`: with d_valid, so the region also holds the count's
            # hipMemsetAsync per call and the launch its one integer atomic per wave on that one word
            u16, f32 = _lib.depth_params(format=_lib.UGSM_DEPTH_16U, unit=UNIT), _lib.depth_params(min_conf=0.5)
            forms = {"16u_no_conf": (u16, None, None, 8 + 2), "16u_no_conf_count": (u16, None, dV, 8 + 2),
                     "32f_conf": (f32, dF + 8 * n, None, 12 + 4), "32f_conf_count": (f32, dF + 8 * n, dV, 12 + 4)}
            q = [(C.c_double * 12)(*np.asarray(p, np.float64).reshape(12)) for p in (P1, P2)]
            for name, (prm, conf, valid, per_pixel) in forms.items():
                ref = C.byref(prm)     # the C call itself: no Python conversion inside the region
                f = lambda: c.check(c.lib.ugsm_depth_image(c.handle, 0, dF, dF + 4 * n, conf, W, H, q[0], q[1], ref, dD, valid))   # noqa: E731
                region(f, 10)
                reps = int(min(max(args.region / (region(f, 30) / 30), 30), 5000))
                region(f, reps)
                dt = region(f, reps)
                out[name] = dict(us_per_call=dt / reps * 1e6, reps=reps, bytes=n * per_pixel)
    print("DEPTHBENCH " + json.dumps(out), flush=True)


def measure(config, size, images, parent):
    tree = parent if config.endswith("_parent") else ROOT
    cmd = [sys.executable, os.path.abspath(__file__), "--child", config, "--size", size, "--tree", tree, "--images", images, "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--region", str(args.region)]
    if args.lens:
        cmd += ["--lens", "--calibration", args.calibration, "--rig", args.rig, "--iterations", str(args.iterations)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DEPTHBENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("DEPTHBENCH "):])


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    from ug_stereomatcher_amd import synth
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit(f"{parent}: no built ug_stereomatcher_amd/libugsm.so")
    configs = [k for k in (args.configs or CONFIGS) if parent or not k.endswith("_parent")]
    if args.lens:
        configs = ["kernel", "kernel_lens"]
        args.sizes = [s for s in args.sizes if s == "16mp"] or ["16mp"]
    result = dict(tool="tools/depth_bench.py", levels=LEVELS, rounds=args.rounds, reps=args.reps, parent_measured=bool(parent), unit=UNIT,
                  hbm_peak_spec_bytes_per_s=HBM_PEAK_SPEC, hbm_peak_measured_bytes_per_s=HBM_PEAK_MEASURED,
                  timing="a, b, c, d: host clock around one blocking step, the median of `reps` after `warmup`; kernel: region / reps", sizes={})
    with tempfile.TemporaryDirectory() as tmp:
        for size in args.sizes:
            W, H = SIZES[size]
            L, R, dx, dy = synth.make_pair(W, H, synth.BASE_SEED + 2)
            images = os.path.join(tmp, f"{size}.npz")
            np.savez(images, L=L, R=R, field=np.stack([dx, dy, np.full((H, W), 0.75, np.float32)]).astype(np.float32))
            kept = {k: [] for k in configs}
            for rnd in range(args.rounds):
                for k in (configs if rnd % 2 == 0 or not args.lens else configs[::-1]):       # (the parent's children and this build's alternate)
                    kept[k].append(measure(k, size, images, parent))
                print(size, rnd, {k: round(v[-1]["ms"], 3) for k, v in kept.items() if not k.startswith("kernel")}, flush=True)
            row = dict(W=W, H=H, configs={}, kernel={})
            med = {}
            for k in configs:
                if k.startswith("kernel"):
                    continue
                ms = [x["ms"] for x in kept[k]]
                med[k] = statistics.median(ms)
                row["configs"][k] = dict(ms=med[k], ms_children=ms, spread_ms=max(ms) - min(ms), children=kept[k])
            for cfg, name in [(cfg, name) for cfg in ("kernel", "kernel_lens") if cfg in kept for name in kept[cfg][0]]:
                us = [x[name]["us_per_call"] for x in kept[cfg]]
                m, nbytes = statistics.median(us), kept[cfg][0][name]["bytes"]
                row.setdefault(cfg, {})[name] = dict(us_per_call=m, us_per_call_children=us, spread_us=max(us) - min(us), bytes=nbytes,
                                           reps=[x[name]["reps"] for x in kept[cfg]],
                                           hbm_bound_us_spec=nbytes / HBM_PEAK_SPEC * 1e6, hbm_bound_us_measured=nbytes / HBM_PEAK_MEASURED * 1e6,
                                           bytes_per_s=nbytes / (m * 1e-6))
            a = "a_parent" if parent else "a_this"
            cc = "c_parent" if parent else "c_this"
            if "b" in med and a in med:
                row["b_over_a"] = med["b"] / med[a]
            if "d" in med and cc in med:
                row["d_over_c"] = med["d"] / med[cc]
                row["c_minus_d_ms"] = med[cc] - med["d"]
            if parent and all(k in med for k in ("a_this", "a_parent", "c_this", "c_parent")):
                row["a_this_minus_a_parent_ms"] = med["a_this"] - med["a_parent"]
                row["c_this_minus_c_parent_ms"] = med["c_this"] - med["c_parent"]
            result["sizes"][size] = row
            print(json.dumps({k: v for k, v in row.items() if k not in ("configs",)}), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "lens_bench.json" if args.lens else "depth_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if args.lens:   # beside the cloud tool's result
        result.update(tool="tools/depth_bench.py --lens", rig=args.rig, iterations=args.iterations)
        doc = json.load(open(out)) if os.path.exists(out) else {}
        doc["depth"] = result
        result = doc
    json.dump(result, open(out, "w"), indent=1, sort_keys=True)
    print(f"wrote {out}")


if __name__ == "__main__":
    if args.frame:
        frame_child() if args.child else frame_main()
    else:
        child() if args.child else main()
