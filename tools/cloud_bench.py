#!/usr/bin/env python3
"""The coloured point cloud on the device (ugsm_point_cloud) -- time, bytes, rate, and the host copy it replaces.

    python tools/cloud_bench.py [--reps 25] [--warmup 5] [--out FILE.json]

For 16 MP (4928 x 3264) and 1080p, each cloud form (dense PCL32, dense 16-byte, compact PCL32 / 16-byte with min_conf 0.5) at sampling
1 and 2, from the (dx, dy, conf) of a real match of the synthetic pair:
  - device_ms: the call's device time, median over --reps calls after --warmup, from the library's own in-dispatch events
    (ugsm_config.profile_events 2: from the first launch's begin to the last launch's end; a compact cloud is two launches);
  - MB: bytes the call must move, from the shapes and the count -- dx, dy (+ conf when compacting; the count launch reads dx, dy, conf
    once more) and 3 B of rgb per sampled point read, count x point_step written;
  - GBps, of_copy: MB / device_ms, and that over the device-to-device copy rate measured here the way bench.py records device_copy_GBps
    (a streaming elementwise kernel, 1 GiB read + 1 GiB written per pass); floor_ms = MB at that rate, of_floor = floor_ms / device_ms;
  - d2h_ms: the device-to-host copy of the cloud (count x point_step) into page-locked memory, median of wall-clock copies.
Today's path, per size: ugsm_triangulate (device_ms as above) and the copy of its three float planes to page-locked memory.
Prints one JSON line per row and writes them all to --out.

    python tools/cloud_bench.py --resized [--out profiles/cloud_resized_bench.json]

The resized cloud (ugsm_point_cloud_resized[_fovea]) instead: per size, today's path as above, then dense PCL32 and compact PCL32
(min_conf 0.5) at f = 0.2 and 0.5, and at 16 MP the fovea stack's level 0 at f = 0.2 (dense PCL32, the reference's colour).  MB: dx, dy
read once (8 B per pixel of the planes: every row is touched, by a tap or by yy; the compact form's count launch reads them again, and
conf once per point), the rgb rows the points read (dh rows of 3 W bytes), count x 32 written.

    python tools/cloud_bench.py --stack [--out profiles/cloud_stack_bench.json]

The merged cloud of the whole fovea stack (ugsm_point_cloud_fovea_all) instead: per size, after one ugsm_submit_foveated on the slot,
dense PCL32, dense 16-byte and compact PCL32 (min_conf 0.5) as one call, and in the same run the two paths it replaces: the F per-level
ugsm_point_cloud_fovea calls (each repeat is the F calls together; the covered points are written F times over) and
ugsm_reconstruct_full followed by the dense ugsm_point_cloud of the W x H field.  device_ms is the median over --reps repeats of the
summed in-dispatch kernel times of a repeat, device_ms_min / _max their range; wall_ms the median host time from the first call to the
end of ugsm_wait (launch gaps and the compact forms' memsets included); MB = count x point_step, the bytes a consumer receives; d2h_ms
their copy to page-locked memory.

    python tools/cloud_bench.py --queue [--pairs 64] [--out profiles/queue_cloud_bench.json]

The cloud from the queue (ugsm_enqueue_*_cloud_managed, ugsm_done_cloud) instead: 16 MP, four slots, calls of up to eight pairs, managed
kind (any host memory in, library-owned results out), --pairs pairs after a warm-up burst, full mode and the foveated stack.  Legs, pairs/s
(median of five bursts after two warm-up bursts; every burst's figure is kept): planes only (ugsm_enqueue_*_managed), cloud only (XYZRGB16, sampling 2, dense),
cloud only (XYZRGB16, sampling 1, compact: min_conf = the median confidence of the first pair), cloud plus planes (the dense cloud with
want_planes).  Then the device time (profile_events 2: the in-dispatch events of the launches) of ONE batched cloud launch for a call of
eight pairs against eight single-pair ugsm_point_cloud / ugsm_point_cloud_fovea_all launches on planes of the same size, for the 16 MP
stack and for 1080p full mode, dense and compact PCL32.  --leg NAME runs one leg only (each GPU step under a time limit of its own).

    python tools/cloud_bench.py --multi [--parent-tree DIR] [--rounds 3] [--out profiles/cloud_multi_bench.json]

The merged cloud of several windows of one pair (ugsm_point_cloud_fovea_multi) instead: 16 MP and 1080p at 14 / 7 levels, n = 2, 4, 8
windows at two offset sets -- spread over the frame (little overlap) and clustered round the centre (heavy overlap) -- after one
ugsm_submit_foveated_multi on the slot.  Per case: one merged call, dense PCL32 and compact XYZRGB16 (min_conf 0.5), and the n
ugsm_point_cloud_fovea_all calls it replaces (each repeat is the n calls together, cloud behind cloud in one buffer): device_ms (the summed
in-dispatch kernel times of a repeat, median over --reps repeats after --warmup), wall_ms (first call .. end of ugsm_wait: launch gaps,
the table's upload and the compact forms' memsets included) and the records written.  Every measurement runs in a child process of its
own (one context per process), as tools/lr_bench.py does it: this build's child and -- when --parent-tree names a checkout of the parent
commit with its libraries built -- the parent's child, which times the n calls there, take turns round by round in alternating order;
every child's value is kept, `spread` is the range between a configuration's own children.  Written beside the numbers: whether the
merged call takes no longer than the n calls on the parent commit, beyond the spread between those calls' own repeats.

    python tools/cloud_bench.py --lens [--calibration tests/golden/lens_cal.json] [--rig rig16mp] [--rounds 3] [--out profiles/lens_bench.json]

What honouring the lens costs (ugsm_set_lens): at 16 MP with the calibration's K, D and P, from a synthetic field and a random confidence,
the dense PCL32 cloud, the compact PCL32 cloud (min_conf 0.5) and the dense resized cloud at f = 0.2, each without a lens and with it.
Every measurement is a child process of its own; the children without and with the lens take turns round by round in alternating order;
every child's value is kept (device_ms: the median of --reps repeats of the call's in-dispatch kernel time after --warmup).  The result
goes under "cloud" of --out, beside what tools/depth_bench.py --lens put there.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)   # (a --multi child puts its --tree in front of it)

P1 = np.array([[7.3230899280915291e+03, 0., 2.4836974544986647e+03, 0.],
               [0., 7.3035803715514758e+03, 1.7170248033347561e+03, 0.], [0., 0., 1., 0.]])
P2 = P1.copy()
P2[0, 3] = -7.3230899280915291e+03 * 0.12


def device_ms(c, call):
    """One call's device time from the library's events (profile_events 2): reset, call, wait, sum what was harvested."""
    lib = c.lib
    c.check(lib.ugsm_reset_kernel_stats(c.handle))
    call()
    c.check(lib.ugsm_wait(c.handle, 0))
    from ug_stereomatcher_amd import _lib
    st = (_lib.KernelStat * 64)()
    n = lib.ugsm_get_kernel_stats(c.handle, st, 64)
    return sum(st[k].total_ms for k in range(min(n, 64)))


def median_ms(c, call, reps, warmup):
    for _ in range(warmup):
        device_ms(c, call)
    return float(np.median([device_ms(c, call) for _ in range(reps)]))


def spread_ms(c, call, reps, warmup):
    """-> (median, min, max) of the device time of `reps` repeats, and the median wall-clock time of a repeat (call .. end of ugsm_wait)."""
    for _ in range(warmup):
        device_ms(c, call)
    ts = [device_ms(c, call) for _ in range(reps)]
    ws = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        c.check(c.lib.ugsm_wait(c.handle, 0))
        ws.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), float(np.median(ws))


def host_copy_ms(c, dst, src, nbytes, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c.check(c.lib.ugsm_copy_to_host(c.handle, dst, src, nbytes))
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def copy_rate_GBps(torch):
    a = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        torch.add(a, 1.0, out=b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(8):
        torch.add(a, 1.0, out=b)
    e1.record()
    torch.cuda.synchronize()
    r = 8 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
    del a, b
    torch.cuda.empty_cache()
    return r


def resized_rows(args, emit, copy, p1, p2, dp):
    from ug_stereomatcher_amd import _lib, synth
    P1p, P2p = p1.ctypes.data_as(dp), p2.ctypes.data_as(dp)

    def row(c, name, call, pw, ph, W, f, npts, compact, d_pts, d_cnt, h_addr, **extra):
        t = median_ms(c, call, args.reps, args.warmup)
        count = int(c.to_host(d_cnt, (1,), np.int64)[0])
        dh = int(np.float32(ph) * np.float32(f))
        read = 8 * pw * ph + dh * 3 * W + ((8 * pw * ph + 4 * npts) + 4 * npts if compact else 0)
        mb = (read + count * 32) / 1e6
        floor = mb / 1e3 / copy * 1e3
        t_d2h = host_copy_ms(c, h_addr, d_pts, count * 32, max(5, args.reps // 3)) if count else 0.0
        emit(dict({"what": name, "factor": f, "points": npts, "count": count, "device_ms": round(t, 4), "MB": round(mb, 1),
                   "GBps": round(mb / t, 1), "floor_ms": round(floor, 4), "of_floor": round(floor / t, 3), "d2h_MB": round(count * 32 / 1e6, 2),
                   "d2h_ms": round(t_d2h, 3), "total_ms": round(t + t_d2h, 3)}, **extra))

    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 2)
        with _lib.Context(levels=14, profile_events=2) as c:
            pL, pR = c.to_device(L), c.to_device(R)
            plane = W * H * 4
            d_out, d_xyz = c.alloc(3 * plane), c.alloc(3 * plane)
            c.check(c.lib.ugsm_submit_full(c.handle, 0, pL, pR, W, H, L.strides[0], d_out))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            d_dx, d_dy, d_conf = d_out, d_out + plane, d_out + 2 * plane
            cap = _lib.resized_cloud_points(W, H, 0.5)
            d_pts, d_cnt = c.alloc(cap * 32), c.alloc(8)
            host = c.host_array((3 * plane,), np.uint8)
            h_addr = host.ctypes.data
            # today's path: the X, Y, Z planes, then the three planes to the host (where the resize would run)
            tri = lambda: c.check(c.lib.ugsm_triangulate(c.handle, 0, d_dx, d_dy, W, H, P1p, P2p, d_xyz))
            t_tri = median_ms(c, tri, args.reps, args.warmup)
            t_planes = host_copy_ms(c, h_addr, d_xyz, 3 * plane, max(5, args.reps // 3))
            mb = (8 + 12) * W * H / 1e6
            emit({"what": "planes_today", "size": size, "device_ms": round(t_tri, 4), "MB": round(mb, 1), "GBps": round(mb / t_tri, 1),
                  "d2h_MB": round(3 * plane / 1e6, 1), "d2h_ms": round(t_planes, 3), "total_ms": round(t_tri + t_planes, 3)})
            for f in (0.2, 0.5):
                npts = _lib.resized_cloud_points(W, H, f)
                for name, compact in (("resized_dense_pcl32", False), ("resized_compact_pcl32", True)):
                    prm = _lib.cloud_params(compact=compact, min_conf=0.5 if compact else None)
                    call = lambda: c.check(c.lib.ugsm_point_cloud_resized(c.handle, 0, d_dx, d_dy, d_conf, pL, W, H, L.strides[0], P1p, P2p,
                                                                          C.c_float(f), C.byref(prm), d_pts, npts, d_cnt))
                    row(c, name, call, W, H, W, f, npts, compact, d_pts, d_cnt, h_addr, size=size)
            if (W, H) == (4928, 3264):   # the fovea stack's level 0 (ugsm_fovea_mapping's margins)
                fw, fh = _lib.fovea_dims(W, H, 14, 7)
                d_stack = c.alloc(3 * 7 * fw * fh * 4)
                c.check(c.lib.ugsm_submit_foveated(c.handle, 0, pL, pR, W, H, L.strides[0], 0, 0, d_stack, None, None))
                c.check(c.lib.ugsm_wait(c.handle, 0))
                lvl = 7 * fw * fh * 4
                left, upper, scale = _lib.fovea_mapping(W, H, 0)
                npts = _lib.resized_cloud_points(fw, fh, 0.2)
                prm = _lib.cloud_params()
                call = lambda: c.check(c.lib.ugsm_point_cloud_resized_fovea(c.handle, 0, d_stack, d_stack + lvl, d_stack + 2 * lvl, fw, fh, 0,
                                                                            left, upper, C.c_float(scale), pL, W, H, L.strides[0], P1p, P2p,
                                                                            C.c_float(0.2), 0, C.byref(prm), d_pts, npts, d_cnt))
                row(c, "resized_fovea_dense_pcl32", call, fw, fh, fw, 0.2, npts, False, d_pts, d_cnt, h_addr, size=f"{fw}x{fh} level 0")
                c.free(d_stack)
            for p in (pL, pR, d_out, d_xyz, d_pts, d_cnt):
                c.free(p)


def stack_rows(args, emit, p1, p2, dp):
    from ug_stereomatcher_amd import _lib, synth
    P1p, P2p = p1.ctypes.data_as(dp), p2.ctypes.data_as(dp)
    levels, F = 14, 7
    forms = (("dense_pcl32", 0, False), ("dense_xyzrgb16", 1, False), ("compact_pcl32", 0, True))
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 2)
        fw, fh = _lib.fovea_dims(W, H, levels, F)
        with _lib.Context(levels=levels, fovea_levels=F, profile_events=2) as c:
            lib, h = c.lib, c.handle
            pL, pR = c.to_device(L), c.to_device(R)
            lvl = F * fw * fh * 4
            d_stack = c.alloc(3 * lvl)
            c.check(lib.ugsm_submit_foveated(h, 0, pL, pR, W, H, L.strides[0], 0, 0, d_stack, None, None))
            c.check(lib.ugsm_wait(h, 0))
            sx, sy, sc = d_stack, d_stack + lvl, d_stack + 2 * lvl
            plane = W * H * 4
            d_full = c.alloc(3 * plane)
            d_pts, d_cnt, d_lvl = c.alloc(W * H * 32), c.alloc(8 * F), c.alloc(8 * F)
            host = c.host_array((W * H * 32,), np.uint8)
            maps = [_lib.fovea_level_mapping(W, H, levels, F, k) for k in range(F)]
            copies = max(5, args.reps // 3)

            def row(what, call, count, step, **extra):
                t, lo, hi, wall = spread_ms(c, call, args.reps, args.warmup)
                n = count()
                t_d2h = host_copy_ms(c, host.ctypes.data, d_pts, n * step, copies) if n else 0.0
                emit(dict({"what": what, "size": size, "count": n, "device_ms": round(t, 4), "device_ms_min": round(lo, 4),
                           "device_ms_max": round(hi, 4), "wall_ms": round(wall, 4), "MB": round(n * step / 1e6, 2), "d2h_ms": round(t_d2h, 3),
                           "total_ms": round(t + t_d2h, 3)}, **extra))

            for name, fmt, compact in forms:
                prm = _lib.cloud_params(format=fmt, compact=compact, min_conf=0.5 if compact else None)
                step = 32 if fmt == 0 else 16
                merged = lambda: c.check(lib.ugsm_point_cloud_fovea_all(h, 0, sx, sy, sc, W, H, 0, 0, pL, L.strides[0], P1p, P2p, C.byref(prm),
                                                                        d_pts, W * H, d_cnt, d_lvl))
                row("stack_" + name, merged, lambda: int(c.to_host(d_cnt, (1,), np.int64)[0]), step, launches=2 if compact else 1)
                # the F per-level calls, each level's cloud behind the one before (a compact cloud needs each count back first: not timed)
                counts = []
                for k in range(F):
                    c.check(lib.ugsm_point_cloud_fovea(h, 0, sx, sy, sc, fw, fh, k, maps[k][0], maps[k][1], C.c_float(maps[k][2]), pL, W, H,
                                                       L.strides[0], P1p, P2p, C.byref(prm), d_pts, fw * fh, d_cnt + 8 * k))
                c.check(lib.ugsm_wait(h, 0))
                counts = c.to_host(d_cnt, (F,), np.int64).tolist()
                first = np.concatenate([[0], np.cumsum(counts)]).tolist()

                def per_level():
                    for k in range(F):
                        c.check(lib.ugsm_point_cloud_fovea(h, 0, sx, sy, sc, fw, fh, k, maps[k][0], maps[k][1], C.c_float(maps[k][2]), pL, W, H,
                                                           L.strides[0], P1p, P2p, C.byref(prm), d_pts + first[k] * step, fw * fh, d_cnt + 8 * k))
                row("per_level_" + name, per_level, lambda: int(sum(counts)), step, launches=F * (2 if compact else 1))
            # the dense field: hierarchicalDisparity's upsampled planes, then the cloud of every pixel
            prm = _lib.cloud_params()

            def dense_path():
                c.check(lib.ugsm_reconstruct_full(h, 0, sx, sy, sc, W, H, 0, 0, d_full))
                c.check(lib.ugsm_point_cloud(h, 0, d_full, d_full + plane, d_full + 2 * plane, pL, W, H, L.strides[0], P1p, P2p, C.byref(prm),
                                             d_pts, W * H, d_cnt))
            row("reconstruct_full_then_dense_pcl32", dense_path, lambda: int(c.to_host(d_cnt, (1,), np.int64)[0]), 32, launches=F,
                planes_MB=round(3 * plane / 1e6, 1))
            for p in (pL, pR, d_stack, d_full, d_pts, d_cnt, d_lvl):
                c.free(p)


QUEUE_LEGS = ("planes", "cloud_dense_s2", "cloud_compact_s1", "cloud_dense_s2_planes")


def queue_rows(args, emit, p1, p2):
    from ug_stereomatcher_amd import _lib, synth
    W, H, levels, F = 4928, 3264, 14, 7
    pairs = [synth.make_pair(W, H, synth.BASE_SEED + 2 + 16 * k)[:2] for k in range(2)]
    xyz16 = _lib.UGSM_CLOUD_XYZRGB16
    legs = [l for l in QUEUE_LEGS if args.leg in (None, l)]
    for fovea in (False, True):
        if args.mode not in (None, "foveated" if fovea else "full"):
            continue
        # the compact leg's threshold: the median confidence of the first pair (slot-level match)
        with _lib.Context(levels=levels, fovea_levels=F) as c:
            L, R = pairs[0]
            pL, pR = c.to_device(L), c.to_device(R)
            fw, fh = _lib.fovea_dims(W, H, levels, F) if fovea else (W, H)
            plane = (F if fovea else 1) * fw * fh
            d_out = c.alloc(3 * plane * 4)
            if fovea:
                c.check(c.lib.ugsm_submit_foveated(c.handle, 0, pL, pR, W, H, L.strides[0], 0, 0, d_out, None, None))
            else:
                c.check(c.lib.ugsm_submit_full(c.handle, 0, pL, pR, W, H, L.strides[0], d_out))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            med = float(np.median(c.to_host(d_out + 2 * plane * 4, (plane,), np.float32)))
        specs = {"cloud_dense_s2": _lib.queue_cloud(p1, p2, _lib.cloud_params(sampling=2, format=xyz16)),
                 "cloud_compact_s1": _lib.queue_cloud(p1, p2, _lib.cloud_params(format=xyz16, compact=True, min_conf=med)),
                 "cloud_dense_s2_planes": _lib.queue_cloud(p1, p2, _lib.cloud_params(sampling=2, format=xyz16), want_planes=True)}
        for leg in legs:
            with _lib.Context(levels=levels, fovea_levels=F, slots=4, batch=8) as c:
                spec = specs.get(leg)

                def burst(n):
                    out, sent, t0 = 0, 0, time.perf_counter()
                    cloud_mb = 0.0
                    while out < n:
                        while sent < n and sent - out < 32:
                            L, R = pairs[sent % len(pairs)]
                            if spec is None:
                                (c.enqueue_foveated_managed(L, R, (0, 0), False, sent) if fovea else c.enqueue_full_managed(L, R, sent))
                            else:
                                (c.enqueue_foveated_cloud_managed(L, R, (0, 0), spec, sent) if fovea else c.enqueue_full_cloud_managed(L, R, spec, sent))
                            sent += 1
                        d = c.next_done(sent == n or sent - out >= 32)
                        while d is not None:
                            if spec is not None:
                                rec, cnt, _ = c.done_cloud()
                                cloud_mb = rec.nbytes / 1e6
                            out += 1
                            d = c.next_done(False) if out < n else None
                    return n / (time.perf_counter() - t0), cloud_mb

                for _ in range(2):   # warm-up: every slot's buffers, the managed staging at its final size
                    burst(args.pairs)
                rates = [burst(args.pairs) for _ in range(5)]
                emit({"what": "queue_" + leg, "mode": "foveated" if fovea else "full", "size": f"{W}x{H}", "pairs": args.pairs, "slots": 4, "batch": 8,
                      "pairs_per_s": round(float(np.median([r[0] for r in rates])), 2), "bursts_pairs_per_s": [round(r[0], 2) for r in rates],
                      "cloud_MB_per_pair": round(rates[-1][1], 2), "min_conf": round(med, 4) if leg == "cloud_compact_s1" else None,
                      "device_bytes": int(c.lib.ugsm_context_device_bytes(c.handle))})


def queue_launch_rows(args, emit, p1, p2, dp):
    """One batched cloud launch for eight pairs against eight single-pair launches, device time from the in-dispatch events."""
    from ug_stereomatcher_amd import _lib, synth
    P1p, P2p = p1.ctypes.data_as(dp), p2.ctypes.data_as(dp)
    n = 8

    def misc_ms(c):   # (the cloud launches are the only ones of a context without the LR check that the statistics file under "misc")
        return sum(r["total_ms"] for r in c.kernel_stats() if r["name"] == "misc")

    for fovea, W, H in ((True, 4928, 3264), (False, 1920, 1080)):
        levels, F = 14, 7
        L, R = synth.make_pair(W, H, synth.BASE_SEED + 2)[:2]
        fw, fh = _lib.fovea_dims(W, H, levels, F) if fovea else (W, H)
        plane = (F if fovea else 1) * fw * fh
        for name, compact in (("dense_pcl32", False), ("compact_pcl32", True)):
            prm = _lib.cloud_params(compact=compact, min_conf=0.5 if compact else None)
            cap = _lib.fovea_cloud_points(W, H, levels, F) if fovea else _lib.cloud_points(W, H, 1)
            with _lib.Context(levels=levels, fovea_levels=F, slots=1, batch=n, profile_events=2) as c:
                pL, pR = c.to_device(L), c.to_device(R)
                outs = [c.alloc(3 * plane * 4) for _ in range(n)]
                pts = [c.alloc(cap * 32) for _ in range(n)]
                cnts = [c.alloc(8) for _ in range(n)]
                spec = _lib.queue_cloud(p1, p2, prm)
                batched, single = [], []
                for rep_ in range(args.warmup + args.reps):
                    c.reset_kernel_stats()
                    for b in range(n):
                        if fovea:
                            c.enqueue_foveated_cloud(pL, pR, W, H, L.strides[0], (0, 0), outs[b], spec, pts[b], cap, cnts[b], b)
                        else:
                            c.enqueue_full_cloud(pL, pR, W, H, L.strides[0], outs[b], spec, pts[b], cap, cnts[b], b)
                    done = c.drain()
                    assert len(done) == n and all(d.call_pairs == n for d in done)
                    batched.append(misc_ms(c))
                    c.reset_kernel_stats()
                    for b in range(n):
                        sx, sy, sc = outs[b], outs[b] + plane * 4, outs[b] + 2 * plane * 4
                        if fovea:
                            c.check(c.lib.ugsm_point_cloud_fovea_all(c.handle, 0, sx, sy, sc, W, H, 0, 0, pL, L.strides[0], P1p, P2p, C.byref(prm), pts[b], cap,
                                                                     cnts[b], None))
                        else:
                            c.check(c.lib.ugsm_point_cloud(c.handle, 0, sx, sy, sc, pL, W, H, L.strides[0], P1p, P2p, C.byref(prm), pts[b], cap, cnts[b]))
                    c.check(c.lib.ugsm_wait(c.handle, 0))
                    single.append(misc_ms(c))
                b_, s_ = batched[args.warmup:], single[args.warmup:]
                emit({"what": "queue_cloud_launch_" + name, "mode": "foveated stack" if fovea else "full", "size": f"{W}x{H}", "pairs": n,
                      "batched_device_ms": round(float(np.median(b_)), 4), "batched_min": round(min(b_), 4), "batched_max": round(max(b_), 4),
                      "single_x8_device_ms": round(float(np.median(s_)), 4), "single_min": round(min(s_), 4), "single_max": round(max(s_), 4)})


MULTI_FORMS = (("dense_pcl32", 0, False), ("compact_xyzrgb16", 1, True))


def multi_offsets(kind, n, W, H, fw, fh):
    """n window offsets: 'spread' -- a grid over the frame, the level-0 windows far apart; 'clustered' -- the same grid an eighth of a
    window apart round the centre."""
    nx, ny = {2: (2, 1), 4: (2, 2), 8: (4, 2)}[n]
    dx, dy = (int(0.8 * W / nx), int(0.8 * H / ny)) if kind == "spread" else (fw // 8, fh // 8)
    return [(int((i - (nx - 1) / 2) * dx), int((j - (ny - 1) / 2) * dy)) for j in range(ny) for i in range(nx)]


def multi_child(args):
    """One size in this process, every case: prints one line "MULTIBENCH <json list of rows>"."""
    sys.path.insert(0, args.tree)
    from ug_stereomatcher_amd import _lib, synth
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(args.tree), "ug_stereomatcher_amd")
    p1, p2 = (np.ascontiguousarray(m, np.float64).reshape(12) for m in (P1, P2))
    dp = C.POINTER(C.c_double)
    P1p, P2p = p1.ctypes.data_as(dp), p2.ctypes.data_as(dp)
    levels, F = 14, 7
    W, H = (int(v) for v in args.size.split("x"))
    merged_too = hasattr(_lib.Context, "point_cloud_fovea_multi")
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 2)
    fw, fh = _lib.fovea_dims(W, H, levels, F)
    lvl = F * fw * fh * 4
    rows = []
    with _lib.Context(levels=levels, fovea_levels=F, profile_events=2) as c:
        lib, h = c.lib, c.handle
        pL, pR = c.to_device(L), c.to_device(R)
        stacks = [c.alloc(3 * lvl) for _ in range(8)]
        d_pts, d_cnt = c.alloc(8 * F * fw * fh * 32), c.alloc(8 * 8)
        for n in (2, 4, 8):
            for kind in ("spread", "clustered"):
                offs = multi_offsets(kind, n, W, H, fw, fh)
                c.submit_foveated_multi(0, pL, pR, W, H, L.strides[0], offs, stacks[:n])
                c.check(lib.ugsm_wait(h, 0))
                ox, oy = c._offsets(offs, n)
                ptrs = c._ptrs(stacks[:n])
                for name, fmt, compact in MULTI_FORMS:
                    prm = _lib.cloud_params(format=fmt, compact=compact, min_conf=0.5 if compact else None)
                    step = 32 if fmt == 0 else 16
                    row = {"size": args.size, "n": n, "offsets": kind, "form": name}
                    if merged_too:
                        cap = _lib.fovea_multi_cloud_points(W, H, levels, F, offs)
                        merged = lambda: c.check(lib.ugsm_point_cloud_fovea_multi(h, 0, n, ptrs, W, H, ox, oy, pL, L.strides[0], P1p, P2p, C.byref(prm),
                                                                                  d_pts, cap, d_cnt, None))
                        t, lo, hi, wall = spread_ms(c, merged, args.reps, args.warmup)
                        row.update(merged_device_ms=t, merged_device_ms_min=lo, merged_device_ms_max=hi, merged_wall_ms=wall,
                                   merged_records=int(c.to_host(d_cnt, (1,), np.int64)[0]), merged_launches=2 if compact else 1)
                    # the n calls it replaces, each stack's cloud behind the one before (a compact cloud needs each count back first: not timed)
                    caps = [_lib.fovea_cloud_points(W, H, levels, F, o) for o in offs]
                    one = lambda k, at: c.check(lib.ugsm_point_cloud_fovea_all(h, 0, stacks[k], stacks[k] + lvl, stacks[k] + 2 * lvl, W, H, offs[k][0],
                                                                               offs[k][1], pL, L.strides[0], P1p, P2p, C.byref(prm),
                                                                               d_pts + at * step, caps[k], d_cnt + 8 * k, None))
                    for k in range(n):
                        one(k, 0)
                    c.check(lib.ugsm_wait(h, 0))
                    counts = c.to_host(d_cnt, (n,), np.int64).tolist()
                    first = np.concatenate([[0], np.cumsum(counts)]).tolist()

                    def per_stack():
                        for k in range(n):
                            one(k, first[k])
                    t, lo, hi, wall = spread_ms(c, per_stack, args.reps, args.warmup)
                    row.update(per_stack_device_ms=t, per_stack_device_ms_min=lo, per_stack_device_ms_max=hi, per_stack_wall_ms=wall,
                               per_stack_records=int(sum(counts)), per_stack_launches=n * (2 if compact else 1))
                    rows.append(row)
        for p in [pL, pR, d_pts, d_cnt] + stacks:
            c.free(p)
    print("MULTIBENCH " + json.dumps(rows), flush=True)


def multi_main(args):
    import statistics
    import subprocess
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and not os.path.exists(os.path.join(parent, "ug_stereomatcher_amd", "libugsm.so")):
        raise SystemExit(f"{parent}: no built ug_stereomatcher_amd/libugsm.so")
    trees = {"this": ROOT}
    if parent:
        trees["parent"] = parent

    def measure(tree, size):
        cmd = [sys.executable, os.path.abspath(__file__), "--multi", "--child", "--tree", tree, "--size", size, "--reps", str(args.reps),
               "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("MULTIBENCH ")]
        if r.returncode != 0 or not lines:
            raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(lines[-1][11:])

    result = dict(tool="tools/cloud_bench.py --multi", levels=14, fovea_levels=7, rounds=args.rounds, reps=args.reps, warmup=args.warmup,
                  parent_measured=bool(parent), cases=[])
    for size in args.sizes.split(","):
        kept = {name: [] for name in trees}
        for rnd in range(args.rounds):
            names = list(trees)
            for name in (names if rnd % 2 == 0 else names[::-1]):     # alternating order
                kept[name].append(measure(trees[name], size))
                print(size, name, "round", rnd, flush=True)
        for k, first in enumerate(kept["this"][0]):
            med = lambda name, key: statistics.median(ch[k][key] for ch in kept[name])
            rng = lambda name, key: max(ch[k][key] for ch in kept[name]) - min(ch[k][key] for ch in kept[name])
            case = {key: first[key] for key in ("size", "n", "offsets", "form", "merged_records", "per_stack_records", "merged_launches",
                                                "per_stack_launches")}
            for key in ("merged_device_ms", "merged_wall_ms", "per_stack_device_ms", "per_stack_wall_ms"):
                case[key] = round(med("this", key), 4)
                case[key + "_children"] = [round(ch[k][key], 4) for ch in kept["this"]]
                case[key + "_spread"] = round(rng("this", key), 4)
            case["records_ratio"] = round(first["merged_records"] / first["per_stack_records"], 3)
            if parent:
                for key in ("per_stack_device_ms", "per_stack_wall_ms"):
                    case["parent_" + key] = round(med("parent", key), 4)
                    case["parent_" + key + "_children"] = [round(ch[k][key], 4) for ch in kept["parent"]]
                    case["parent_" + key + "_spread"] = round(rng("parent", key), 4)
                # (the spread of the parent's calls: between its children, and inside a child between its own repeats, whichever is larger)
                inside = max(ch[k]["per_stack_device_ms_max"] - ch[k]["per_stack_device_ms_min"] for ch in kept["parent"])
                case["parent_per_stack_device_ms_repeat_range"] = round(inside, 4)
                case["merged_no_longer_than_parent_calls_device"] = bool(
                    case["merged_device_ms"] <= case["parent_per_stack_device_ms"] + max(case["parent_per_stack_device_ms_spread"], inside))
                case["merged_no_longer_than_parent_calls_wall"] = bool(
                    case["merged_wall_ms"] <= case["parent_per_stack_wall_ms"] + case["parent_per_stack_wall_ms_spread"])
            result["cases"].append(case)
            print(json.dumps({a: b for a, b in case.items() if not a.endswith("_children")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
        print(f"wrote {args.out}")


LENS_CASES = (("dense_pcl32", False, None), ("compact_pcl32", True, None), ("resized_0.2_pcl32", False, 0.2))


def lens_rig(path, name):
    """K1, D1, K2, D2, P1, P2 of rig `name` of a calibration file laid out as tests/golden/lens_cal.json."""
    r = json.load(open(path))[name]
    return {k: np.array(r[k], np.float64) for k in ("K1", "D1", "K2", "D2", "P1", "P2")}


def lens_child(args):
    """One size in this process, with the lens or without: prints one line "LENSBENCH <json list of rows>"."""
    from ug_stereomatcher_amd import _lib, synth
    rig = lens_rig(args.calibration, args.rig)
    dp = C.POINTER(C.c_double)
    P1p, P2p = rig["P1"].ctypes.data_as(dp), rig["P2"].ctypes.data_as(dp)
    W, H = (int(v) for v in args.size.split("x"))
    L, _, dx, dy = synth.make_pair(W, H, synth.BASE_SEED + 2)
    conf = np.random.Generator(np.random.PCG64(7)).uniform(0, 1, (H, W)).astype(np.float32)
    rows = []
    with _lib.Context(levels=14, profile_events=2) as c:
        lib, h = c.lib, c.handle
        if args.lens_state == "on":
            c.set_lens(rig["K1"], rig["D1"], rig["K2"], rig["D2"], args.iterations)
        d = [c.to_device(np.ascontiguousarray(a)) for a in (-dx, dy, conf, L)]     # (the rig's right camera lies on the side of negative disparities)
        d_pts, d_cnt = c.alloc(W * H * 32), c.alloc(8)
        for name, compact, factor in LENS_CASES:
            prm = _lib.cloud_params(compact=compact, min_conf=0.5 if compact else None)
            if factor is None:
                call = lambda: c.check(lib.ugsm_point_cloud(h, 0, d[0], d[1], d[2], d[3], W, H, L.strides[0], P1p, P2p, C.byref(prm), d_pts, W * H, d_cnt))
            else:
                call = lambda: c.check(lib.ugsm_point_cloud_resized(h, 0, d[0], d[1], d[2], d[3], W, H, L.strides[0], P1p, P2p, C.c_float(factor),
                                                                    C.byref(prm), d_pts, W * H, d_cnt))
            t, lo, hi, wall = spread_ms(c, call, args.reps, args.warmup)
            rows.append(dict(case=name, device_ms=t, device_ms_min=lo, device_ms_max=hi, wall_ms=wall, records=int(c.to_host(d_cnt, (1,), np.int64)[0])))
        for p in d + [d_pts, d_cnt]:
            c.free(p)
    print("LENSBENCH " + json.dumps(rows), flush=True)


def lens_merge(out, key, value):
    """profiles/lens_bench.json holds the cloud tool's and the depth tool's results side by side."""
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(f"wrote {out}")


def lens_main(args):
    import statistics
    import subprocess

    def measure(state, size):
        cmd = [sys.executable, os.path.abspath(__file__), "--lens", "--child", "--lens-state", state, "--size", size, "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--calibration", args.calibration, "--rig", args.rig, "--iterations", str(args.iterations)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LENSBENCH ")]
        if r.returncode != 0 or not lines:
            raise SystemExit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(lines[-1][10:])

    result = dict(tool="tools/cloud_bench.py --lens", rig=args.rig, iterations=args.iterations, rounds=args.rounds, reps=args.reps, warmup=args.warmup,
                  cases=[])
    for size in args.sizes.split(","):
        kept = {"off": [], "on": []}
        for rnd in range(args.rounds):
            for state in (("off", "on") if rnd % 2 == 0 else ("on", "off")):     # alternating order
                kept[state].append(measure(state, size))
                print(size, "lens", state, "round", rnd, flush=True)
        for k, first in enumerate(kept["off"][0]):
            case = dict(size=size, case=first["case"], records=first["records"], records_lens=kept["on"][0][k]["records"])
            for state, tag in (("off", "no_lens"), ("on", "lens")):
                ms = [ch[k]["device_ms"] for ch in kept[state]]
                case[tag + "_device_ms"] = round(statistics.median(ms), 4)
                case[tag + "_device_ms_children"] = [round(v, 4) for v in ms]
                case[tag + "_device_ms_spread"] = round(max(ms) - min(ms), 4)
                case[tag + "_wall_ms"] = round(statistics.median(ch[k]["wall_ms"] for ch in kept[state]), 4)
            case["lens_over_no_lens"] = round(case["lens_device_ms"] / case["no_lens_device_ms"], 3)
            result["cases"].append(case)
            print(json.dumps({a: b for a, b in case.items() if not a.endswith("_children")}), flush=True)
    lens_merge(args.out or os.path.join(ROOT, "profiles", "lens_bench.json"), "cloud", result)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="4928x3264,1920x1080")
    ap.add_argument("--resized", action="store_true", help="the resized cloud's rows instead")
    ap.add_argument("--stack", action="store_true", help="the merged cloud of the fovea stack and the two paths it replaces instead")
    ap.add_argument("--queue", action="store_true", help="the cloud from the queue: pairs/s of the managed legs and the batched launch's device time")
    ap.add_argument("--pairs", type=int, default=64, help="--queue: pairs per timed burst")
    ap.add_argument("--leg", choices=QUEUE_LEGS + ("launch",), help="--queue: this leg only")
    ap.add_argument("--mode", choices=("full", "foveated"), help="--queue: this mode only")
    ap.add_argument("--multi", action="store_true", help="the merged cloud of several windows of one pair and the per-stack calls it replaces instead")
    ap.add_argument("--parent-tree", default=None, help="--multi: a checkout of the parent commit with its libraries built")
    ap.add_argument("--rounds", type=int, default=3, help="--multi: children per configuration")
    ap.add_argument("--child", action="store_true", help="(internal) --multi: measure in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the tree whose package the child loads")
    ap.add_argument("--size", default="4928x3264", help="(internal)")
    ap.add_argument("--lens", action="store_true", help="the dense, compact and resized cloud without a lens and with it instead")
    ap.add_argument("--calibration", default=os.path.join(ROOT, "tests", "golden", "lens_cal.json"), help="--lens: K, D, P of the two cameras")
    ap.add_argument("--rig", default="rig16mp", help="--lens: the rig of the calibration file")
    ap.add_argument("--iterations", type=int, default=5, help="--lens: ugsm_set_lens's iterations")
    ap.add_argument("--lens-state", choices=("off", "on"), default="off", help="(internal) --lens: the child's setting")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.multi:
        return multi_child(args) if args.child else multi_main(args)
    if args.lens:
        if args.sizes == "4928x3264,1920x1080":
            args.sizes = "4928x3264"
        return lens_child(args) if args.child else lens_main(args)
    from ug_stereomatcher_amd import _lib, synth
    import torch
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    p1, p2 = (np.ascontiguousarray(m, np.float64).reshape(12) for m in (P1, P2))
    dp = C.POINTER(C.c_double)
    if args.queue:
        if args.leg != "launch":
            queue_rows(args, emit, p1, p2)
        if args.leg == "launch" or (args.leg is None and args.mode is None):
            queue_launch_rows(args, emit, p1, p2, dp)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            old = []
            if os.path.exists(args.out) and (args.leg or args.mode):   # legs run one by one add to the file
                with open(args.out) as f:
                    old = json.load(f)
            with open(args.out, "w") as f:
                json.dump(old + rows, f, indent=1)
        return
    copy = copy_rate_GBps(torch)
    emit({"what": "device_copy", "GBps": round(copy, 1)})
    if args.resized:
        resized_rows(args, emit, copy, p1, p2, dp)
        sizes = []
    elif args.stack:
        stack_rows(args, emit, p1, p2, dp)
        sizes = []
    else:
        sizes = args.sizes.split(",")
    for size in sizes:
        W, H = (int(v) for v in size.split("x"))
        L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 2)
        with _lib.Context(levels=14, profile_events=2) as c:
            pL, pR = c.to_device(L), c.to_device(R)
            d_out = c.alloc(3 * W * H * 4)
            c.check(c.lib.ugsm_submit_full(c.handle, 0, pL, pR, W, H, L.strides[0], d_out))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            plane = W * H * 4
            d_dx, d_dy, d_conf = d_out, d_out + plane, d_out + 2 * plane
            d_pts, d_cnt = c.alloc(W * H * 32), c.alloc(8)
            host = c.host_array((W * H * 32,), np.uint8)
            h_addr = host.ctypes.data
            # today's path: X, Y, Z planes, then the three planes to the host
            d_xyz = c.alloc(3 * plane)
            tri = lambda: c.check(c.lib.ugsm_triangulate(c.handle, 0, d_dx, d_dy, W, H, p1.ctypes.data_as(dp), p2.ctypes.data_as(dp), d_xyz))
            t_tri = median_ms(c, tri, args.reps, args.warmup)
            t_planes = host_copy_ms(c, h_addr, d_xyz, 3 * plane, max(5, args.reps // 3))
            mb = (8 + 12) * W * H / 1e6
            emit({"what": "planes_today", "size": size, "device_ms": round(t_tri, 4), "MB": round(mb, 1), "GBps": round(mb / t_tri, 1),
                  "d2h_MB": round(3 * plane / 1e6, 1), "d2h_ms": round(t_planes, 3), "total_ms": round(t_tri + t_planes, 3)})
            c.free(d_xyz)
            for s in (1, 2):
                for name, fmt, compact in (("dense_pcl32", 0, False), ("dense_xyzrgb16", 1, False), ("compact_pcl32", 0, True),
                                           ("compact_xyzrgb16", 1, True)):
                    prm = _lib.cloud_params(sampling=s, format=fmt, compact=compact, min_conf=0.5 if compact else None)
                    npts = _lib.cloud_points(W, H, s)
                    call = lambda: c.check(c.lib.ugsm_point_cloud(c.handle, 0, d_dx, d_dy, d_conf, pL, W, H, L.strides[0], p1.ctypes.data_as(dp),
                                                                  p2.ctypes.data_as(dp), C.byref(prm), d_pts, npts, d_cnt))
                    t = median_ms(c, call, args.reps, args.warmup)
                    count = int(c.to_host(d_cnt, (1,), np.int64)[0])
                    step = 32 if fmt == 0 else 16
                    read = npts * ((8 + 4) + (8 + 4 + 3) if compact else 8 + 3)
                    mb = (read + count * step) / 1e6
                    floor = mb / 1e3 / copy * 1e3  # ms
                    t_d2h = host_copy_ms(c, h_addr, d_pts, count * step, max(5, args.reps // 3)) if count else 0.0
                    emit({"what": name, "size": size, "sampling": s, "points": npts, "count": count, "device_ms": round(t, 4),
                          "MB": round(mb, 1), "GBps": round(mb / t, 1), "of_copy": round(mb / t / copy, 3), "floor_ms": round(floor, 4),
                          "of_floor": round(floor / t, 3), "d2h_MB": round(count * step / 1e6, 1), "d2h_ms": round(t_d2h, 3),
                          "total_ms": round(t + t_d2h, 3)})
            for p in (pL, pR, d_out, d_pts, d_cnt):
                c.free(p)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
