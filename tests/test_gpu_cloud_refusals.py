"""What row f-1's entry points refuse: a table of (entry point, one argument broken) -> status and, where the call sets one, ugsm_last_error.

The slot-level calls of ugsm_cloud.cpp, ugsm_match_full_depth and the queue's ugsm_enqueue_*_cloud*.  Every row starts from arguments the call
would accept -- real device buffers of the right size, 32 x 24 planes; a 280 x 210 image for the fovea forms, the blocking call and the
queue, the smallest 4 : 3 size ugsm_fovea_dims accepts at 14 / 7 levels -- and breaks one.  No kernel runs: every row is refused, and at
the end nothing is outstanding on the queue.  The expected column is what the library answered before the row f-1 fold."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_cloud import P1 as P1_, P2 as P2_

pytestmark = pytest.mark.gpu

PW, PH = 32, 24                     # the planes of the slot-level calls (and their image)
W, H, LEVELS, F = 280, 210, 14, 7   # the fovea forms, the blocking call, the queue
BAD, MISMATCH = 1, 2                # UGSM_ERR_BAD_ARG, UGSM_ERR_SIZE_MISMATCH
NAN = math.nan

Q_SPEC = "ugsm_enqueue_*_cloud*: null spec"
Q_FORMAT = "ugsm_enqueue_*_cloud*: sampling < 1 or an unknown record format"
Q_WINDOW = "ugsm_enqueue_*_cloud*: a NaN min_conf / z_min / z_max, or z_min > z_max"
Q_MAX = "ugsm_enqueue_*_cloud*: max_points < 0"
Q_BUFFER = "ugsm_enqueue_*_cloud: a null or misaligned cloud buffer, or cap_points < 0"
Q_STRIDE = "ugsm_enqueue_*: stride < bytes per pixel of the input format * W"
Q_TAU = "ugsm_enqueue_full_checked*: tau must be > 0"
Q_IMAGE = "ugsm_enqueue_*_managed: null image"

# entry point -> the names of its arguments, in order ("p.*": fields of the params struct, "spec.*": of the ugsm_queue_cloud)
CLOUD_TAIL = ["rgb", "W", "H", "stride", "P1", "P2"]
OUT = ["p", "points", "cap", "count"]
FOVEA = ["fw", "fh", "level", "left", "upper", "scale"]
ARGS = {
    "ugsm_triangulate": ["ctx", "slot", "dx", "dy", "pw", "ph", "P1", "P2", "xyz"],
    "ugsm_triangulate_fovea": ["ctx", "slot", "sx", "sy"] + FOVEA + ["P1", "P2", "xyz"],
    "ugsm_point_cloud": ["ctx", "slot", "dx", "dy", "conf"] + CLOUD_TAIL + OUT,
    "ugsm_point_cloud_fovea": ["ctx", "slot", "sx", "sy", "sc"] + FOVEA + CLOUD_TAIL + OUT,
    "ugsm_point_cloud_fovea_all": ["ctx", "slot", "sx", "sy", "sc", "W", "H", "off_x", "off_y", "rgb", "stride", "P1", "P2"] + OUT + ["level_counts"],
    "ugsm_point_cloud_fovea_multi": ["ctx", "slot", "n", "stacks", "W", "H", "offs_x", "offs_y", "rgb", "stride", "P1", "P2"] + OUT + ["level_counts"],
    "ugsm_point_cloud_resized": ["ctx", "slot", "dx", "dy", "conf"] + CLOUD_TAIL + ["factor"] + OUT,
    "ugsm_point_cloud_resized_fovea": ["ctx", "slot", "sx", "sy", "sc"] + FOVEA + CLOUD_TAIL + ["factor", "colour_mapped"] + OUT,
    "ugsm_depth_image": ["ctx", "slot", "dx", "dy", "conf", "pw", "ph", "P1", "P2", "dp", "depth", "valid"],
    "ugsm_depth_image_fovea": ["ctx", "slot", "sx", "sy", "sc", "W", "H", "off_x", "off_y", "level", "P1", "P2", "dp", "depth", "valid"],
    "ugsm_match_full_depth": ["ctx", "L", "R", "W", "H", "stride", "P1", "P2", "dp", "host_depth", "null", "null", "null"],
    "ugsm_enqueue_full_cloud": ["ctx", "dL", "dR", "W", "H", "stride", "out", "spec", "points", "cap", "count", "tag"],
    "ugsm_enqueue_foveated_cloud": ["ctx", "dL", "dR", "W", "H", "stride", "off_x", "off_y", "out", "spec", "points", "cap", "count", "level_counts", "tag"],
    "ugsm_enqueue_full_cloud_managed": ["ctx", "L", "R", "W", "H", "stride", "spec", "tag"],
    "ugsm_enqueue_foveated_cloud_managed": ["ctx", "L", "R", "W", "H", "stride", "off_x", "off_y", "spec", "tag"],
    "ugsm_enqueue_full_checked_cloud": ["ctx", "dL", "dR", "W", "H", "stride", "out", "back", "tau", "spec", "points", "cap", "count", "tag"],
    "ugsm_enqueue_full_checked_cloud_managed": ["ctx", "L", "R", "W", "H", "stride", "tau", "want_back", "spec", "tag"],
}
PLANES = {"ugsm_point_cloud", "ugsm_point_cloud_resized"}          # (their image is the planes' size)


def _rows():
    rows = []

    def add(entry, broken, status=BAD, message=None):
        rows.append(pytest.param(entry, broken, status, message, id=f"{entry[5:]}-" + ",".join(f"{k}={v}" for k, v in broken.items())))

    def nulls(entry, names):
        for a in names:
            add(entry, {a: None})

    window = [{"p.min_conf": NAN}, {"p.z_min": NAN}, {"p.z_max": NAN}, {"p.z_min": 2.0, "p.z_max": 1.0}]
    nulls("ugsm_triangulate", ["ctx", "dx", "dy", "P1", "P2", "xyz"])
    add("ugsm_triangulate", {"pw": 0})
    nulls("ugsm_triangulate_fovea", ["ctx", "sx", "sy", "P1", "P2", "xyz"])
    add("ugsm_triangulate_fovea", {"fh": 0})
    add("ugsm_triangulate_fovea", {"level": -1})
    for e in ("ugsm_point_cloud", "ugsm_point_cloud_fovea", "ugsm_point_cloud_resized", "ugsm_point_cloud_resized_fovea"):
        first = ["dx", "dy"] if e in PLANES else ["sx", "sy"]
        nulls(e, ["ctx"] + first + ["rgb", "P1", "P2", "p", "points", "count"])
        add(e, {"points": "+8"})
        add(e, {"count": "+4"})
        add(e, {"cap": -1})
        add(e, {"p.sampling": 0})
        add(e, {"p.format": 2})
        for w in window:
            add(e, w)
        add(e, {"p.min_conf": 0.5, "conf" if e in PLANES else "sc": None})
        add(e, {"stride": "-1"})
        add(e, {"H": 0})
    for e in ("ugsm_point_cloud_fovea", "ugsm_point_cloud_resized_fovea"):
        add(e, {"level": -1})
        add(e, {"level": 32})
        add(e, {"scale": NAN})
    for e in ("ugsm_point_cloud_resized", "ugsm_point_cloud_resized_fovea"):
        add(e, {"factor": 0.0})
        add(e, {"factor": 1.5})
        add(e, {"factor": 0.03})                                  # (int)(32 * 0.03f) = 0: a side at 0
        add(e, {"p.sampling": 2})
    add("ugsm_point_cloud_resized_fovea", {"colour_mapped": 2})
    add("ugsm_point_cloud_resized_fovea", {"colour_mapped": -1})
    for e in ("ugsm_point_cloud_fovea_all", "ugsm_point_cloud_fovea_multi"):
        nulls(e, ["ctx", "rgb", "P1", "P2", "p", "points", "count"] + (["sx", "sy"] if e.endswith("all") else ["stacks", "stack1"]))
        add(e, {"points": "+8"})
        add(e, {"count": "+4"})
        add(e, {"level_counts": "+4"})
        add(e, {"cap": -1})
        add(e, {"p.sampling": 0})
        add(e, {"p.format": -1})
        for w in window:
            add(e, w)
        add(e, {"stride": "-1"})
    add("ugsm_point_cloud_fovea_all", {"p.min_conf": 0.5, "sc": None})
    add("ugsm_point_cloud_fovea_multi", {"n": 0})
    add("ugsm_point_cloud_fovea_multi", {"n": 17})
    for e in ("ugsm_depth_image", "ugsm_depth_image_fovea"):
        first = ["dx", "dy"] if e == "ugsm_depth_image" else ["sx", "sy"]
        nulls(e, ["ctx"] + first + ["P1", "P2", "dp", "depth"])
        add(e, {"depth": "+2"})                                   # (32FC1: 4-byte elements)
        add(e, {"depth": "+1", "dp.format": 1})                   # (16UC1: 2-byte elements)
        add(e, {"valid": "+4"})
        add(e, {first[0]: "+2"})
        add(e, {"dp.format": 2})
        for unit in (0.0, -1.0, NAN, math.inf):
            add(e, {"dp.unit": unit})
        for w in window:
            add(e, {"d" + k: v for k, v in w.items()})
        add(e, {"dp.min_conf": 0.5, "conf" if e == "ugsm_depth_image" else "sc": None})
        add(e, {"dp.factor": 0.0})
        add(e, {"dp.factor": 1.5})
        add(e, {"dp.factor": 0.03})
        for src in first + ["conf" if e == "ugsm_depth_image" else "sc"]:
            add(e, {"depth": "=" + src})                          # the image would overwrite what it is made from
            add(e, {"depth": "=" + src + "+last"})                # ... its first element on the input's last float
    add("ugsm_depth_image", {"pw": 0})
    add("ugsm_depth_image_fovea", {"level": F})
    add("ugsm_depth_image_fovea", {"level": -2})
    add("ugsm_depth_image_fovea", {"W": 0})
    nulls("ugsm_match_full_depth", ["ctx", "P1", "P2", "dp", "host_depth"])
    add("ugsm_match_full_depth", {"dp.format": 2})
    add("ugsm_match_full_depth", {"dp.unit": 0.0})
    for w in window:
        add("ugsm_match_full_depth", {"d" + k: v for k, v in w.items()})
    for f in (0.0, 1.5, 0.001):
        add("ugsm_match_full_depth", {"dp.factor": f})
    for e in [k for k in ARGS if k.startswith("ugsm_enqueue")]:
        managed, name = e.endswith("_managed"), e
        add(e, {"ctx": None})
        add(e, {"spec": None}, BAD, Q_SPEC)
        add(e, {"L" if managed else "dL": None}, BAD, Q_IMAGE if managed else f"{name}: null buffer")
        add(e, {"R" if managed else "dR": None}, BAD, Q_IMAGE if managed else f"{name}: null buffer")
        add(e, {"stride": "-1"}, MISMATCH, Q_STRIDE)
        add(e, {"spec.sampling": 0}, BAD, Q_FORMAT)
        add(e, {"spec.format": 2}, BAD, Q_FORMAT)
        for w in window:
            add(e, {"spec." + k[2:]: v for k, v in w.items()}, BAD, Q_WINDOW)
        add(e, {"spec.max_points": -1}, BAD, Q_MAX)
        if "checked" in e:
            add(e, {"tau": 0.0}, BAD, Q_TAU)
        if managed:
            continue
        add(e, {"out": None}, BAD, f"{name}: null buffer")
        for broken in ({"points": None}, {"count": None}, {"points": "+8"}, {"count": "+4"}, {"cap": -1}):
            add(e, broken, BAD, Q_BUFFER)
    add("ugsm_enqueue_foveated_cloud", {"level_counts": "+4"}, BAD, Q_BUFFER)
    return rows


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def base(lib):
    """A one-slot context and the arguments every entry point would accept."""
    with lib.Context(levels=LEVELS, fovea_levels=F, slots=1, batch=4) as c:
        fw, fh = lib.fovea_dims(W, H, LEVELS, F)
        n, sn = PW * PH, F * fw * fh
        held = []

        def dev(nbytes):
            held.append(c.to_device(np.zeros(nbytes, np.uint8)))
            return held[-1]
        planes, stacks = dev(3 * n * 4), [dev(3 * sn * 4) for _ in range(2)]
        left, upper, scale = lib.fovea_level_mapping(W, H, LEVELS, F, 2)
        L = np.zeros((H, W, 3), np.uint8)
        dp = C.POINTER(C.c_double)
        p1, p2 = np.ascontiguousarray(P1_, np.float64).reshape(12), np.ascontiguousarray(P2_, np.float64).reshape(12)
        a = dict(ctx=c.handle, slot=0, null=None, tag=7, dx=planes, dy=planes + 4 * n, conf=planes + 8 * n, pw=PW, ph=PH,
                 sx=stacks[0], sy=stacks[0] + 4 * sn, sc=stacks[0] + 8 * sn, stack1=stacks[1], fw=fw, fh=fh, level=2, left=left, upper=upper,
                 scale=float(scale), rgb=dev(3 * W * H), dL=dev(3 * W * H), dR=dev(3 * W * H), L=L.ctypes.data, R=L.ctypes.data, W=W, H=H, stride=3 * W,
                 P1=p1.ctypes.data_as(dp), P2=p2.ctypes.data_as(dp), xyz=dev(3 * sn * 4), points=dev(32 * W * H), cap=W * H, count=dev(8),
                 level_counts=dev(8 * 32), n=2, off_x=0, off_y=0, offs_x=None, offs_y=None, factor=0.5, colour_mapped=0,
                 depth=dev(4 * sn), valid=dev(8 * F), host_depth=np.zeros(W * H, np.float32).ctypes.data, out=dev(3 * max(W * H, sn) * 4),
                 back=None, tau=1.0, want_back=0, p=lib.cloud_params(), dp=lib.depth_params(), spec=None)
        a["spec"] = lib.queue_cloud(P1_, P2_, lib.cloud_params())
        a["_keep"], a["_sizes"] = (L, p1, p2), dict(dx=4 * n, dy=4 * n, conf=4 * n, sx=4 * sn, sy=4 * sn, sc=4 * sn)
        yield c, a
        assert c.queue_depth() == (0, 0, 0), "a refused pair was enqueued"
        for p in held:
            c.free(p)


def _copy(s):
    t = type(s)()
    C.memmove(C.byref(t), C.byref(s), C.sizeof(s))
    return t


@pytest.mark.parametrize("entry,broken,status,message", _rows())
def test_refused(lib, base, entry, broken, status, message):
    c, good = base
    a = dict(good)
    if entry in PLANES:
        a.update(W=PW, H=PH, stride=3 * PW)
    for k, v in broken.items():
        if "." in k:
            struct, field = k.split(".")
            a[struct] = _copy(a[struct])
            target = a[struct].params if struct == "spec" and field != "max_points" else a[struct]
            setattr(target, field, v)
        elif isinstance(v, str) and v[0] == "=":                 # the depth image over one of its inputs
            src = v[1:].split("+")[0]
            a[k] = good[src] + (good["_sizes"][src] - 4 if v.endswith("+last") else 0)
        elif isinstance(v, str):                                  # "+8": misaligned by 8 bytes; "-1": one less
            a[k] = a[k] + int(v)
        else:
            a[k] = v
    if entry == "ugsm_point_cloud_fovea_multi":
        a["stacks"] = None if "stacks" in broken else (C.c_void_p * 17)(*([a["sx"], a["stack1"]] + [a["sx"]] * 15))
    args = []
    for name in ARGS[entry]:
        v = a[name]
        if name in ("scale", "factor", "tau"):
            v = C.c_float(v)
        elif name in ("p", "dp", "spec") and v is not None:
            v = C.byref(v)
        args.append(v)
    got = getattr(c.lib, entry)(*args)
    text = c.lib.ugsm_last_error(c.handle).decode()
    print(f"{entry} {broken}: status {got}, last error {text!r}")
    assert got == status
    if message is not None:
        assert text == message
