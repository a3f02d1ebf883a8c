"""The coloured point cloud (ugsm_point_cloud / ugsm_point_cloud_fovea) without a GPU: the C-ABI's declarations and exports, the
parameter defaults and layout, the host-only size rule, argument refusals, and the CPU restatement (tests/cloud_np.py) on a hand-made
example."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_np as cn
from conftest import ROOT

NEW = ["ugsm_default_cloud_params", "ugsm_cloud_points", "ugsm_point_cloud", "ugsm_point_cloud_fovea"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_cloud_symbols_are_declared_and_exported_by_both_libraries(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    assert "#define UGSM_CLOUD_PCL32    0" in hdr and "#define UGSM_CLOUD_XYZRGB16 1" in hdr
    assert lib.load().ugsm_abi_version() == 6


def test_default_cloud_params(lib):
    p = lib.CloudParams(7, 9, 9, 1.0, 2.0, 3.0)
    lib.load().ugsm_default_cloud_params(C.byref(p))
    assert (p.sampling, p.format, p.compact) == (1, lib.UGSM_CLOUD_PCL32, 0)
    assert p.min_conf == -np.inf and p.z_min == -np.inf and p.z_max == np.inf
    lib.load().ugsm_default_cloud_params(None)   # (no crash)


def test_cloud_points(lib):
    f = lib.load().ugsm_cloud_points
    for (W, H, s) in [(5, 4, 1), (5, 4, 2), (5, 4, 3), (33, 7, 7), (4928, 3264, 1), (4928, 3264, 2), (1920, 1080, 3), (1, 1, 9)]:
        assert f(W, H, s) == cn.cloud_points(W, H, s) == -(-W // s) * -(-H // s)
    assert f(5, 4, 2) == 6 and f(4928, 3264, 1) == 4928 * 3264
    for bad in [(0, 4, 1), (5, 0, 1), (5, 4, 0), (-1, 4, 1), (5, 4, -2)]:
        assert f(*bad) == -1, bad


def test_cloud_params_layout_matches_c99(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ugsm.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ugsm_cloud_params), offsetof(ugsm_cloud_params, sampling),\n'
                   "           offsetof(ugsm_cloud_params, format), offsetof(ugsm_cloud_params, compact), offsetof(ugsm_cloud_params, min_conf),\n"
                   "           offsetof(ugsm_cloud_params, z_min), offsetof(ugsm_cloud_params, z_max));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = lib.CloudParams
    assert got == [C.sizeof(P), P.sampling.offset, P.format.offset, P.compact.offset, P.min_conf.offset, P.z_min.offset, P.z_max.offset]


def _call(lib, ctx=None, fovea=False, **over):
    """One ugsm_point_cloud[_fovea] call with plausible (fake, never dereferenced) device pointers, `over` replacing arguments."""
    P = (C.c_double * 12)(*range(12))
    a = dict(dx=0x10000, dy=0x20000, conf=0x30000, rgb=0x40000, W=64, H=32, stride=192, P1=P, P2=P,
             p=lib.cloud_params(), points=0x50000, cap=100, count=0x60000)
    a.update(over)
    p = C.byref(a["p"]) if a["p"] is not None else None
    so = lib.load()
    if fovea:
        return so.ugsm_point_cloud_fovea(ctx, 0, a["dx"], a["dy"], a["conf"], 40, 20, 0, 8, 6, C.c_float(1.0), a["rgb"], a["W"], a["H"],
                                         a["stride"], a["P1"], a["P2"], p, a["points"], a["cap"], a["count"])
    return so.ugsm_point_cloud(ctx, 0, a["dx"], a["dy"], a["conf"], a["rgb"], a["W"], a["H"], a["stride"], a["P1"], a["P2"], p,
                               a["points"], a["cap"], a["count"])


def bad_argument_cases(lib):
    """Every argument refusal of the cloud entry points (name, overrides); shared with the GPU test, which makes them on a live context."""
    nan = float("nan")
    return [
        ("dx", dict(dx=None)), ("dy", dict(dy=None)), ("rgb", dict(rgb=None)), ("P1", dict(P1=None)), ("P2", dict(P2=None)),
        ("params", dict(p=None)), ("points", dict(points=None)), ("count", dict(count=None)),
        ("W", dict(W=0)), ("H", dict(H=0)), ("stride", dict(stride=191)),
        ("sampling", dict(p=lib.cloud_params(sampling=0))), ("format", dict(p=lib.cloud_params(format=2))),
        ("min_conf NaN", dict(p=lib.cloud_params(compact=True, min_conf=nan))), ("z_min NaN", dict(p=lib.cloud_params(z_min=nan))),
        ("z_max NaN", dict(p=lib.cloud_params(z_max=nan))), ("z_min > z_max", dict(p=lib.cloud_params(z_min=2.0, z_max=1.0))),
        ("conf NULL, min_conf finite", dict(conf=None, p=lib.cloud_params(compact=True, min_conf=0.5))),
        ("cap < 0", dict(cap=-1)), ("points misaligned", dict(points=0x50008)),
    ]


def test_null_context_and_bad_arguments_are_refused_without_a_device(lib):
    assert _call(lib) == lib.UGSM_ERR_BAD_ARG           # (no context)
    assert _call(lib, fovea=True) == lib.UGSM_ERR_BAD_ARG
    for name, over in bad_argument_cases(lib):
        assert _call(lib, **over) == lib.UGSM_ERR_BAD_ARG, name
        assert _call(lib, fovea=True, **over) == lib.UGSM_ERR_BAD_ARG, name


# ---- the restatement on a hand-made 5 x 4 example ---------------------------------------------------------------------------------

W5, H4 = 5, 4


def _hand_planes():
    y, x = np.mgrid[0:H4, 0:W5]
    X = (10 * x + y).astype(np.float32)            # X names the pixel: 10 * column + row
    Y = (-x).astype(np.float32)
    Z = (1 + x + y).astype(np.float32)
    rgb = np.zeros((H4, W5, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 16 * x + y, 200, 255 - x
    return np.stack([X, Y, Z]), rgb


def test_restatement_order_colour_and_record_bytes():
    xyz, rgb = _hand_planes()
    word = cn.colour_word(rgb)
    assert word[1, 2] == (33 << 16) | (200 << 8) | 253
    r = cn.records(xyz, word)
    assert r.size == 20
    # column ii outer, row jj inner
    assert r["x"].tolist() == [10 * i + j for i in range(W5) for j in range(H4)]
    b = r[6].tobytes()   # record 6 = column 1, row 2
    assert len(b) == 32
    assert np.frombuffer(b[:16], np.float32).tolist() == [12.0, -1.0, 4.0, 1.0]
    assert b[16:20] == bytes([254, 200, 18, 0])     # the rgb word little-endian: B, G, R, alpha 0
    assert b[20:] == bytes(12)
    r16 = cn.records(xyz, word, fmt=cn.XYZRGB16)
    assert r16.dtype.itemsize == 16 and r16[6].tobytes() == b[:12] + b[16:20]


def test_restatement_sampling():
    xyz, rgb = _hand_planes()
    word = cn.colour_word(rgb)
    r = cn.records(xyz, word, s=2)
    assert r["x"].tolist() == [0, 2, 20, 22, 40, 42] and r.size == cn.cloud_points(W5, H4, 2)
    r = cn.records(xyz, word, s=3)
    assert r["x"].tolist() == [0, 3, 30, 33]
    assert cn.records(xyz, word, s=7)["x"].tolist() == [0]


def test_restatement_compaction():
    xyz, rgb = _hand_planes()
    word = cn.colour_word(rgb)
    xyz[0, 0, 1] = np.nan        # pixel (1, 0): X NaN
    xyz[2, 1, 0] = np.inf        # pixel (0, 1): Z inf
    xyz[1, 3, 4] = -np.inf       # pixel (4, 3): Y -inf
    conf = np.full((H4, W5), 0.9, np.float32)
    conf[2, 2] = 0.1             # pixel (2, 2)
    conf[0, 3] = np.nan          # pixel (3, 0)
    dense = cn.records(xyz, word, conf=conf)
    assert dense.size == 20 and np.isnan(dense["x"][4])
    r = cn.records(xyz, word, conf=conf, compact=True, min_conf=0.5)
    drop = {(1, 0), (0, 1), (4, 3), (2, 2), (3, 0)}
    keep = [(i, j) for i in range(W5) for j in range(H4) if (i, j) not in drop]
    assert r["x"].tolist() == [10 * i + j for i, j in keep]
    # -inf min_conf still drops the NaN confidence; without a plane there is no confidence test
    assert (30.0 not in cn.records(xyz, word, conf=conf, compact=True)["x"])
    assert (30.0 in cn.records(xyz, word, compact=True)["x"])
    # the Z window (Z = 1 + x + y)
    r = cn.records(xyz, word, compact=True, z_min=3.0, z_max=4.0)
    assert r["x"].tolist() == [10 * i + j for i in range(W5) for j in range(H4) if 3 <= 1 + i + j <= 4 and (i, j) not in {(1, 0), (0, 1), (4, 3)}]
    r = cn.records(xyz, word, s=2, compact=True, z_max=3.0)
    assert r["x"].tolist() == [0, 2, 20]


def test_fovea_colour_clamp_never_fires_at_the_rig_sizes(lib):
    """At destination level 0, every fovea level's mapped window lies inside the image at 16 MP, 1080p, 640 x 480 and 160 x 120 (the
    clamp of the colour lookup is inert there); margins pushed past the edge make it act."""
    for (W, H, levels) in [(4928, 3264, 14), (1920, 1080, 14), (640, 480, 14), (160, 120, 8)]:
        fw, fh = lib.fovea_dims(W, H, levels, 7)
        for src in range(7):
            left, upper, scale = lib.fovea_mapping(W, H, src)
            cx, cy, fired = cn.fovea_colour_at(W, H, fw, fh, left, upper, scale)
            assert not fired, (W, H, src)
    fw, fh = lib.fovea_dims(4928, 3264, 14, 7)
    left, upper, scale = lib.fovea_mapping(4928, 3264, 6)
    cx, cy, fired = cn.fovea_colour_at(4928, 3264, fw, fh, left, upper, scale)
    assert cx.max() == 4911 and cy.max() == 3247    # the worst case: level 6 at 16 MP
    assert cn.fovea_colour_at(4928, 3264, fw, fh, left + 100, upper - 300, scale)[2]
