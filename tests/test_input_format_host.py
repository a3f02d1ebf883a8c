"""The input formats (include/ugsm.h UGSM_INPUT_*) without a GPU: the new entry points are declared and exported by both libraries at ABI 6,
the bytes-per-pixel and encoding tables, the NumPy conversions of tests/encode_np.py, the argument checks that need no device, and the ROS node
with its in-place path still passing the syntax check against tests/ros_stubs/."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import encode_np as en

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ugsm_input_bytes_per_pixel", "ugsm_input_format_from_encoding", "ugsm_set_input_format", "ugsm_get_input_format"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_declared_and_exported_by_both_libraries_at_abi_6(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    assert re.search(r"#define UGSM_ABI_VERSION 6\b", hdr)
    for k, name in enumerate(("RGB8", "BGR8", "RGBA8", "BGRA8", "MONO8")):
        assert re.search(rf"#define UGSM_INPUT_{name}\s+{k}\b", hdr), name
        assert getattr(lib, f"UGSM_INPUT_{name}") == k
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert re.search(rf"\b{name}\s*\(", hdr), name
            assert hasattr(so, name), (path, name)
        assert so.ugsm_abi_version() == 6
    assert set(NEW) <= set(lib.EXPORTS)


def test_bytes_per_pixel_table(lib):
    assert [lib.input_bytes_per_pixel(f) for f in range(5)] == [3, 3, 4, 4, 1]
    for bad in (-1, 5, 6, 1 << 20, -(1 << 31)):
        assert lib.input_bytes_per_pixel(bad) == -1
    assert {f: lib.input_bytes_per_pixel(f) for f in en.FORMATS} == en.BPP


def test_encoding_table(lib):
    for f, name in en.NAMES.items():
        assert lib.input_format_from_encoding(name) == f
    for bad in ("RGB8", "rgb8 ", "", "bgr16", "mono16", "bayer_rggb8", "yuv422", "8UC3", "rgb"):
        assert lib.input_format_from_encoding(bad) == -1, bad
    assert lib.load().ugsm_input_format_from_encoding(None) == -1
    assert lib.input_format_from_encoding(None) == -1


def test_context_entry_points_refuse_a_null_context(lib):
    so = lib.load()
    f = C.c_int(-7)
    assert so.ugsm_set_input_format(None, 0) == lib.UGSM_ERR_BAD_ARG
    assert so.ugsm_get_input_format(None, C.byref(f)) == lib.UGSM_ERR_BAD_ARG and f.value == -7


def test_numpy_round_trips():
    rng = np.random.Generator(np.random.PCG64(5))
    rgb = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    for f in en.FORMATS:
        img = en.encode(rgb, f)
        assert img.dtype == np.uint8 and img.shape == ((7, 13) if f == en.MONO8 else (7, 13, en.BPP[f]))
        conv = en.to_rgb8(img, f)
        if f == en.MONO8:
            assert np.array_equal(conv, np.repeat(rgb[..., :1], 3, axis=2))
        else:
            assert np.array_equal(conv, rgb)
    # the table itself, pixel by pixel
    p = np.array([[[10, 20, 30, 40]]], np.uint8)
    assert en.to_rgb8(p[..., :3], en.BGR8).tolist() == [[[30, 20, 10]]]
    assert en.to_rgb8(p, en.RGBA8).tolist() == [[[10, 20, 30]]]
    assert en.to_rgb8(p, en.BGRA8).tolist() == [[[30, 20, 10]]]
    assert en.to_rgb8(p[..., 0], en.MONO8).tolist() == [[[10, 10, 10]]]
    # alpha is carried but never read back
    a = en.encode(rgb, en.BGRA8)
    assert len(np.unique(a[..., 3])) > 1
    b = a.copy()
    b[..., 3] ^= 0xFF
    assert np.array_equal(en.to_rgb8(a, en.BGRA8), en.to_rgb8(b, en.BGRA8))
    buf = en.padded(en.encode(rgb, en.RGBA8), 8)
    assert buf.shape == (7, 13 * 4 + 8) and (buf[:, 52:] == 0xA5).all()


def test_ros_node_with_the_in_place_path_compiles_against_the_stubs():
    """The node reads a message's payload in place when ugsm_input_format_from_encoding knows its encoding (no cv_bridge copy) and falls back
    to toCvCopy(RGB8) otherwise; the stubs are unchanged (they declare enc::RGB8 only: the string table is the library's)."""
    node = open(os.path.join(ROOT, "ros", "UG_GPU_matcher_ugsm.cpp")).read()
    shim = open(os.path.join(ROOT, "ros", "MatchGPULib_ugsm.hpp")).read()
    assert "ugsm_input_format_from_encoding" in node and "toCvCopy" in node
    assert "setInputFormat" in shim and "ugsm_set_input_format" in shim
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    r = subprocess.run([gxx, "-std=c++14", "-fsyntax-only", "-Itests/ros_stubs", "-Iros", "-Iinclude", "ros/UG_GPU_matcher_ugsm.cpp"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
