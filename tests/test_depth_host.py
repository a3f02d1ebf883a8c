"""The depth image (ugsm_depth_image, ugsm_depth_image_fovea, ugsm_match_full_depth; REP 118 32FC1 / 16UC1) without a GPU: declarations and
exports, the host-only size rule and default parameters, the refusal of calls without a context, and the known answers of the numpy
restatement (tests/depth_np.py) that the GPU tests compare against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import depth_np as dn
import resize_np as rn
from conftest import ROOT

NEW = ["ugsm_default_depth_params", "ugsm_depth_image_size", "ugsm_depth_image", "ugsm_depth_image_fovea", "ugsm_match_full_depth"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_depth_symbols_are_declared_and_exported_by_both_libraries(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().ugsm_abi_version() == 6
    assert (lib.UGSM_DEPTH_32F, lib.UGSM_DEPTH_16U, lib.UGSM_DEPTH_ALL_LEVELS) == (0, 1, -1)
    for macro in ("#define UGSM_DEPTH_32F 0", "#define UGSM_DEPTH_16U 1", "#define UGSM_DEPTH_ALL_LEVELS (-1)"):
        assert macro in hdr
    for word in ("queue forms", "a strided output", "depth in the right camera", "camera_info", "undistortion"):   # the out-of-scope list is stated
        assert word in hdr, word


def test_default_parameters(lib):
    p = lib.depth_params()
    assert (p.format, p.unit, p.min_conf, p.z_min, p.z_max, p.factor) == (lib.UGSM_DEPTH_32F, 1.0, -np.inf, -np.inf, np.inf, 1.0)
    assert C.sizeof(lib.DepthParams) == 24
    lib.load().ugsm_default_depth_params(None)           # (a null pointer is ignored)
    q = lib.depth_params(format=lib.UGSM_DEPTH_16U, unit=0.5, min_conf=0.25, z_min=1.0, z_max=9.0, factor=0.5)
    assert (q.format, q.unit, q.min_conf, q.z_min, q.z_max, q.factor) == (1, 0.5, 0.25, 1.0, 9.0, 0.5)


def test_image_size_is_the_resized_clouds_rule(lib):
    for W, H in [(1, 1), (8, 3), (67, 41), (255, 2), (64, 48), (4928, 3264), (1920, 1080), (615, 407), (7, 5)]:
        for f in (1.0, 0.2, 0.3, 1 / 3, 0.5, 0.7, 0.99, 1e-3):
            dw, dh = rn.resized_size(W, H, f)
            got = lib.depth_image_size(W, H, f)
            if min(dw, dh) < 1:
                assert got is None and lib.resized_cloud_points(W, H, f) == -1, (W, H, f)
            else:
                assert got == (dw, dh) and dw * dh == lib.resized_cloud_points(W, H, f), (W, H, f)
        assert lib.depth_image_size(W, H, 1.0) == (W, H)
    so = lib.load()
    w, h = C.c_int(-5), C.c_int(-5)
    for pw, ph, f in [(0, 4, 1.0), (4, 0, 1.0), (-1, 4, 1.0), (4, 4, 0.0), (4, 4, -0.5), (4, 4, 1.5), (4, 4, np.nan), (4, 4, np.inf), (4, 4, 0.2)]:
        assert so.ugsm_depth_image_size(pw, ph, C.c_float(f), C.byref(w), C.byref(h)) == lib.UGSM_ERR_BAD_ARG, (pw, ph, f)
        assert (w.value, h.value) == (-5, -5)           # (a refused call writes nothing)
    assert so.ugsm_depth_image_size(4, 4, C.c_float(1.0), None, C.byref(h)) == lib.UGSM_ERR_BAD_ARG
    assert so.ugsm_depth_image_size(4, 4, C.c_float(1.0), C.byref(w), None) == lib.UGSM_ERR_BAD_ARG


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------

def call(lib, name, **over):
    """One call of entry point `name`; without overrides: plausible (fake, never dereferenced) device pointers and no context."""
    P = (C.c_double * 12)(*np.eye(3, 4).reshape(12))
    a = dict(ctx=None, slot=0, dx=0x100000, dy=0x200000, conf=0x300000, W=64, H=48, P1=P, P2=P, p=lib.depth_params(), depth=0x400000, valid=0x500000,
             off=(0, 0), level=0, L=0x600000, R=0x700000, stride=192, planes=(None, None, None))
    a.update(over)
    p = C.byref(a["p"]) if a["p"] is not None else None
    so = lib.load()
    if name == "ugsm_depth_image":
        return so.ugsm_depth_image(a["ctx"], a["slot"], a["dx"], a["dy"], a["conf"], a["W"], a["H"], a["P1"], a["P2"], p, a["depth"], a["valid"])
    if name == "ugsm_depth_image_fovea":
        return so.ugsm_depth_image_fovea(a["ctx"], a["slot"], a["dx"], a["dy"], a["conf"], a["W"], a["H"], a["off"][0], a["off"][1], a["level"],
                                         a["P1"], a["P2"], p, a["depth"], a["valid"])
    return so.ugsm_match_full_depth(a["ctx"], a["L"], a["R"], a["W"], a["H"], a["stride"], a["P1"], a["P2"], p, a["depth"], *a["planes"])


def bad_argument_cases(lib, name):
    """Every argument refusal of entry point `name` (label, overrides); shared with the GPU test, which makes them on a live context with
    real buffers in the place of dx / dy / conf / depth / valid (a case names a buffer by its key: the test offsets the real pointer)."""
    nan, inf = float("nan"), float("inf")
    dp = lib.depth_params
    cases = [("no P1", dict(P1=None)), ("no P2", dict(P2=None)), ("no params", dict(p=None)), ("no depth", dict(depth=None)),
             ("format 2", dict(p=dp(format=2))), ("format -1", dict(p=dp(format=-1))),
             ("unit 0", dict(p=dp(unit=0.0))), ("unit < 0", dict(p=dp(unit=-1.0))), ("unit NaN", dict(p=dp(unit=nan))), ("unit inf", dict(p=dp(unit=inf))),
             ("factor 0", dict(p=dp(factor=0.0))), ("factor < 0", dict(p=dp(factor=-0.5))), ("factor > 1", dict(p=dp(factor=1.25))),
             ("factor NaN", dict(p=dp(factor=nan))), ("factor inf", dict(p=dp(factor=inf))), ("factor leaves a side 0", dict(p=dp(factor=1e-3))),
             ("W 0", dict(W=0)), ("H 0", dict(H=0)), ("W < 0", dict(W=-3)), ("above 2^28 pixels", dict(W=1 << 15, H=(1 << 13) + 1))]
    if name != "ugsm_match_full_depth":
        cases += [("no dx", dict(dx=None)), ("no dy", dict(dy=None)), ("slot -1", dict(slot=-1)), ("slot 99", dict(slot=99)),
                  ("min_conf NaN", dict(p=dp(min_conf=nan))), ("z_min NaN", dict(p=dp(z_min=nan))), ("z_max NaN", dict(p=dp(z_max=nan))),
                  ("z_min > z_max", dict(p=dp(z_min=2.0, z_max=1.0))), ("conf NULL, min_conf finite", dict(conf=None, p=dp(min_conf=0.5))),
                  ("depth misaligned 32F", dict(depth=("depth", 2))), ("depth misaligned 16U", dict(depth=("depth", 1), p=dp(format=1))),
                  ("valid misaligned", dict(valid=("valid", 4))), ("dx misaligned", dict(dx=("dx", 2))), ("conf misaligned", dict(conf=("conf", 1))),
                  ("depth is dx", dict(depth=("dx", 0))), ("depth inside dy", dict(depth=("dy", 8))), ("depth is conf", dict(depth=("conf", 0))),
                  ("depth ends inside dx", dict(depth=("dx", -16)))]
    if name == "ugsm_depth_image_fovea":
        cases += [("level -2", dict(level=-2)), ("level F", dict(level=7)), ("level 99", dict(level=99))]
    return cases


def resolve(over, bufs):
    """The overrides of a case with its (buffer key, byte offset) pairs turned into addresses inside `bufs`."""
    return {k: (bufs[v[0]] + v[1] if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], str) else v) for k, v in over.items()}


@pytest.mark.parametrize("name", ["ugsm_depth_image", "ugsm_depth_image_fovea", "ugsm_match_full_depth"])
def test_null_context_and_bad_arguments_are_refused_without_a_device(lib, name):
    """Without a device there is no context, so every call here is refused for its null context, whatever else it carries: the entry point
    takes the argument list and answers with a status code before it touches anything.  Each check on its own: tests/test_gpu_depth.py, on
    a live context."""
    fake = dict(dx=0x100000, dy=0x200000, conf=0x300000, depth=0x400000, valid=0x500000)
    assert call(lib, name) == lib.UGSM_ERR_BAD_ARG
    for label, over in bad_argument_cases(lib, name):
        assert call(lib, name, **resolve(over, fake)) == lib.UGSM_ERR_BAD_ARG, label


def test_shim_declares_depth_image_and_depth_image_stack(tmp_path):
    """ros/MatchGPULib_ugsm.hpp: depthImage on a pair of image pointers and depthImageStack on matchStack's stacks compile against the
    declaration stubs (a syntax / interface check, as the node's)."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "depth_image.cpp"
    src.write_text('#include <cv_bridge/cv_bridge.h>\n#include "MatchGPULib_ugsm.hpp"\n'
                   "void *one(MatchGPULib &m, cv_bridge::CvImagePtr L, cv_bridge::CvImagePtr R, const double *P1, const double *P2, float ***fin)\n"
                   "{\n"
                   "    ugsm_depth_params p;\n"
                   "    ugsm_default_depth_params(&p);\n"
                   "    p.format = UGSM_DEPTH_16U;\n"
                   "    int dw, dh;\n"
                   "    void *a = m.depthImage(L, R, P1, P2, &p, &dw, &dh);\n"
                   "    std::free(a);\n"
                   "    return m.depthImage(L, R, P1, P2, &p, &dw, &dh, fin);\n"
                   "}\n"
                   "void *all(MatchGPULib &m, float ***stack, const double *P1, const double *P2, unsigned long long *valid)\n"
                   "{\n"
                   "    ugsm_depth_params p;\n"
                   "    ugsm_default_depth_params(&p);\n"
                   "    int dw, dh;\n"
                   "    return m.depthImageStack(stack, 640, 480, P1, P2, &p, &dw, &dh, valid);\n"
                   "}\n")
    r = subprocess.run([gxx, "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-Itests/ros_stubs", "-Iros", "-Iinclude", str(src)], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the restatement's known answers -----------------------------------------------------------------------------------------------------

def test_restatement_known_answers_16u():
    z = np.array([[1.0, 65.5354, 65.5356, 0.0004, np.nan, np.inf, -np.inf, -1.0, 0.0, 2.5]], np.float32)
    img, valid = dn.convert(z, dn.FMT_16U)
    assert img.dtype == np.uint16 and img.tolist() == [[1000, 65535, 0, 0, 0, 0, 0, 0, 0, 2500]]
    assert valid.tolist() == [[True, True, False, False, False, False, False, False, False, True]]
    # the unit scales before the millimetres: Z in centimetres
    img, _ = dn.convert(np.array([[100.0, 250.0]], np.float32), dn.FMT_16U, unit=0.01)
    assert img.tolist() == [[1000, 2500]]
    # rounding is (m * 1000 + 0.5) truncated: 1.0004 -> 1000, 1.0006 -> 1001
    assert dn.convert(np.array([[1.0004, 1.0006]], np.float32), dn.FMT_16U)[0].tolist() == [[1000, 1001]]


def test_restatement_known_answers_32f():
    z = np.array([[1.0, -0.0, np.nan, np.inf, -np.inf, 3e38, 1e-40]], np.float32)
    img, valid = dn.convert(z, dn.FMT_32F)
    assert img.dtype == np.float32
    assert img.view(np.uint32).tolist() == [[0x3F800000, 0x80000000, 0x7FC00000, 0x7FC00000, 0x7FC00000, z.view(np.uint32)[0, 5], z.view(np.uint32)[0, 6]]]
    assert valid.tolist() == [[True, True, False, False, False, True, True]]
    # any NaN in, the one quiet NaN out
    odd = np.array([[0xFFC12345, 0x7F800001]], np.uint32).view(np.float32)
    assert dn.convert(odd)[0].view(np.uint32).tolist() == [[0x7FC00000, 0x7FC00000]]
    # the window is on Z itself, before the unit; the confidence test fails a NaN and, without a plane, is no test
    z = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    conf = np.array([[0.9, np.nan, 0.1, 0.5]], np.float32)
    img, valid = dn.convert(z, unit=10.0, z_min=2.0, z_max=4.0, conf=conf, min_conf=0.5)
    assert valid.tolist() == [[False, False, False, True]] and img[0, 3] == 40.0 and np.isnan(img[0, :3]).all()
    assert dn.convert(z, conf=conf)[1].tolist() == [[True, False, True, True]]         # (-inf threshold: only the NaN fails)
    assert dn.convert(z)[1].all()


def test_restatement_resized_image_reads_the_confidence_at_the_registered_pixel():
    rng = np.random.Generator(np.random.PCG64(5))
    z = rng.uniform(1, 5, (41, 67)).astype(np.float32)
    conf = rng.uniform(0, 1, (41, 67)).astype(np.float32)
    for f in (0.2, 0.5):
        img, valid = dn.depth_of_z(z, conf=conf, factor=f, min_conf=0.5)
        dw, dh = rn.resized_size(67, 41, f)
        assert img.shape == (dh, dw)
        xs, ys = rn.sample_at(67, f), rn.sample_at(41, f)
        assert np.array_equal(valid, conf[np.ix_(ys, xs)] >= 0.5)
        assert np.array_equal(img[valid], rn.resize_cubic(z, dw, dh)[valid])
    img, valid = dn.depth_of_z(z, factor=1.0)
    assert valid.all() and np.array_equal(img, z)
