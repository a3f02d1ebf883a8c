"""The depth image of the whole frame from a fovea stack (ugsm_depth_image_fovea_full, ugsm_depth_image_fovea_multi,
ugsm_match_foveated_depth) without a GPU: declarations, exports and bindings, the refusal of calls without a context, the header as plain C99
with the three names, and the shim's depthImageFrame.  The refusals one by one on a live context: tests/test_gpu_depth_frame.py, which
shares the cases below."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CALLS = ["ugsm_depth_image_fovea_full", "ugsm_depth_image_fovea_multi", "ugsm_match_foveated_depth"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_the_three_names_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in CALLS:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in CALLS:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    so = lib.load()
    assert so.ugsm_abi_version() == 6
    for name, nargs in zip(CALLS, (14, 13, 15)):
        assert len(getattr(so, name).argtypes) == nargs, name
    for method in ("depth_image_fovea_full", "depth_image_fovea_multi", "match_foveated_depth"):
        assert callable(getattr(lib.Context, method)), method
    from ug_stereomatcher_amd import MatchGPULib
    assert callable(MatchGPULib.depthImageFrame)
    # the section says what the calls are and what stays out of scope
    for word in ("byte for byte", "HIGHEST-numbered", "conf * s^depth", "The full-resolution field is never formed", "queue forms", "a strided output",
                 "depth in the right camera"):
        assert word in hdr, word
    assert "compose\n * ugsm_reconstruct_full[_multi] with ugsm_depth_image)" not in hdr


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------

def call(lib, name, **over):
    """One call of entry point `name`; without overrides: plausible (fake, never dereferenced) device pointers and no context.  stacks: the
    multi form's device stacks (n: their number unless given; stack1_shift: bytes added to the second entry)."""
    P = (C.c_double * 12)(*np.eye(3, 4).reshape(12))
    a = dict(ctx=None, slot=0, dx=0x100000, dy=0x200000, conf=0x300000, W=64, H=48, P1=P, P2=P, p=lib.depth_params(), depth=0x400000, valid=0x500000,
             off=(0, 0), offs=None, stacks=[0x100000, 0x800000, 0xA00000], n=None, stack1_shift=0, L=0x600000, R=0x700000, stride=192,
             planes=(None, None, None))
    a.update(over)
    p = C.byref(a["p"]) if a["p"] is not None else None
    so = lib.load()
    if name == "ugsm_depth_image_fovea_full":
        return so.ugsm_depth_image_fovea_full(a["ctx"], a["slot"], a["dx"], a["dy"], a["conf"], a["W"], a["H"], a["off"][0], a["off"][1], a["P1"], a["P2"],
                                              p, a["depth"], a["valid"])
    if name == "ugsm_depth_image_fovea_multi":
        st = a["stacks"]
        arr = None
        if st is not None:
            st = [(q + a["stack1_shift"] if k == 1 and q is not None else q) for k, q in enumerate(st)]
            arr = (C.c_void_p * max(len(st), 1))(*st)
        n = a["n"] if a["n"] is not None else (len(st) if st is not None else 3)
        ox = oy = None
        if a["offs"] is not None:
            ox, oy = (C.c_int * len(a["offs"]))(*[o[0] for o in a["offs"]]), (C.c_int * len(a["offs"]))(*[o[1] for o in a["offs"]])
        return so.ugsm_depth_image_fovea_multi(a["ctx"], a["slot"], n, arr, a["W"], a["H"], ox, oy, a["P1"], a["P2"], p, a["depth"], a["valid"])
    return so.ugsm_match_foveated_depth(a["ctx"], a["L"], a["R"], a["W"], a["H"], a["stride"], a["off"][0], a["off"][1], a["P1"], a["P2"], p, a["depth"],
                                        *a["planes"])


def bad_argument_cases(lib, name):
    """Every argument refusal of entry point `name` (label, overrides); a case names a buffer by its key and a byte offset, which the GPU test
    resolves inside its real buffers.  The first block is what ugsm_depth_image refuses (tests/test_depth_host.py)."""
    nan, inf = float("nan"), float("inf")
    dp = lib.depth_params
    cases = [("no P1", dict(P1=None)), ("no P2", dict(P2=None)), ("no params", dict(p=None)), ("no depth", dict(depth=None)),
             ("format 2", dict(p=dp(format=2))), ("format -1", dict(p=dp(format=-1))),
             ("unit 0", dict(p=dp(unit=0.0))), ("unit < 0", dict(p=dp(unit=-1.0))), ("unit NaN", dict(p=dp(unit=nan))), ("unit inf", dict(p=dp(unit=inf))),
             ("factor 0", dict(p=dp(factor=0.0))), ("factor < 0", dict(p=dp(factor=-0.5))), ("factor > 1", dict(p=dp(factor=1.25))),
             ("factor NaN", dict(p=dp(factor=nan))), ("factor inf", dict(p=dp(factor=inf))), ("factor leaves a side 0", dict(p=dp(factor=1e-3))),
             ("W 0", dict(W=0)), ("H 0", dict(H=0)), ("W < 0", dict(W=-3)), ("above 2^28 pixels", dict(W=1 << 15, H=(1 << 13) + 1))]
    if name == "ugsm_match_foveated_depth":
        return cases
    cases += [("slot -1", dict(slot=-1)), ("slot 99", dict(slot=99)),
              ("min_conf NaN", dict(p=dp(min_conf=nan))), ("z_min NaN", dict(p=dp(z_min=nan))), ("z_max NaN", dict(p=dp(z_max=nan))),
              ("z_min > z_max", dict(p=dp(z_min=2.0, z_max=1.0))),
              ("depth misaligned 32F", dict(depth=("depth", 2))), ("depth misaligned 16U", dict(depth=("depth", 1), p=dp(format=1))),
              ("valid misaligned", dict(valid=("valid", 4))),
              ("depth is dx", dict(depth=("dx", 0))), ("depth inside dy", dict(depth=("dy", 8))), ("depth is conf", dict(depth=("conf", 0))),
              ("depth ends inside dx", dict(depth=("dx", -16)))]
    if name == "ugsm_depth_image_fovea_full":
        cases += [("no dx", dict(dx=None)), ("no dy", dict(dy=None)), ("conf NULL, min_conf finite", dict(conf=None, p=dp(min_conf=0.5))),
                  ("dx misaligned", dict(dx=("dx", 2))), ("conf misaligned", dict(conf=("conf", 1)))]
    else:
        cases += [("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("n 17", dict(n=17)), ("no stacks", dict(stacks=None)),
                  ("a null stack entry", dict(stacks=[0x100000, None, 0xA00000])), ("a null first entry", dict(stacks=[None, 0x800000])),
                  ("a misaligned stack", dict(stack1_shift=2)),
                  ("depth is stack 1", dict(depth=("stack1", 0))), ("depth inside stack 2", dict(depth=("stack2", 64))),
                  ("depth ends inside stack 2", dict(depth=("stack2", -16)))]
    return cases


def resolve(over, bufs):
    """The overrides of a case with its (buffer key, byte offset) pairs turned into addresses inside `bufs`; a list of stacks with fake
    entries takes the real ones in their place."""
    out = {}
    for k, v in over.items():
        if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], str):
            v = bufs[v[0]] + v[1]
        elif k == "stacks" and v is not None and "stack1" in bufs:
            real = [bufs["dx"], bufs["stack1"], bufs["stack2"]]
            v = [None if q is None else real[j] for j, q in enumerate(v)]
        out[k] = v
    return out


@pytest.mark.parametrize("name", CALLS)
def test_null_context_and_bad_arguments_are_refused_without_a_device(lib, name):
    """Without a device there is no context, so every call here is refused for its null context, whatever else it carries: the entry point
    takes the argument list and answers with a status code before it touches anything."""
    fake = dict(dx=0x100000, dy=0x200000, conf=0x300000, depth=0x400000, valid=0x500000, stack1=0x800000, stack2=0xA00000)
    fake_only = {k: v for k, v in fake.items() if not k.startswith("stack")}
    assert call(lib, name) == lib.UGSM_ERR_BAD_ARG
    for label, over in bad_argument_cases(lib, name):
        assert call(lib, name, **resolve(over, dict(fake_only, **{k: fake[k] for k in ("stack1", "stack2")}))) == lib.UGSM_ERR_BAD_ARG, label


def test_the_header_is_plain_c99_with_the_three_names(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "ugsm.h"\n'
                   "int use(ugsm_ctx *c, const float *const *st, const float *s, const double *P, void *img, unsigned long long *n,\n"
                   "        const uint8_t *L, float *out)\n"
                   "{\n"
                   "    ugsm_depth_params p;\n"
                   "    ugsm_default_depth_params(&p);\n"
                   "    p.format = UGSM_DEPTH_16U;\n"
                   "    if (ugsm_depth_image_fovea_full(c, 0, s, s, s, 640, 480, 3, -2, P, P, &p, img, n) != UGSM_OK) return 1;\n"
                   "    if (ugsm_depth_image_fovea_multi(c, 0, 3, st, 640, 480, 0, 0, P, P, &p, img, n) != UGSM_OK) return 2;\n"
                   "    return ugsm_match_foveated_depth(c, L, L, 640, 480, 1920, 0, 0, P, P, &p, img, out, 0, 0);\n"
                   "}\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_shim_declares_depth_image_frame(tmp_path):
    """ros/MatchGPULib_ugsm.hpp: depthImageFrame on a pair of image pointers compiles against the declaration stubs, and depthImageStack keeps
    its per-level signature."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "depth_frame.cpp"
    src.write_text('#include <cv_bridge/cv_bridge.h>\n#include "MatchGPULib_ugsm.hpp"\n'
                   "void *frame(MatchGPULib &m, cv_bridge::CvImagePtr L, cv_bridge::CvImagePtr R, const double *P1, const double *P2)\n"
                   "{\n"
                   "    ugsm_depth_params p;\n"
                   "    ugsm_default_depth_params(&p);\n"
                   "    p.format = UGSM_DEPTH_16U;\n"
                   "    int dw, dh;\n"
                   "    void *a = m.depthImageFrame(L, R, P1, P2, &p, &dw, &dh);\n"
                   "    std::free(a);\n"
                   "    return m.depthImageFrame(L, R, P1, P2, &p, &dw, &dh, 13, -9);\n"
                   "}\n"
                   "void *levels(MatchGPULib &m, float ***stack, const double *P1, const double *P2, unsigned long long *valid)\n"
                   "{\n"
                   "    ugsm_depth_params p;\n"
                   "    ugsm_default_depth_params(&p);\n"
                   "    int dw, dh;\n"
                   "    return m.depthImageStack(stack, 640, 480, P1, P2, &p, &dw, &dh, valid);\n"
                   "}\n")
    r = subprocess.run([gxx, "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-Itests/ros_stubs", "-Iros", "-Iinclude", str(src)], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
