"""The checked full-mode call (ugsm_submit_full_checked, ugsm_match_full_checked, ugsm_last_lr_marked_pair) without a GPU: the three names are
declared in a header that is plain C99, exported by both libraries through ugsm.map and bound; the Python binding marshals its lists; a null
context is a status code; the shims and the documents carry the call."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

NAMES = ("ugsm_submit_full_checked", "ugsm_match_full_checked", "ugsm_last_lr_marked_pair")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_the_header_is_plain_c99_with_the_three_names(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ugsm.h"
    src = tmp_path / "use.c"
    src.write_text('#include "ugsm.h"\n'
                   "int use(ugsm_ctx *c, const uint8_t *const *l, float *const *o, const uint8_t *h, float *p, long long *m)\n"
                   "{\n"
                   "    return ugsm_submit_full_checked(c, 0, 1, l, l, 64, 48, 192, o, 0, 1.0f) + ugsm_match_full_checked(c, h, h, 64, 48, 192, p, p, p, 0, 0, 0, 1.0f)\n"
                   "           + ugsm_last_lr_marked_pair(c, 0, 0, m, m);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert re.search(r"#define UGSM_ABI_VERSION 6\b", hdr), "additions only: the ABI number stays"
    # tau is the last argument of the two calls, a float
    for name in NAMES[:2]:
        proto = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert re.search(r",\s*float tau\s*$", proto), proto
    said = hdr.split("int ugsm_submit_full_checked(")[0].rsplit("NOT built:", 1)[1]
    assert "queue form" in said and "page-locked _host kind" in said


def test_both_libraries_export_them_through_the_map(lib):
    script = open(os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm.map")).read()
    assert re.search(r"global:\s*ugsm_\*;", script) and re.search(r"local:\s*\*;", script)
    for name in NAMES:
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
            assert hasattr(C.CDLL(path), name), f"{os.path.basename(path)} does not export {name}"
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(rf" T {name}$", dyn, re.M), f"{name} is not a dynamic symbol of {os.path.basename(path)}"
    so = lib.load()
    assert so.ugsm_abi_version() == 6
    assert so.ugsm_submit_full_checked.argtypes[-1] is C.c_float and so.ugsm_match_full_checked.argtypes[-1] is C.c_float
    assert len(so.ugsm_submit_full_checked.argtypes) == 11 and len(so.ugsm_match_full_checked.argtypes) == 13


@pytest.mark.parametrize("tau", [1.0, 0.0, float("nan")])
@pytest.mark.parametrize("n", [1, 0, 17])
def test_a_null_context_is_a_status_code_whatever_else_is_wrong(lib, tau, n):
    for dev in (False, True):
        so = lib.load(dev)
        ptrs = (C.c_void_p * 1)(None)
        assert so.ugsm_submit_full_checked(None, 0, n, ptrs, ptrs, 64, 48, 192, ptrs, None, tau) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_match_full_checked(None, None, None, 64, 48, 192, None, None, None, None, None, None, tau) == lib.UGSM_ERR_BAD_ARG
        f, b = C.c_longlong(-5), C.c_longlong(-5)
        assert so.ugsm_last_lr_marked_pair(None, 0, 0, C.byref(f), C.byref(b)) == lib.UGSM_ERR_BAD_ARG
        assert (f.value, b.value) == (-5, -5)


class _FakeLib:
    """Stands in for the loaded library: records what Context.submit_full_checked hands to the C call."""

    def __init__(self):
        self.calls = []

    def ugsm_submit_full_checked(self, *args):
        self.calls.append(args)
        return 0

    def ugsm_last_lr_marked_pair(self, h, slot, pair, f, b):
        f._obj.value, b._obj.value = 11 + pair, 22 + pair
        return 0


def test_the_python_binding_marshals_its_lists(lib):
    c = object.__new__(lib.Context)
    c._h, c.lib = 1234, _FakeLib()
    c.submit_full_checked(1, [10, 20, 30], [11, 21, 31], 64, 48, 192, [12, 22, 32], [13, None, 33], 0.5)
    c.submit_full_checked(0, [10], [11], 64, 48, 200, [12], None, 2.0)
    (h, slot, n, dl, dr, W, H, stride, do, db, tau), second = c.lib.calls
    assert (h, slot, n, W, H, stride, tau) == (1234, 1, 3, 64, 48, 192, 0.5)
    assert list(dl) == [10, 20, 30] and list(dr) == [11, 21, 31] and list(do) == [12, 22, 32] and list(db) == [13, None, 33]
    assert second[2] == 1 and second[9] is None and second[7] == 200 and second[10] == 2.0
    with pytest.raises(lib.UgsmError):
        c.submit_full_checked(0, [10, 20], [11], 64, 48, 192, [12, 22], None, 1.0)
    with pytest.raises(lib.UgsmError):
        c.submit_full_checked(0, [10, 20], [11, 21], 64, 48, 192, [12, 22], [13], 1.0)
    assert len(c.lib.calls) == 2
    assert c.last_lr_marked_pair(0, 2) == (13, 24)


def test_the_python_mirror_and_the_shims_expose_the_call(lib):
    for method in ("submit_full_checked", "match_full_checked", "last_lr_marked_pair"):
        assert hasattr(lib.Context, method), method
    assert list(inspect.signature(lib.Context.submit_full_checked).parameters)[-2:] == ["d_back", "tau"]
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    assert inspect.signature(MatchGPULib.match).parameters["tau"].default is None
    shim = open(os.path.join(ROOT, "ros", "MatchGPULib_ugsm.hpp")).read()
    assert "float **match(ImgPtr L, ImgPtr R, int fov, float tau, float ***back = nullptr)" in shim and "ugsm_match_full_checked(ctx_," in shim
    node = open(os.path.join(ROOT, "ros", "UG_GPU_matcher_ugsm.cpp")).read()
    assert node.count("mgpu_->match(L, R, fov, lr_check_tau())") == 2
    assert "m.match(L, R, 0, 1.0f, &bk)" in open(os.path.join(ROOT, "ros", "shim_selftest.cpp")).read()


def test_the_shim_selftest_compiles_against_the_header(lib, tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "ros", "shim_selftest.cpp"),
                           "-o", str(tmp_path / "shim_selftest.o")])


def test_the_documents_carry_the_call():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text, what in ((integ, "INTEGRATION.md"), (design, "DESIGN.md"), (readme, "README.md")):
        assert "ugsm_submit_full_checked" in text, what
    assert "ugsm_last_lr_marked_pair" in integ
    assert "lr_full_bench.json" in design
