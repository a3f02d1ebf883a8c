"""The checked multi-window call (ugsm_submit_foveated_multi_checked, ugsm_match_foveated_multi_checked) without a GPU: the two names are
declared, listed, exported by both libraries and bound; the refusals that need no device are status codes; the Python mirror and the shims
expose the call; and the documents no longer list it as not built."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT

NAMES = ("ugsm_submit_foveated_multi_checked", "ugsm_match_foveated_multi_checked")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_the_two_entry_points_are_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ugsm.h"
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
            assert hasattr(C.CDLL(path), name), f"{os.path.basename(path)} does not export {name}"
    assert lib.load().ugsm_abi_version() == 6        # additions: the ABI number stays
    # tau is the last argument of both, a float
    for name in NAMES:
        proto = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert re.search(r",\s*float tau\s*$", proto), proto
        assert getattr(lib.load(), name).argtypes[-1] is C.c_float


@pytest.mark.parametrize("tau", [1.0, 0.0, -1.0, float("nan")])
@pytest.mark.parametrize("n", [1, 0, -3, 17])
def test_a_null_context_is_a_status_code_whatever_else_is_wrong(lib, tau, n):
    for dev in (False, True):
        so = lib.load(dev)
        ptrs = (C.c_void_p * 1)(None)
        assert so.ugsm_submit_foveated_multi_checked(None, 0, None, None, 64, 48, 192, n, None, None, ptrs, tau) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_match_foveated_multi_checked(None, None, None, 64, 48, 192, n, None, None, ptrs, ptrs, ptrs, tau) == lib.UGSM_ERR_BAD_ARG


def test_the_python_mirror_and_the_shims_expose_the_call(lib):
    for method in ("submit_foveated_multi_checked", "match_foveated_multi_checked"):
        assert hasattr(lib.Context, method), method
    assert list(inspect.signature(lib.Context.submit_foveated_multi_checked).parameters)[-1] == "tau"
    assert inspect.signature(lib.Context.match_foveated_multi).parameters["tau"].default is None
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    assert inspect.signature(MatchGPULib.matchStackMulti).parameters["tau"].default is None
    shim = open(os.path.join(ROOT, "ros", "MatchGPULib_ugsm.hpp")).read()
    assert "float ****out, float tau = 0.0f)" in shim and "ugsm_match_foveated_multi_checked(ctx_," in shim


def test_the_documents_no_longer_list_the_call_as_not_built():
    """... and still list the queue form, the page-locked form, the pyramid stacks and the resized cloud of several stacks."""
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (hdr, integ, design):
        for sentence in re.findall(r"N(?:OT|ot) built:[^.]*\.", text):
            assert "LR check" not in sentence, sentence
    plain = hdr.split("int ugsm_submit_foveated_multi(")[0].rsplit("NOT built:", 1)[1]
    for what in ("pyramid stacks", "queue form", "page-locked _host kind"):
        assert what in plain, what
    cloud = hdr.split("long long ugsm_fovea_multi_cloud_points(")[0].rsplit("NOT built:", 1)[1]
    assert "queue or managed form" in cloud and "resized cloud of several stacks" in cloud
    assert "The checked multi-window call" in design and "ugsm_submit_foveated_multi_checked" in integ
    assert "ugsm_submit_foveated_multi_checked" in open(os.path.join(ROOT, "README.md")).read()
