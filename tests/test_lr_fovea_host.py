"""The LR check of the foveated calls, without a GPU: the entry points exist in both libraries and in the bindings, answer a null context
with a status code, and the header, the bindings and the node's shim agree on the mode bits."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NAMES = ("ugsm_set_lr_check", "ugsm_get_lr_check", "ugsm_last_lr_marked_levels")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_entry_points_are_exported_and_bound(lib):
    for dev in (False, True):
        so = lib.load(dev=dev)
        for name in NAMES:
            assert name in lib.EXPORTS and hasattr(so, name), name
        assert so.ugsm_abi_version() == 6                       # additions only
    for method in ("set_lr_check", "lr_check", "last_lr_marked", "last_lr_marked_levels"):
        assert hasattr(lib.Context, method), method


def test_null_context_answers(lib):
    so = lib.load()
    tau, modes = C.c_float(-3.0), C.c_int(-3)
    assert so.ugsm_set_lr_check(None, 1.0, lib.UGSM_LR_FOVEATED) == lib.UGSM_ERR_BAD_ARG
    assert so.ugsm_get_lr_check(None, C.byref(tau), C.byref(modes)) == lib.UGSM_ERR_BAD_ARG
    assert (tau.value, modes.value) == (-3.0, -3)               # nothing written
    per = (C.c_longlong * lib.UGSM_MAX_LEVELS)(*([-7] * lib.UGSM_MAX_LEVELS))
    assert so.ugsm_last_lr_marked_levels(None, 0, 0, per) == lib.UGSM_ERR_BAD_ARG
    assert list(per) == [-7] * lib.UGSM_MAX_LEVELS
    assert so.ugsm_last_lr_marked(None, 0) == -1


def test_header_bindings_and_shim_agree_on_the_mode_bits(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    bits = {k: int(v) for k, v in re.findall(r"^#define (UGSM_LR_[A-Z]+)\s+(\d+)", hdr, re.M)}
    assert bits == {"UGSM_LR_FULL": lib.UGSM_LR_FULL, "UGSM_LR_FOVEATED": lib.UGSM_LR_FOVEATED} == {"UGSM_LR_FULL": 1, "UGSM_LR_FOVEATED": 2}
    # the calls the header leaves unchecked are named there
    for name in ("ugsm_submit_fovea_coarse", "ugsm_submit_fovea_shard", "ugsm_stage_"):
        assert name in hdr.split("NOT checked, whatever the setting:")[1].split("*/")[0], name
    shim = open(os.path.join(ROOT, "ros", "MatchGPULib_ugsm.hpp")).read()
    assert '"-lrmodes="' in shim and "setLRCheck(float tau, int modes)" in shim and "ugsm_set_lr_check(ctx_, tau, modes)" in shim


def test_the_queue_and_the_kernel_set_are_as_before(lib):
    """The queue reaches the check through the batch calls: ugsm_queue.cpp names nothing of it (and so keeps linking against the tests' fake
    runtime); the check's stack form is a form of k_lr_check, not a kernel of another name."""
    q = open(os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm_queue.cpp")).read()
    assert "lr_check" not in q and "lr_marked" not in q
    aux = open(os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm_kernels_aux.hip")).read()
    assert len(re.findall(r"__global__[^\n]*\bvoid k_lr_check\(", aux)) == 2
    blob = open(lib.LIB_PATH, "rb").read()
    forms = set(re.findall(rb"_ZN4ugsm10k_lr_check[A-Za-z0-9_]*", blob))
    assert len(forms) == 2, forms
