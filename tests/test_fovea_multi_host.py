"""Several fovea windows on one pair (ugsm_submit_foveated_multi, ugsm_match_foveated_multi, ugsm_reconstruct_full_multi) without a GPU:
the three names are declared, listed and exported; a NULL context is a status code; and the NumPy restatement of the reconstruction
(tests/reconstruct_multi_np.py), which the GPU tests compare the device against, equals the CPU oracle's hierarchicalDisparity for one window
bit for bit -- NaN and inf included."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reconstruct_multi_np as rm
from conftest import ROOT, assert_bit_equal

NAMES = ("ugsm_submit_foveated_multi", "ugsm_match_foveated_multi", "ugsm_reconstruct_full_multi")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_the_three_entry_points_are_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ugsm.h"
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
            assert hasattr(C.CDLL(path), name), f"{os.path.basename(path)} does not export {name}"
    assert lib.load().ugsm_abi_version() == 6        # additions: the ABI number stays


def test_a_null_context_is_a_status_code(lib):
    for dev in (False, True):
        so = lib.load(dev)
        ptrs = (C.c_void_p * 1)(None)
        assert so.ugsm_submit_foveated_multi(None, 0, None, None, 64, 48, 192, 1, None, None, ptrs) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_match_foveated_multi(None, None, None, 64, 48, 192, 1, None, None, ptrs, ptrs, ptrs) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_reconstruct_full_multi(None, 0, 1, ptrs, 64, 48, None, None, None) == lib.UGSM_ERR_BAD_ARG


@pytest.mark.parametrize("W,H,lv,F,off", [(333, 251, 8, 3, (0, 0)), (333, 251, 8, 3, (-90, 60)), (640, 480, 10, 4, (0, 0))])
def test_the_numpy_restatement_with_one_window_is_the_oracles_reconstruction(orc, W, H, lv, F, off):
    fw, fh = orc.fovea_geometry(W, H, lv, F, off[0], off[1])[:2]
    rng = np.random.Generator(np.random.PCG64(1000 * W + 10 * F + (off[0] != 0)))
    st = rm.random_stack(rng, F, fh, fw)
    assert np.isnan(st).any() and np.isposinf(st).any() and np.isneginf(st).any()
    exp = orc.reconstruct_full(st, W, H, lv, off[0], off[1])
    got = rm.reconstruct_multi(orc, [st], W, H, lv, [off])
    assert_bit_equal(got, exp, f"{W}x{H}, levels {lv}, F {F}, offset {off}: restatement vs oracle")


def test_the_restatement_lets_the_highest_window_win(orc):
    """Three windows: 2 is 0's duplicate, so it covers 0 wholly and beats 1 where they overlap; outside every window the upsample."""
    W, H, lv, F = 333, 251, 8, 3
    offs = [(0, 0), (30, -20), (0, 0)]
    fw, fh, ox, oy, _, _ = orc.fovea_geometry(W, H, lv, F, 0, 0)
    rng = np.random.Generator(np.random.PCG64(77))
    sts = [rm.random_stack(rng, F, fh, fw, specials=0) for _ in offs]
    for s in sts[1:]:
        s[:, F - 1] = sts[0][:, F - 1]
    out = rm.reconstruct_multi(orc, sts, W, H, lv, offs)
    assert_bit_equal(out[:, oy[0]:oy[0] + fh, ox[0]:ox[0] + fw], sts[2][:, 0], "window 2 over window 0 and 1")
    _, _, ox1, oy1, _, _ = orc.fovea_geometry(W, H, lv, F, 30, -20)
    assert (ox1[0], oy1[0]) != (ox[0], oy[0])
    x, y = (ox1[0] + fw - 1, oy1[0]) if ox1[0] > ox[0] else (ox1[0], oy1[0])        # a pixel of window 1 that window 0 / 2 does not hold
    if not (ox[0] <= x < ox[0] + fw and oy[0] <= y < oy[0] + fh):
        assert_bit_equal(out[:, y, x], sts[1][:, 0, y - oy1[0], x - ox1[0]], "window 1 where it lies alone")
