"""Whole calls on the device against what the REFERENCE'S OWN HOST DRIVER gave, bit for bit.

tests/golden/ref_driver_*.npz holds the outputs of the reference's MatchGPULib.cpp, compiled for the CPU with its MatchLib.cu
(oracle/ref_cpu/, tests/ref_driver.py, tests/golden/make_driver_golden.py): match() in both modes, the fovea stack, hierarchicalDisparity's
field, the pyramid and the warped right image, for three pairs (A 231 x 211, B 333 x 251 ragged at every level, C the half-black pair at A's
size: 0 / 0 quotients and pyramid values outside the guarded division range) with the class's own MAX_LEVEL 14 and foveatelevel 7.
Only those files are read here.  Every K-cost / K-smooth form of tests/test_gpu_ref_pin.py carries all fourteen levels of the reference's
schedule, with the kernels that ran asserted from kernel_stats(); tests/test_ref_driver_host.py holds the oracle and the numpy restatement
to the same files on the CPU.
"""
import numpy as np
import pytest

import ref_driver as rd
from conftest import assert_bit_equal
from test_gpu_ref_pin import FORMS
from test_gpu_small import stats_names

pytestmark = pytest.mark.gpu

LEVELS, FL = rd.LEVELS, rd.FOVEA_LEVELS
CASES = list(rd.CASES)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def fixtures():
    return {case: rd.load(case) for case in CASES}


def padded(img, extra=13):
    """The image in rows of 3 * W + extra bytes, as a cv::Mat with a step of its own; the padding holds 0xA5, which no result may show."""
    H, W, _ = img.shape
    out = np.full((H, 3 * W + extra), 0xA5, np.uint8)
    out[:, :3 * W] = img.reshape(H, 3 * W)
    return out


def match_full_host(c, L, R):
    """ugsm_match_full from host bytes with a padded stride"""
    H, W, _ = L.shape
    Lp, Rp = padded(L), padded(R)
    out = np.empty((3, H, W), np.float32)
    c.check(c.lib.ugsm_match_full(c.handle, Lp.ctypes.data, Rp.ctypes.data, W, H, Lp.strides[0], out[0].ctypes.data, out[1].ctypes.data,
                                  out[2].ctypes.data))
    return out


def submit_full_device(c, L, R, slot=0):
    """ugsm_submit_full from device memory, then ugsm_wait"""
    H, W, _ = L.shape
    dL, dR, dO = c.to_device(L), c.to_device(R), c.alloc(3 * W * H * 4)
    try:
        c.check(c.lib.ugsm_submit_full(c.handle, slot, dL, dR, W, H, 3 * W, dO))
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return c.to_host(dO, (3, H, W))
    finally:
        for p in (dL, dR, dO):
            c.free(p)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("form", list(FORMS))
def test_match_full_every_kernel_form(lib, fixtures, monkeypatch, form, case):
    """match(L, R, 0): ugsm_match_full and ugsm_submit_full with every level on one K-cost / K-smooth form."""
    kw, env, must, must_not = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fx, L, R = fixtures[case]
    with lib.Context(levels=LEVELS, fovea_levels=FL, profile_events=2, **kw) as c:
        assert_bit_equal(match_full_host(c, L, R), fx["full"], f"{form}, case {case}: ugsm_match_full")
        assert_bit_equal(submit_full_device(c, L, R), fx["full"], f"{form}, case {case}: ugsm_submit_full")
        names = stats_names(c)
    print(form, case, sorted(names))
    assert must <= names and not (must_not & names), f"{form}: ran {sorted(names)}"


@pytest.mark.parametrize("case", CASES)
def test_match_full_one_slot_and_a_lone_call_on_four_slots(lib, fixtures, case):
    fx, L, R = fixtures[case]
    with lib.Context(levels=LEVELS, fovea_levels=FL, slots=1) as c:
        assert_bit_equal(match_full_host(c, L, R), fx["full"], f"case {case}: slots=1, ugsm_match_full")
        assert_bit_equal(submit_full_device(c, L, R), fx["full"], f"case {case}: slots=1, ugsm_submit_full")
    with lib.Context(levels=LEVELS, fovea_levels=FL, slots=4) as c:
        assert_bit_equal(submit_full_device(c, L, R, slot=2), fx["full"], f"case {case}: slots=4, a lone ugsm_submit_full on slot 2")
    with lib.Context(levels=LEVELS, fovea_levels=FL, slots=4) as c:
        assert_bit_equal(match_full_host(c, L, R), fx["full"], f"case {case}: slots=4, a lone ugsm_match_full")


@pytest.mark.parametrize("case", CASES)
def test_match_foveated_stack_at_the_centred_window(lib, fixtures, case):
    """setFoveated(1), initStack, matchStackPyramid: ugsm_match_foveated with offsets (0, 0)."""
    fx, L, R = fixtures[case]
    H, W, _ = L.shape
    fw, fh = lib.fovea_dims(W, H, LEVELS, FL)
    assert fx["stack"].shape == (3, FL, fh, fw)
    Lp, Rp = padded(L), padded(R)
    st = np.empty((3, FL, fh, fw), np.float32)
    with lib.Context(levels=LEVELS, fovea_levels=FL) as c:
        c.check(c.lib.ugsm_match_foveated(c.handle, Lp.ctypes.data, Rp.ctypes.data, W, H, Lp.strides[0], 0, 0, st[0].ctypes.data, st[1].ctypes.data,
                                          st[2].ctypes.data, None, None))
    assert_bit_equal(st, fx["stack"], f"case {case}: ugsm_match_foveated")


@pytest.mark.parametrize("case", CASES)
def test_reconstruct_full_of_the_reference_stack(lib, fixtures, case):
    """hierarchicalDisparity: ugsm_reconstruct_full of the reference's own stack, so that this does not depend on the stack test."""
    fx, L, _ = fixtures[case]
    H, W, _ = L.shape
    stack = np.ascontiguousarray(fx["stack"])
    with lib.Context(levels=LEVELS, fovea_levels=FL) as c:
        ds = [c.to_device(stack[k]) for k in range(3)]
        dO = c.alloc(3 * W * H * 4)
        try:
            c.reconstruct_full(ds[0], ds[1], ds[2], W, H, dO)
            out = c.to_host(dO, (3, H, W))
        finally:
            for p in ds + [dO]:
                c.free(p)
    assert_bit_equal(out, fx["fovea_full"], f"case {case}: ugsm_reconstruct_full")


@pytest.mark.parametrize("case", CASES)
def test_match_foveated_full(lib, fixtures, case):
    """match(L, R, 1): ugsm_match_foveated_full."""
    fx, L, R = fixtures[case]
    H, W, _ = L.shape
    Lp, Rp = padded(L), padded(R)
    out = np.empty((3, H, W), np.float32)
    with lib.Context(levels=LEVELS, fovea_levels=FL) as c:
        c.check(c.lib.ugsm_match_foveated_full(c.handle, Lp.ctypes.data, Rp.ctypes.data, W, H, Lp.strides[0], 0, 0, out[0].ctypes.data,
                                               out[1].ctypes.data, out[2].ctypes.data))
    assert_bit_equal(out, fx["fovea_full"], f"case {case}: ugsm_match_foveated_full")


@pytest.mark.parametrize("path", [0, 1])
def test_pyramid_levels_0_to_13(lib, fixtures, path):
    """CreatePyramidFromImage: ugsm_stage_pyramid, every level, from an image with a padded stride."""
    fx, L, _ = fixtures["A"]
    H, W, _ = L.shape
    Lp = padded(L)
    with lib.Context(levels=LEVELS, fovea_levels=FL, kernel_path=path) as c:
        p = c.to_device(Lp)
        try:
            for lev in range(LEVELS):
                exp = fx[f"pyr{lev}"].astype(np.float32)
                out = c.alloc(exp.nbytes)
                try:
                    c.check(c.lib.ugsm_stage_pyramid(c.handle, p, W, H, Lp.strides[0], lev, out))
                    assert_bit_equal(c.to_host(out, exp.shape), exp, f"path {path} level {lev}")
                finally:
                    c.free(out)
        finally:
            c.free(p)


def test_warp_planes_against_warp_right_image(lib, fixtures):
    """warpRightImage of the right planes by the reference's full-mode field: ugsm_warp_planes."""
    fx, _, R = fixtures["A"]
    H, W, _ = R.shape
    src = np.ascontiguousarray(R.transpose(2, 0, 1)).astype(np.float32)
    field = np.ascontiguousarray(fx["full"])
    with lib.Context(levels=LEVELS, fovea_levels=FL) as c:
        dS, dX, dY, dO = c.to_device(src), c.to_device(field[0]), c.to_device(field[1]), c.alloc(src.nbytes)
        try:
            c.warp_planes(dS, 3, W, H, dX, dY, dO)
            out = c.to_host(dO, (3, H, W))
        finally:
            for p in (dS, dX, dY, dO):
                c.free(p)
    assert_bit_equal(out, fx["warp_right"].astype(np.float32), "ugsm_warp_planes")
