"""The warped right image and the photometric residual (ugsm_warp_planes, ugsm_warp_right, ugsm_warp_right_fovea,
ugsm_photometric_residual, ugsm_photometric_residual_fovea) without a GPU: declarations and exports, the numpy restatement
(tests/warp_np.py) against the fixture written from the reference's own `warp` stage and against that stage live, its residual against the
oracle's weightedDifference, the refusal of calls without a context, and the shim's warpRightImage against the reference's signature."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ref_stages as rs
import warp_np as wn
from conftest import ROOT, assert_bit_equal, load_golden

NEW = ["ugsm_warp_planes", "ugsm_warp_right", "ugsm_warp_right_fovea", "ugsm_photometric_residual", "ugsm_photometric_residual_fovea"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_warp_symbols_are_declared_and_exported_by_both_libraries(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().ugsm_abi_version() == 6
    for word in ("per-pixel residual map", "queue / managed forms", "feeds back into the confidence"):   # the NOT-built list is stated
        assert word in hdr, word


def test_fixture_covers_the_shapes():
    g = load_golden("warp_right.npz")
    assert [tuple(s) for s in g["shapes"].tolist()] == wn.SHAPES == [(37, 29), (130, 75), (160, 120), (333, 217)]
    assert (int(g["pair_seed"]), int(g["field_seed"])) == (wn.PAIR_SEED, wn.FIELD_SEED)
    for W, H in wn.SHAPES:
        assert g[f"{W}x{H}"].shape == (3, H, W) and g[f"{W}x{H}"].dtype == np.uint8
    assert g["130x75_wild"].shape == (3, 75, 130)
    wild = wn.fixture_inputs(wn.SHAPES.index(wn.WILD))[3]
    for v in (np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -(2.0 ** 31), -0.5, 1e-40):
        assert (wild == np.float32(v)).any(), v
    assert np.isnan(wild).any()


@pytest.mark.parametrize("k", range(len(wn.SHAPES)))
def test_restatement_equals_the_fixture(k):
    g = load_golden("warp_right.npz")
    W, H = wn.SHAPES[k]
    _, R, d, wild = wn.fixture_inputs(k)
    assert d[0].min() < -W / 40 and (d[0] + np.arange(W)).max() > W and (d[1] + np.arange(H)[:, None]).max() > H   # past the borders
    assert_bit_equal(wn.warp(wn.planes(R), d[0], d[1]), g[f"{W}x{H}"].astype(np.float32), f"warp_np vs the fixture, {W}x{H}")
    if wild is not None:
        assert_bit_equal(wn.warp(wn.planes(R), wild[0], wild[1]), g[f"{W}x{H}_wild"].astype(np.float32), "warp_np vs the fixture, wild field")


@pytest.mark.parametrize("k", range(len(wn.SHAPES)))
def test_restatement_equals_the_reference_stage_live(orc, k):
    ref = rs.load(orc)
    if ref is None:
        pytest.skip("oracle/_ref/libmatchlib_cpu.so was not built (no reference checkout)")
    W, H = wn.SHAPES[k]
    _, R, d, wild = wn.fixture_inputs(k)
    for f in (d, wild):
        if f is not None:
            live = np.stack([ref.warp(p, f[0], f[1]) for p in wn.planes(R)])
            assert_bit_equal(wn.warp(wn.planes(R), f[0], f[1]), live, f"warp_np vs RefStages.warp, {W}x{H}")


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("weighted", [True, False])
def test_residual_equals_weighted_difference(orc, k, weighted):
    W, H = wn.SHAPES[k]
    L, R, d, _ = wn.fixture_inputs(k)
    conf = d[2] if weighted else None
    c = d[2] if weighted else np.ones((H, W), np.float32)
    L3, Rw3 = wn.planes(L), wn.warp(wn.planes(R), d[0], d[1])
    q, total = wn.residual(L3, Rw3, conf)
    a = orc.weighted_difference(np.stack([L3[0], L3[1], c]), np.stack([Rw3[0], Rw3[1], c]))
    b = orc.weighted_difference(np.stack([L3[2], L3[1], c]), np.stack([Rw3[2], Rw3[1], c]))
    assert_bit_equal(q, np.array([a[0], a[1], b[0]], np.float32), f"S / C vs weighted_difference, {W}x{H}")
    assert np.float32(b[1]) == q[1]
    # the order matters at this size: the sums are not np.sum's
    sums = wn.residual_sums(L3, Rw3, conf)
    assert sums.dtype == np.float64 and sums[3] == total and np.isfinite(sums).all()
    if not weighted:
        assert sums[3] == W * H


def test_a_null_confidence_is_a_confidence_of_ones():
    L, R, d, _ = wn.fixture_inputs(0)
    L3, Rw3 = wn.planes(L), wn.warp(wn.planes(R), d[0], d[1])
    assert wn.residual_sums(L3, Rw3, None).tobytes() == wn.residual_sums(L3, Rw3, np.ones(L3.shape[1:], np.float32)).tobytes()


def _fake(lib, name, **over):
    """One call of entry point `name` with plausible (fake, never dereferenced) device pointers."""
    a = dict(ctx=None, slot=0, src=0x10000, L=0x10000, R=0x20000, dx=0x30000, dy=0x40000, conf=0x50000, dst=0x60000, sums=0x70000, W=64, H=48,
             stride=192, channels=3)
    a.update(over)
    so = lib.load()
    if name == "ugsm_warp_planes":
        return so.ugsm_warp_planes(a["ctx"], a["slot"], a["src"], a["channels"], a["W"], a["H"], a["dx"], a["dy"], a["dst"])
    if name == "ugsm_warp_right":
        return so.ugsm_warp_right(a["ctx"], a["slot"], a["R"], a["W"], a["H"], a["stride"], a["dx"], a["dy"], a["dst"])
    if name == "ugsm_warp_right_fovea":
        return so.ugsm_warp_right_fovea(a["ctx"], a["slot"], a["R"], a["dx"], a["dy"], a["W"], a["H"], a["dst"])
    if name == "ugsm_photometric_residual":
        return so.ugsm_photometric_residual(a["ctx"], a["slot"], a["L"], a["R"], a["W"], a["H"], a["stride"], a["dx"], a["dy"], a["conf"], a["sums"])
    return so.ugsm_photometric_residual_fovea(a["ctx"], a["slot"], a["L"], a["R"], a["dx"], a["dy"], a["conf"], a["W"], a["H"], a["sums"])


def bad_argument_cases(name):
    """Every argument refusal of entry point `name` (label, overrides); shared with the GPU test, which makes them on a live context."""
    image = name in ("ugsm_warp_right", "ugsm_photometric_residual")
    sums = name.startswith("ugsm_photometric")
    cases = [("W 0", dict(W=0)), ("H 0", dict(H=0)), ("W < 0", dict(W=-3)), ("above 2^28 pixels", dict(W=1 << 15, H=(1 << 13) + 1)),
             ("slot -1", dict(slot=-1)), ("slot 99", dict(slot=99)), ("no dx", dict(dx=None)), ("no dy", dict(dy=None))]
    cases += [("no right", dict(R=None))] if name != "ugsm_warp_planes" else [("no source", dict(src=None))]
    if image:
        cases += [("stride short", dict(stride=64 * 3 - 1)), ("stride 0", dict(stride=0))]
    if sums:
        cases += [("no left", dict(L=None)), ("no sums", dict(sums=None)), ("sums misaligned", dict(sums=0x70004))]
    else:
        cases += [("no destination", dict(dst=None))]
    if name == "ugsm_warp_planes":
        cases += [("channels 0", dict(channels=0)), ("channels 97", dict(channels=97)), ("in place", dict(dst=0x10000))]
    if name == "ugsm_warp_right_fovea":
        cases += [("in place", dict(dst=0x20000))]
    return cases


@pytest.mark.parametrize("name", NEW)
def test_null_context_and_bad_arguments_are_refused_without_a_device(lib, name):
    """Without a device there is no context, so every call here is refused for its null context, whatever else it carries: the entry point
    takes the argument list and answers before it touches anything.  Each check on its own: tests/test_gpu_warp.py, on a live context."""
    assert _fake(lib, name) == lib.UGSM_ERR_BAD_ARG
    for label, over in bad_argument_cases(name):
        assert _fake(lib, name, **over) == lib.UGSM_ERR_BAD_ARG, label


def test_shim_declares_warp_right_image_with_the_reference_signature(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "warp_right_image.cpp"
    src.write_text('#include "MatchGPULib_ugsm.hpp"\n'
                   "float **call(MatchGPULib &m, float **right, float **disparity, int channels, int imageW, int imageH)\n"
                   "{\n"
                   "    float **(MatchGPULib::*member)(float **, float **, int, int, int) = &MatchGPULib::warpRightImage;\n"
                   "    (void)member;\n"
                   "    return m.warpRightImage(right, disparity, channels, imageW, imageH);\n"
                   "}\n")
    r = subprocess.run([gxx, "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-Itests/ros_stubs", "-Iros", "-Iinclude", str(src)], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
