"""Whole calls against what the REFERENCE'S OWN HOST DRIVER gave, bit for bit, on the CPU.

tests/golden/ref_driver_*.npz holds the outputs of MatchGPULib.cpp -- match() in both modes, initStack + matchStackPyramid,
hierarchicalDisparity, CreatePyramidFromImage, gaussiankernel, warpRightImage -- compiled for the CPU with MatchLib.cu and run as
oracle/_ref/ref_driver (oracle/ref_cpu/, tests/ref_driver.py, tests/golden/make_driver_golden.py) on three pairs with the class's own
MAX_LEVEL 14 and foveatelevel 7.  That pins what tests/test_ref_pin_host.py cannot: the order of the stage calls and the buffers that
alias, the iterations and smoothing passes per level, the taps and the threshold schedule, the pyramid, the seeding between ragged levels,
the zero start at the coarsest level, the fovea crop and the reconstruction.

The first half reads only tests/golden/ and always runs: the oracle and the numpy restatement against the fixtures.  The second half runs
where the driver was built (the reference checkout is present): a fresh run gives the fixture; the zero start is the recorded deviation
U1 and is load-bearing; the stand-in's host calls do what the result rests on.  tests/test_gpu_ref_driver.py holds the device to the same
files.
"""
import ctypes as C
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dark_np
import ref_driver as rd
import warp_np as wn
from conftest import GOLDEN, assert_bit_equal

sys.path.insert(0, GOLDEN)
import restate_np as rn  # noqa: E402

F32 = np.float32
LEVELS, FL = rd.LEVELS, rd.FOVEA_LEVELS
CASES = list(rd.CASES)


@pytest.fixture(scope="module")
def fixtures():
    return {case: rd.load(case) for case in CASES}


# ---- the fixtures are what they claim to be ----------------------------------------------------------------------------------------------

def test_case_a_is_the_smallest_odd_size_and_every_case_is_ragged(orc):
    """The cases' own premises: 211 is the smallest odd size 14 levels accept; A's width and height differ at every level down to 4 x 3;
    B's sizes are no multiple of anything the kernels tile by at any level (no level of B is a multiple of 16 in both directions)."""
    with pytest.raises(ValueError):
        orc.level_dims(209, 209, LEVELS)
    assert orc.level_dims(211, 211, LEVELS)[0][-1] == 1
    a = rd.CASES["A"]
    w, h = orc.level_dims(a["W"], a["H"], LEVELS)
    assert a["W"] % 2 == 1 and a["H"] == 211 and all(x != y for x, y in zip(w[:-2], h[:-2])), (w, h)
    assert [x for x in range(213, a["W"], 2) if all(p != q for p, q in zip(orc.level_dims(x, 211, LEVELS)[0][:-2], h[:-2]))] == []
    b = rd.CASES["B"]
    w, h = orc.level_dims(b["W"], b["H"], LEVELS)
    assert not any(x % 16 == 0 and y % 16 == 0 for x, y in zip(w, h)), (w, h)


def test_case_c_has_zero_over_zero_quotients_and_leaves_the_guarded_range(orc, fixtures):
    """Case C's premise: at zero disparity K-cost's quotients N^2 / (A * B) at level 0 include 0 / 0 (NaN), and both
    pyramids hold values outside the guarded division range at levels >= 3 (the range word of the pair is 1)."""
    _, L, R = fixtures["C"]
    num, den = dark_np.kcost_operands(orc, orc.rgb_to_planes(L), orc.rgb_to_planes(R))
    assert int(((num == 0) & (den == 0)).sum()) > 1000
    word, cl, cr = dark_np.pair_word(orc, L, R, LEVELS)
    assert word == 1 and dark_np.trips(cl) and dark_np.trips(cr), (cl, cr)


def test_fixture_shapes(orc, fixtures):
    for case, (fx, L, _) in fixtures.items():
        H, W, _ = L.shape
        fw, fh, *_ = orc.fovea_geometry(W, H, LEVELS, FL)
        assert fx["full"].shape == fx["fovea_full"].shape == (3, H, W) and fx["stack"].shape == (3, FL, fh, fw), case
        assert fx["full"].dtype == fx["stack"].dtype == fx["fovea_full"].dtype == F32
    fx = fixtures["A"][0]
    w, h = orc.level_dims(int(fx["W"]), int(fx["H"]), LEVELS)
    assert [fx[f"pyr{k}"].shape for k in range(LEVELS)] == [(3, h[k], w[k]) for k in range(LEVELS)]  # the driver's own .dims record


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_oracle_match_full(orc, fixtures, case):
    fx, L, R = fixtures[case]
    assert_bit_equal(orc.match_full(L, R, LEVELS), fx["full"], f"case {case}: orc.match_full vs match(L, R, 0)")


@pytest.mark.parametrize("case", CASES)
def test_oracle_match_foveated_stack(orc, fixtures, case):
    fx, L, R = fixtures[case]
    assert_bit_equal(orc.match_foveated(L, R, LEVELS, FL)[0], fx["stack"], f"case {case}: orc.match_foveated vs matchStackPyramid")


@pytest.mark.parametrize("case", CASES)
def test_oracle_reconstruct_full(orc, fixtures, case):
    """Of the reference's stack, so that this does not depend on the stack test."""
    fx, L, _ = fixtures[case]
    H, W, _ = L.shape
    assert_bit_equal(orc.reconstruct_full(fx["stack"], W, H, LEVELS), fx["fovea_full"], f"case {case}: orc.reconstruct_full vs hierarchicalDisparity")


def test_oracle_pyramid(orc, fixtures):
    fx, L, _ = fixtures["A"]
    pyr = orc.pyramid(orc.rgb_to_planes(L), LEVELS)
    for k in range(LEVELS):
        assert_bit_equal(pyr[k], fx[f"pyr{k}"].astype(F32), f"orc.pyramid level {k} vs CreatePyramidFromImage")


def test_oracle_gauss_taps(orc, fixtures):
    assert orc.gauss_taps().view(np.uint32).tolist() == fixtures["A"][0]["taps_bits"].tolist()


@pytest.mark.parametrize("case", CASES)
def test_oracle_schedule_functions_through_the_whole_call(orc, fixtures, case):
    """orc.iterations_for_level and orc.smooth_passes_for_level, as Python sees them, drive the oracle's own pieces (pyramid, iterate_level
    from a zero start, seed) through all fourteen levels: the result is the reference's full-mode field."""
    fx, L, R = fixtures[case]
    pl, pr = orc.pyramid(orc.rgb_to_planes(L), LEVELS), orc.pyramid(orc.rgb_to_planes(R), LEVELS)
    cur = np.zeros_like(pl[LEVELS - 1])
    for i in range(LEVELS - 1, -1, -1):
        cur, _ = orc.iterate_level(pl[i], pr[i], cur, orc.iterations_for_level(i), orc.smooth_passes_for_level(i), i == LEVELS - 1)
        if i > 0:
            cur = orc.seed(cur, pl[i - 1].shape[2], pl[i - 1].shape[1])
    assert_bit_equal(cur, fx["full"], f"case {case}: composed from the oracle's schedule functions")


def test_oracle_threshold_schedule_through_the_whole_call(orc, fixtures, monkeypatch):
    """orc.threshold_schedule (with the two count functions) in the place of the restatement's own schedule, through the restatement's
    whole call: still the reference's field.  The schedule is exercised: a constant 1.0 in its place gives another field."""
    fx, L, R = fixtures["A"]
    used = sorted({orc.iterations_for_level(i) for i in range(LEVELS)})
    assert used == [2, 4, 6, 8, 10, 12, 22]
    monkeypatch.setattr(rn, "iterations", orc.iterations_for_level)
    monkeypatch.setattr(rn, "smooth_passes", orc.smooth_passes_for_level)
    monkeypatch.setattr(rn, "thresholds", lambda mi: [F32(v) for v in orc.threshold_schedule(mi)])
    assert_bit_equal(rn.match_full(L, R, LEVELS), fx["full"], "restate_np.match_full on the oracle's schedule")
    monkeypatch.setattr(rn, "thresholds", lambda mi: [F32(1.0)] * mi)
    assert (rn.match_full(L, R, LEVELS).view(np.uint32) != fx["full"].view(np.uint32)).any()


# ---- the numpy restatement and the warp ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_restatement_match_full(fixtures, case):
    fx, L, R = fixtures[case]
    assert_bit_equal(rn.match_full(L, R, LEVELS), fx["full"], f"case {case}: restate_np.match_full vs match(L, R, 0)")


@pytest.mark.parametrize("case", CASES)
def test_restatement_match_foveated_stack(fixtures, case):
    fx, L, R = fixtures[case]
    assert_bit_equal(rn.match_foveated(L, R, LEVELS, FL), fx["stack"], f"case {case}: restate_np.match_foveated vs matchStackPyramid")


def test_restatement_pyramid_and_taps(fixtures):
    fx, L, _ = fixtures["A"]
    pyr = rn.pyramid(rn.planes(L), LEVELS)
    for k in range(LEVELS):
        assert_bit_equal(pyr[k], fx[f"pyr{k}"].astype(F32), f"restate_np.pyramid level {k}")
    assert rn.gauss_taps().view(np.uint32).tolist() == fx["taps_bits"].tolist()


def test_warp_np_against_warp_right_image(fixtures):
    fx, _, R = fixtures["A"]
    assert_bit_equal(wn.warp(wn.planes(R), fx["full"][0], fx["full"][1]), fx["warp_right"].astype(F32), "warp_np.warp vs warpRightImage")
    assert (fx["warp_right"] != wn.planes(R).astype(np.uint8)).mean() > 0.5  # the field moves most pixels: the warp is exercised


# ---- where the driver is built: fresh runs -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fresh(orc, fixtures):
    """The reference's runs at case A, side by side (each is a process of its own, about a minute): the full-mode call, the same with every
    new word of host memory FLT_MAX in place of zero, the stack with its reconstruction; and the quick ones."""
    if not rd.available():
        pytest.skip("oracle/_ref/ref_driver was not built (no reference checkout): tests/golden/ref_driver_*.npz carry the pin")
    _, L, R = fixtures["A"]
    with rd.Session(L, R) as s, ThreadPoolExecutor(3) as pool:
        full, filled, stack = pool.submit(s.match, 0), pool.submit(s.match, 0, host_fill=rd.NONZERO_FILL), pool.submit(s.stack)
        out = dict(pyr=s.pyramid(), taps=s.taps(), full=full.result(), filled=filled.result())
        out["stack"], out["fovea_full"] = stack.result()
        out["warp_right"] = s.warp_right(out["full"])
    return out


def test_fresh_run_gives_the_fixture(fresh, fixtures):
    fx = fixtures["A"][0]
    for key in ("full", "stack", "fovea_full"):
        assert_bit_equal(fresh[key], fx[key], f"fresh {key} vs fixture")
    for k in range(LEVELS):
        assert_bit_equal(fresh["pyr"][k], fx[f"pyr{k}"].astype(F32), f"fresh pyramid level {k} vs fixture")
    assert fresh["taps"].view(np.uint32).tolist() == fx["taps_bits"].tolist()
    assert_bit_equal(fresh["warp_right"], fx["warp_right"].astype(F32), "fresh warpRightImage vs fixture")


def test_the_zero_start_is_the_recorded_deviation(fresh, fixtures):
    """U1: the driver reads the coarsest level's disparity planes from malloc before anything wrote them (MatchGPULib.cpp:1247, :1764-1765).
    host_alloc.h makes that memory zero, the oracle's start.  With FLT_MAX there instead the field is another one: the fill is read, the
    zero is a decision of this build and not the reference's."""
    fx = fixtures["A"][0]
    differ = fresh["filled"].view(np.uint32) != fx["full"].view(np.uint32)
    print("values that differ with host memory filled with FLT_MAX:", int(differ.sum()), "of", differ.size)
    assert differ.any()


@pytest.fixture(scope="module")
def shim(orc):
    lib = orc.matchlib_cpu()
    if lib is None:
        pytest.skip("oracle/_ref/libmatchlib_cpu.so is not built: the reference checkout is not here")
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_stand_in_array_owns_its_texels(shim):
    """cudaMemcpyToArray, device to device, into an array of cudaMallocArray is a snapshot: matchlevel overwrites the buffer a texture was
    copied from (the warped plane, the smoothed field) and must keep fetching the old values until it copies again."""
    rng = np.random.Generator(np.random.PCG64(9420))
    src = rng.normal(0, 50, (7, 13)).astype(F32)
    out, out2 = np.empty_like(src), np.empty_like(src)
    assert shim.shim_array_snapshot(_p(src), 13, 7, _p(out), _p(out2)) == 0
    assert_bit_equal(out, src, "texels after the source buffer was overwritten")
    assert_bit_equal(out2, -src - F32(1.0), "texels after the second copy")


def test_stand_in_memcpy_to_array_offsets_and_bounds(shim, monkeypatch):
    monkeypatch.setenv("UGSM_REF_DEVICE_FILL", "7fc00000")  # untouched texels are NaN
    src = np.arange(1, 36, dtype=F32)
    f = shim.shim_memcpy_to_array

    def run(w_off, h_off, count):
        out = np.empty((5, 7), F32)
        return f(_p(src), 7, 5, w_off, h_off, count, _p(out)), out

    st, out = run(0, 0, 35 * 4)
    assert st == 0 and (out.ravel() == src).all()
    st, out = run(8, 2, 9 * 4)     # from texel 2 of row 2 on, row after row
    assert st == 0 and (out.ravel()[16:25] == src[:9]).all() and np.isnan(out.ravel()[:16]).all() and np.isnan(out.ravel()[25:]).all()
    for bad in ((0, 0, 35 * 4 + 1), (4, 4, 7 * 4), (0, 5, 4), (28, 0, 4)):
        st, out = run(*bad)
        assert st == 1 and np.isnan(out).all(), bad   # cudaErrorInvalidValue, nothing copied


def test_stand_in_memcpy_between_overlapping_ranges(shim):
    for frm, to in ((0, 3), (3, 0)):
        buf = np.arange(20, dtype=F32)
        assert shim.shim_memcpy_overlap(_p(buf), frm, to, 15) == 0
        exp = np.arange(20, dtype=F32)
        exp[to:to + 15] = np.arange(20, dtype=F32)[frm:frm + 15]
        assert (buf == exp).all(), (frm, to)


def test_stand_in_fresh_memory_holds_the_fill_word(shim, monkeypatch):
    first, last = C.c_uint(1), C.c_uint(1)
    for kind, env in ((0, "UGSM_REF_DEVICE_FILL"), (1, "UGSM_REF_HOST_FILL"), (2, "UGSM_REF_DEVICE_FILL")):
        for word in (None, "7f7fffff"):
            monkeypatch.delenv("UGSM_REF_DEVICE_FILL", raising=False)
            monkeypatch.delenv("UGSM_REF_HOST_FILL", raising=False)
            if word:
                monkeypatch.setenv(env, word)
            assert shim.shim_fresh_words(kind, 4096, C.byref(first), C.byref(last)) == 0
            assert first.value == last.value == (int(word, 16) if word else 0), (kind, word)
