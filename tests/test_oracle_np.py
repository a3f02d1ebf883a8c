"""The C oracle against the independent numpy restatement (tests/golden/restate_np.py), bit for bit, on the committed
fixtures.  Neither is the reference.  The arithmetic of every stage of both IS held to the reference's own stage code, MatchLib.cu
run on the CPU (oracle/ref_cpu/, tests/test_ref_pin_host.py, tests/golden/ref_stages.npz: DESIGN.md section 3); what the two
restatements agreeing still stands in for is what neither that pin nor the pin of whole calls to the reference's host driver
(tests/test_ref_driver_host.py: fourteen levels at three sizes) reaches -- other sizes and level counts, off-centre windows."""
import os
import sys

import numpy as np
import pytest

import dark_np as dk
from conftest import GOLDEN, assert_bit_equal, load_golden

sys.path.insert(0, GOLDEN)
import restate_np as rn  # noqa: E402


def test_constants_and_schedules(orc):
    assert_bit_equal(rn.gauss_taps(), orc.gauss_taps(), "gauss taps")
    assert rn.level_dims(4928, 3264, 14) == tuple(list(v) for v in orc.level_dims(4928, 3264, 14)) or \
        [list(v) for v in rn.level_dims(4928, 3264, 14)] == [list(v) for v in orc.level_dims(4928, 3264, 14)]
    for mi in (2, 4, 6, 8, 10, 12, 22):
        assert_bit_equal(np.array(rn.thresholds(mi), np.float32), orc.threshold_schedule(mi), f"thresholds mi={mi}")
    for i in range(14):
        assert rn.iterations(i) == orc.iterations_for_level(i) and rn.smooth_passes(i) == orc.smooth_passes_for_level(i)


def test_stage_fixture_96x72(orc):
    g = load_golden("stage_96x72.npz")
    pl, pr = rn.planes(g["L"]), rn.planes(g["R"])
    assert_bit_equal(pl, orc.rgb_to_planes(g["L"]), "planes")
    pyr = rn.pyramid(pl, 4)
    for i in (1, 2, 3):
        assert_bit_equal(pyr[i], g[f"pyr{i}"], f"pyramid level {i}")
    # level index 1: mi = 4 iterations, S = 10 passes in the schedule; the fixture ran mi=4, S=5 -> use level 2's S by hand
    d1 = _iterate(rn, pl, pr, g["d0"], mi=4, S=5, is_top=False, m_from=1, m_to=1)
    assert_bit_equal(d1, g["d1"], "after iteration 1")
    d3 = _iterate(rn, pl, pr, g["d0"], mi=4, S=5, is_top=False, m_from=1, m_to=3)
    assert_bit_equal(d3, g["d3"], "after iteration 3")
    assert_bit_equal(rn.smooth_pass(g["d0"]), g["smooth1"], "smooth")
    assert_bit_equal(np.stack([rn.blur(p, rn.BOX, "clamp") for p in g["d0"]]), g["box"], "box")
    assert_bit_equal(rn.seed(g["d0"], g["seed"].shape[2], g["seed"].shape[1]), g["seed"], "seed")


def _iterate(rn, L, R, d, mi, S, is_top, m_from, m_to):
    """restate_np.iterate_level with an explicit (mi, S) instead of the level's schedule (the stage fixture uses its own)"""
    it, sp = rn.iterations, rn.smooth_passes
    rn.iterations, rn.smooth_passes = (lambda i: mi), (lambda i: S)
    try:
        return rn.iterate_level(L, R, d, 0, is_top, m_from, m_to)
    finally:
        rn.iterations, rn.smooth_passes = it, sp


def test_top_level_first_iteration_has_no_blend(orc):
    g = load_golden("stage_96x72.npz")
    pl, pr = rn.planes(g["L"]), rn.planes(g["R"])
    # the fixture: zero seed, mi = 22, S = 10, is_top, iterations 1-2 (tests/golden/make_golden.py)
    assert_bit_equal(_iterate(rn, pl, pr, np.zeros_like(g["d0"]), 22, 10, True, 1, 2), g["dtop"], "top level, iterations 1-2")


def test_full_64x48(orc):
    g = load_golden("full_64x48_l5.npz")
    out = rn.match_full(g["L"], g["R"], int(g["levels"]))
    assert_bit_equal(out, g["out"], "numpy restatement vs fixture")
    assert_bit_equal(out, orc.match_full(g["L"], g["R"], int(g["levels"])), "numpy restatement vs C oracle")


def test_foveated_320x240(orc):
    g = load_golden("fovea_320x240_l9_f4.npz")
    st = rn.match_foveated(g["L"], g["R"], int(g["levels"]), int(g["F"]))
    assert_bit_equal(st, g["stack"], "foveated stack")


# ---- pairs that leave K-cost's guarded-division range (tests/dark_np.py) -------------------------------------------------------------
# The committed fixtures are [1, 255] texture: no pyramid value of theirs is 0, tiny, or a fringe of black.  The two restatements must
# also agree where the pyramids hold zeros and values down to 1e-8 -- 0 / 0 correlations, quotients of tiny numbers -- because the GPU
# tests of the range word (tests/test_gpu_range_word.py) take the C oracle's answer on such pairs as their expectation.


def _plain(W, H, seed_off):
    from ug_stereomatcher_amd import synth
    return synth.make_pair(W, H, synth.BASE_SEED + seed_off)[:2]


@pytest.mark.parametrize("recipe", ["dark noise", "one dim pixel"])
def test_full_on_pairs_outside_the_guarded_range_160x120(orc, recipe):
    """C oracle vs numpy restatement, bit for bit, 160 x 120 x 8 levels, on a pair whose pyramids hold values outside range_ok (the
    premise, asserted: none at levels 0-2, some at a level >= 3; the plain pair has none)."""
    W, H, lv = 160, 120, 8
    L, R = _plain(W, H, 611)
    assert dk.pair_word(orc, L, R, lv)[0] == 0, "the plain pair must stay inside the range"
    if recipe == "dark noise":
        L2, R2 = dk.dark_pair(L, R, 5)
        assert dk.trips(dk.out_of_range_levels(orc, R2, lv))
    else:
        L2, R2 = dk.one_dim_pixel(L, 64, 1, (60, 80)), R
    counts = dk.out_of_range_levels(orc, L2, lv)
    print(f"{recipe}: out-of-range values per level of L: {counts}")
    assert dk.trips(counts), counts
    out = orc.match_full(L2, R2, lv)
    assert np.isfinite(out).all()
    assert_bit_equal(rn.match_full(L2, R2, lv), out, f"numpy restatement vs C oracle, {recipe}")


@pytest.mark.parametrize("name", ["all 0", "all 255", "constant 7", "L black, R textured", "L textured, R black"])
def test_full_on_degenerate_pairs_160x120(orc, name):
    """Flat and black images: every pyramid value is 0 or a constant in range (word 0), every correlation 0 / 0 or 1; both restatements
    give the same finite field."""
    W, H, lv = 160, 120, 8
    L2, R2 = dk.degenerate_pairs(*_plain(W, H, 612))[name]
    assert dk.pair_word(orc, L2, R2, lv)[0] == 0
    out = orc.match_full(L2, R2, lv)
    assert np.isfinite(out).all()
    assert_bit_equal(rn.match_full(L2, R2, lv), out, f"numpy restatement vs C oracle, {name}")


def test_foveated_on_the_dark_pair_320x240(orc):
    """The foveated restatement (320 x 240 x 9 levels, F = 4) on the dark-noise pair."""
    W, H, lv, F = 320, 240, 9, 4
    L2, R2 = dk.dark_pair(*_plain(W, H, 613), 9)
    cl, cr = dk.out_of_range_levels(orc, L2, lv), dk.out_of_range_levels(orc, R2, lv)
    print(f"dark pair, out-of-range values per level: L {cl}, R {cr}")
    assert dk.trips(cl) and dk.trips(cr)
    st = orc.match_foveated(L2, R2, lv, F)[0]
    assert np.isfinite(st).all()
    assert_bit_equal(rn.match_foveated(L2, R2, lv, F), st, "foveated stack, numpy restatement vs C oracle")
