"""One context through calls of changing size, kind and format (tests/context_life.py: the steps, the runner, the scripts).

Every entry point has its own test against the CPU oracle, almost all on a context made for that test and one frame size.  A node keeps one
context for life: service calls of every kind, clouds, depth images and warps, changes of camera resolution and encoding follow each other on
the same few slots, often submitted before the last call has finished.  What meets there is the slot's state (csrc/ugsm_slot.hpp): sizes,
strides and offsets, the grow-only capacities, the layout of the result staging, have_pyr / direct0 / a_from / range_known, the LR words.

Each scripted group is one test: (a) grow, reuse, shrink, grow; (b) the batch dimension and checked -> plain; (c) the staging layouts of the
blocking host calls between foveated and multi-window calls; (d) what a call -- a refused one too -- leaves behind; (e) settings changed right
behind an unfinished call; (f) level 0 read from the images, then everything else; (g) post-processing between matches; (h) two slots, one
borrowing the other's stream, and three slots on one stream; (i) out of memory in the middle.  Then three random walks over all kinds.

For every script: every output of every step equals the CPU oracle's bit for bit (refused steps leave their poison), guard bands and inputs
are untouched, and -- without a memory limit -- the script is played a second time on the same, now warm, context: bit-equal again, with
ugsm_context_device_bytes never decreasing during the first pass and standing still during the replay.  A mismatch is reported with the verdict
of the failing step played alone on a fresh context: right there (the slot's history) or wrong there too (the step itself).
tests/test_context_life_host.py holds the scripts to their purpose on the CPU."""
import pytest

import context_life as cl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def exp(orc):
    """The expected values, once per distinct case for the whole file."""
    return cl.Expect(orc)


@pytest.fixture
def every_level_through_k_cost_march(monkeypatch):
    """The development switches of tests/test_gpu_level0_direct.py: with march_min_pixels = 1 a full-mode call on rgb8 images reads level 0 from
    the images and stores none."""
    monkeypatch.setenv("UGSM_MARCH4", "0,0")
    monkeypatch.delenv("UGSM_LEVEL0_FLOAT", raising=False)


def test_every_frame_is_accepted(lib):
    for name, (W, H) in cl.FRAMES.items():
        w, h = lib.level_dims(W, H, cl.LEVELS)
        assert len(w) == cl.LEVELS and min(w + h) >= 1, name


def _group(lib, exp, name, cfg, script=None):
    return cl.play_twice(lib, cfg, exp, script or cl.GROUPS[name][0](), f"group {name}: ")


def test_a_grow_reuse_shrink_grow(lib, exp):
    _group(lib, exp, "a", cl.MAIN)


def test_b_the_batch_dimension(lib, exp):
    _group(lib, exp, "b", cl.MAIN)


def test_c_staging_layouts(lib, exp):
    _group(lib, exp, "c", cl.MAIN)


def test_d_what_a_call_leaves_behind(lib, exp, every_level_through_k_cost_march):
    """Under the switches of test_fovea_coarse_after_a_full_call_needs_the_pyramids_again: there a full-mode call leaves no whole pyramids.  (On the
    default policy a frame this small keeps its float level 0, and ugsm_submit_fovea_coarse behind it is served: test_gpu_level0_direct.py.)"""
    _group(lib, exp, "d", {**cl.MAIN, **cl.DIRECT})


def test_e_settings_behind_an_unfinished_call(lib, exp):
    _group(lib, exp, "e", cl.MAIN)


def test_f_level0_from_the_images_then_everything_else(lib, exp, every_level_through_k_cost_march):
    _group(lib, exp, "f", {**cl.MAIN, **cl.DIRECT, "dev": True})


def test_g_post_processing_between_matches(lib, exp):
    _group(lib, exp, "g", cl.MAIN)


def test_h_two_slots(lib, exp):
    _group(lib, exp, "h", cl.MAIN)


def test_h_three_slots_on_one_stream(lib, exp):
    _group(lib, exp, "h", cl.SHARED, cl.group_h(third_slot=True))


def test_i_out_of_memory_in_the_middle(lib, exp, monkeypatch):
    """The limit from ugsm_context_device_bytes of two scratch contexts: what one C pair holds (a context of batch 1: the slot sized for the call
    alone, as the limited context falls back to) and what four A pairs hold.  Four C pairs need four times the former."""
    script = cl.group_i()
    with lib.Context(**{**cl.MAIN, "batch": 1}) as c:
        one_c = cl.play(lib, c, exp, [script[0]], what="group i, one C pair: ")[-1]
    with lib.Context(**cl.MAIN) as c:
        four_a = cl.play(lib, c, exp, [script[3]], what="group i, four A pairs: ")[-1]
    limit_mb = (max(one_c, four_a) >> 20) + 2
    print(f"group i: one C pair holds {one_c} bytes, four A pairs {four_a}; the limit is {limit_mb} MB")
    assert four_a < one_c and (limit_mb << 20) < 2 * one_c, "four C pairs must not fit"
    monkeypatch.setenv("UGSM_MEM_LIMIT_MB", str(limit_mb))
    with lib.Context(**cl.MAIN) as c:
        held = cl.play(lib, c, exp, script, cl.MAIN, "group i: ")
    print(f"group i: device bytes behind every step {held}")
    assert max(held) <= limit_mb << 20, held
    assert held[1] <= held[0], "the refused call kept memory it could not use"


@pytest.mark.parametrize("seed", cl.WALK_SEEDS)
def test_random_walk(lib, exp, seed):
    cl.play_twice(lib, cl.MAIN, exp, cl.walk(seed), f"walk {seed}: ")
