"""K-cost's guarded division and the device word that guards it, driven through whole calls on dark, noisy and flat images.

k_cost_march / k_cost_march4 divide with div_inrange (csrc/ugsm_exact.hpp) while the pair's range word (Slot::range_bad, one per pair of
a call) is 0.  The word is zeroed by enqueue_pyramids and set by whichever pyramid kernel writes a value outside range_ok
(v == 0 or 2^-12 <= v <= 2^9).  synth.make_pair images never set it; the images of tests/dark_np.py do, from level 3 down.

Every case asserts its premise on the CPU first (dark_np.pair_word on the oracle's pyramids: the tripping pair has out-of-range values
at some level >= 3 and none at levels 0-2, the control pair none at all), then
  (a) the result equals the oracle's bit for bit, and
  (b) the word read back (ugsm_stage_range_words, libugsm_dev.so) is 1 exactly for the tripping pairs and 0 for the others.
(b) is what makes a missed detection fail -- either division gives the same bits on almost every operand, so (a) alone would pass -- and
its zero half is what catches a stale or over-eager word, which costs a healthy pair ~41 instead of ~26 issue cycles on each of its 15
divisions per pixel-iteration and changes nothing else.  Each case prints its premise (per-level counts) next to the words it read.

The premises as measured on an MI355X run (640 x 480, 14 levels; out-of-range values per level 0 .. 13 of L | R; word expected = read back
in every case of every test):
  plain, plain2   none | none                                                                                       0 = 0
  dark            0 0 0 261 146 904 452 232 29 3 0 0 0 0 | 0 0 0 320 209 1033 461 174 8 0 0 0 0 0                   1 = 1
  dark R          none | as dark's R                                                                                1 = 1
  pixel           0 0 0 3 0 21 0 ... | none                                                                         1 = 1
  pixel32         0 0 0 6 0 ... | none                                                                              1 = 1
  dark as mono8   0 0 0 273 144 906 471 237 27 3 0 0 0 0 | 0 0 0 339 237 1047 477 174 12 0 0 0 0 0                  1 = 1
  16 MP dark      0 0 0 16334 9344 56364 26846 11299 1272 52 0 ... | 0 0 0 15825 9186 56842 27910 11952 1543 41 0 ...   slots 0-3: 1 0 1 0
"""
import ctypes as C

import numpy as np
import pytest

import dark_np as dk
import encode_np as en
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

W, H, LV = 640, 480, 14


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


class Pair:
    """A pair, the word the device must report for it and the per-level counts behind that word; the oracle's answers on demand."""

    def __init__(self, orc, name, L, R, levels=LV):
        self.orc, self.name, self.levels = orc, name, levels
        self.L, self.R = np.ascontiguousarray(L), np.ascontiguousarray(R)
        self.word, self.cl, self.cr = dk.pair_word(orc, self.L, self.R, levels)
        self._full, self._fov = None, {}

    @property
    def full(self):
        if self._full is None:
            self._full = self.orc.match_full(self.L, self.R, self.levels)
        return self._full

    def fovea(self, F, off):
        if (F, off) not in self._fov:
            self._fov[(F, off)] = self.orc.match_foveated(self.L, self.R, self.levels, F, off[0], off[1])[0]
        return self._fov[(F, off)]

    def premise(self):
        return f"{self.name}: out-of-range values per level L {self.cl} R {self.cr} -> word {self.word}"


@pytest.fixture(scope="module")
def bank(orc):
    """The 640 x 480 pairs every case draws from, premises asserted once: two plain pairs, the dark pair (noise in the dark third, black
    frame, saturated block; both images), the dark right image beside the plain left one, and the lone dim pixels."""
    from ug_stereomatcher_amd import synth
    L0, R0 = synth.make_pair(W, H, synth.BASE_SEED + 300)[:2]
    L1, R1 = synth.make_pair(W, H, synth.BASE_SEED + 307)[:2]
    dL, dR = dk.dark_pair(L0, R0, 77)
    b = {
        "plain": Pair(orc, "plain", L0, R0),
        "plain2": Pair(orc, "plain2", L1, R1),
        "dark": Pair(orc, "dark", dL, dR),
        "dark R": Pair(orc, "dark R", L0, dR),
        # a (1, 1, 1) pixel at the centre of a 64 x 64 black block of L: a few dozen values at two levels decide
        "pixel": Pair(orc, "pixel", dk.one_dim_pixel(L0, 64, 1, (H // 5 + 32, W // 4 + 32)), R0),
        # ... and in a 32 x 32 block: the fringe leaves the range at level 3 only
        "pixel32": Pair(orc, "pixel32", dk.one_dim_pixel(L1, 32, 1, (240, 320)), R1),
    }
    for k in ("plain", "plain2"):
        assert b[k].word == 0 and sum(b[k].cl) + sum(b[k].cr) == 0, b[k].premise()
    assert dk.trips(b["dark"].cl) and dk.trips(b["dark"].cr), b["dark"].premise()
    assert sum(b["dark R"].cl) == 0 and dk.trips(b["dark R"].cr), b["dark R"].premise()
    for k in ("pixel", "pixel32"):
        assert dk.trips(b[k].cl) and sum(b[k].cr) == 0, b[k].premise()
    assert [i for i, n in enumerate(b["pixel32"].cl) if n] == [3], b["pixel32"].premise()
    return b


def _report(what, pairs, words):
    for p, w in zip(pairs, words):
        print(f"[range word] {what}: {p.premise()}; read back {w}")


def _single(c, p, slot=0, fmt_imgs=None):
    """One ugsm_submit_full of pair p on `slot`; returns (result, [word])."""
    L, R = fmt_imgs if fmt_imgs is not None else (p.L, p.R)
    dL, dR = c.to_device(L), c.to_device(R)
    out = c.alloc(3 * W * H * 4)
    try:
        c.check(c.lib.ugsm_submit_full(c.handle, slot, dL, dR, W, H, L.strides[0], out))
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return c.to_host(out, (3, H, W)), c.range_words(slot, 1)
    finally:
        for q in (dL, dR, out):
            c.free(q)


def _batch(c, pairs, slot=0):
    """One ugsm_submit_full_batch of `pairs` (equal Pair objects share their device images); returns (results, words)."""
    dev = {}
    for p in pairs:
        if id(p) not in dev:
            dev[id(p)] = (c.to_device(p.L), c.to_device(p.R))
    outs = [c.alloc(3 * W * H * 4) for _ in pairs]
    try:
        c.submit_full_batch(slot, [dev[id(p)][0] for p in pairs], [dev[id(p)][1] for p in pairs], W, H, 3 * W, outs)
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return [c.to_host(o, (3, H, W)) for o in outs], c.range_words(slot, len(pairs))
    finally:
        for q in [x for pr in dev.values() for x in pr] + outs:
            c.free(q)


def _check(what, pairs, got, words):
    _report(what, pairs, words)
    for b, p in enumerate(pairs):
        assert_bit_equal(got[b], p.full, f"{what}, pair {b} ({p.name})")
    assert words == [p.word for p in pairs], f"{what}: range words {words}, the pyramids say {[p.word for p in pairs]}"


# ---- each image alone ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dark", "pixel", "pixel32", "plain"])
@pytest.mark.parametrize("slots, slot", [(1, 0), (2, 0), (2, 1)], ids=["one slot", "two slots, slot 0", "two slots, slot 1"])
def test_single_call(lib, bank, name, slots, slot):
    """A lone call: R's pyramid on the side stream (the slot's own with one slot; the neighbour slot's, borrowed, with two and nothing
    else in flight), L's on the main stream; the word is set from either and read by the main stream's K-cost launches."""
    p = bank[name]
    with lib.Context(levels=LV, slots=slots, dev=True) as c:
        got, words = _single(c, p, slot)
    _check(f"single call, slots={slots}, slot {slot}", [p], [got], words)


@pytest.mark.parametrize("two_streams", ["0", "1"])
def test_word_set_by_the_right_image_alone(lib, bank, monkeypatch, two_streams):
    """L plain, R dark: with the side stream (UGSM_TWO_STREAMS=1, the default) the only stores to the word come from the side stream, after
    the main stream's memset and before its first K-cost launch; without it (0) from the second pyramid of the one stream."""
    monkeypatch.setenv("UGSM_TWO_STREAMS", two_streams)
    p = bank["dark R"]
    with lib.Context(levels=LV, slots=1, dev=True) as c:
        got, words = _single(c, p)
        _check(f"dark R only, UGSM_TWO_STREAMS={two_streams}", [p], [got], words)
        got, words = _single(c, bank["plain"])      # ... and the next pair on the slot starts from 0 again
        _check(f"plain after dark R, UGSM_TWO_STREAMS={two_streams}", [bank["plain"]], [got], words)


def test_kernel_path_1_holds_no_word_and_stays_exact(lib, bank):
    """The one-kernel-per-stage path divides literally and keeps no word: the entry point says so instead of reporting a stale one."""
    p = bank["dark"]
    with lib.Context(levels=LV, kernel_path=1) as c:
        dL, dR = c.to_device(p.L), c.to_device(p.R)
        out = c.alloc(3 * W * H * 4)
        c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, out))
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert_bit_equal(c.to_host(out, (3, H, W)), p.full, "dark pair, kernel_path 1")
        words = (C.c_uint * 1)()
        assert c.lib.ugsm_stage_range_words(c.handle, 0, words, 1) == lib.UGSM_ERR_STATE
        for q in (dL, dR, out):
            c.free(q)
    with lib.Context(levels=LV, dev=True) as c:
        words = (C.c_uint * 17)()
        assert c.lib.ugsm_stage_range_words(c.handle, 0, words, 1) == lib.UGSM_ERR_STATE      # no call yet
        _single(c, p)
        for n in (0, 2, 17):                                                                    # the call had one pair
            assert c.lib.ugsm_stage_range_words(c.handle, 0, words, n) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_stage_range_words(c.handle, 0, None, 1) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_stage_range_words(c.handle, 3, words, 1) == lib.UGSM_ERR_BAD_ARG


# ---- every K-cost form -----------------------------------------------------------------------------------------------------------------

FORMS = {"march": {"UGSM_MARCH_MIN_PIXELS": "1"}, "march4": {"UGSM_MARCH4": "1,2000000000"}, "shared": {"UGSM_ALONE": "0"}, "alone": {"UGSM_ALONE": "1"},
         "tiled": {"UGSM_MARCH_MIN_PIXELS": "-1", "UGSM_SMALL_MAX_PIXELS": "-1", "UGSM_MARCH4": "0,0"}, "no_fused_seed": {"UGSM_FUSE_SEED": "0"}}


@pytest.mark.parametrize("force", sorted(FORMS))
def test_every_kernel_form_on_the_dark_pair(lib, bank, monkeypatch, force):
    """The dark pair and a plain one through every K-cost / K-smooth form, alone and as a batch of two.  The two marching forms read the
    word (march, march4: on every level here); the others divide literally or on their own terms and must simply stay exact on zeros,
    0 / 0 correlations and values down to 1e-8.  The word is set by the pyramid kernels whatever K-cost form follows."""
    for k, v in FORMS[force].items():
        monkeypatch.setenv(k, v)
    with lib.Context(levels=LV, slots=2, batch=2, dev=True) as c:
        got, words = _single(c, bank["dark"])
        _check(f"{force}, single call", [bank["dark"]], [got], words)
        pairs = [bank["dark"], bank["plain"]]
        got, words = _batch(c, pairs)
        _check(f"{force}, batch of two", pairs, got, words)


# ---- every live detection site ---------------------------------------------------------------------------------------------------------

def _decimate_launches(orc, counts, images, lone_full_pair):
    """Which kernel form writes each TRIPPING level (>= 3) of a launch of `images` images: launch_blur_decimate's choice restated from the
    level's output pixels -- 16 / 8 / 4 = k_blur_decimate2's strip height, 0 = k_blur_decimate_tiled (a lone full-mode pair below 1.5 M
    outputs, build_pyramids' stream_min)."""
    w, h = orc.level_dims(W, H, LV)
    forms = set()
    for i, n in enumerate(counts):
        if n and i >= 3:
            px = w[i] * h[i] * images
            forms.add(0 if (lone_full_pair and px < 1500000) else (16 if px >= 400000 else (8 if px >= 40000 else 4)))
    return forms


@pytest.mark.parametrize("site", ["tiled, forced", "tiled, a lone pair", "strips of 4", "strips of 8", "strips of 8 and 4"])
def test_every_pyramid_kernel_that_can_set_the_word(lib, orc, bank, monkeypatch, site):
    """With 8-bit input the first value below 2^-12 appears at level 3, so the sites inside k_pyr_base (levels 1, 2) cannot fire and the
    live ones are k_blur_decimate_tiled and k_blur_decimate2<16 | 8 | 4>.  One case per site, the launch each tripping level reaches
    computed from the level's size as launch_blur_decimate computes it (strips of 16: the 16 MP case below):
      tiled, forced       UGSM_PYR_STREAM=0: the tiled kernel on every level, a single call and a batch
      tiled, a lone pair  default knobs: a lone full-mode pair keeps the tiled kernel below 1.5 M outputs
      strips of 4         a single call that shares the chip (UGSM_ALONE=0): level 3 = 225 x 168 = 38 k outputs and everything below it
      strips of 8         a batch of four whose only tripping pair leaves the range at level 3 alone (4 x 38 k = 151 k outputs)
      strips of 8 and 4   the same batch with the dark pair (levels 3 .. 9)"""
    plain, plain2, dark, px32 = bank["plain"], bank["plain2"], bank["dark"], bank["pixel32"]
    if site == "tiled, forced":
        monkeypatch.setenv("UGSM_PYR_STREAM", "0")
        with lib.Context(levels=LV, slots=2, batch=4, dev=True) as c:
            got, words = _single(c, px32)
            _check(site, [px32], [got], words)
            pairs = [plain, dark, px32, plain2]
            got, words = _batch(c, pairs)
            _check(site + ", batch", pairs, got, words)
    elif site == "tiled, a lone pair":
        assert _decimate_launches(orc, px32.cl, 1, True) == {0} and _decimate_launches(orc, dark.cr, 1, True) == {0}
        with lib.Context(levels=LV, slots=1, dev=True) as c:
            for p in (px32, dark, plain2):
                got, words = _single(c, p)
                _check(site, [p], [got], words)
    elif site == "strips of 4":
        monkeypatch.setenv("UGSM_ALONE", "0")
        assert _decimate_launches(orc, px32.cl, 1, False) == {4} and _decimate_launches(orc, dark.cl, 1, False) == {4}
        with lib.Context(levels=LV, slots=1, dev=True) as c:
            for p in (px32, dark, plain2):
                got, words = _single(c, p)
                _check(site, [p], [got], words)
    else:
        trip = px32 if site == "strips of 8" else dark
        assert _decimate_launches(orc, trip.cl, 4, False) == ({8} if site == "strips of 8" else {8, 4})
        for at in (1, 3):
            pairs = [plain, plain2, plain, plain2]
            pairs[at] = trip
            with lib.Context(levels=LV, slots=1, batch=4, dev=True) as c:
                got, words = _batch(c, pairs)
            _check(f"{site}, tripping pair at {at}", pairs, got, words)


# ---- batches: one word per pair --------------------------------------------------------------------------------------------------------

def test_batch_of_four_one_word_per_pair(lib, bank):
    pairs = [bank["plain"], bank["dark"], bank["plain2"], bank["pixel"]]
    assert [p.word for p in pairs] == [0, 1, 0, 1]
    for slots in (1, 2):
        with lib.Context(levels=LV, slots=slots, batch=4, dev=True) as c:
            got, words = _batch(c, pairs, slot=slots - 1)
        _check(f"batch of four, slots={slots}", pairs, got, words)


@pytest.mark.parametrize("at", [0, 15])
def test_batch_of_sixteen_with_one_tripping_pair(lib, bank, at):
    """The word of pair `at` and of nobody else: the ends of Batch::cx."""
    pairs = [bank["plain"], bank["plain2"]] * 8
    pairs[at] = bank["pixel"]
    with lib.Context(levels=LV, slots=1, batch=16, dev=True) as c:
        got, words = _batch(c, pairs)
    _check(f"batch of sixteen, tripping pair at {at}", pairs, got, words)
    assert words == [int(b == at) for b in range(16)]


def test_batch_whose_fine_levels_run_pair_by_pair(lib, bank, monkeypatch):
    """UGSM_BATCH_MAX_PIXELS=100000: levels 0 and 1 (307 k, 153 k pixels) run pair by pair, in groups that start at pair b0 > 0 -- K-cost
    reads range_bad + b0 there -- and the levels below them as one launch for all four."""
    monkeypatch.setenv("UGSM_BATCH_MAX_PIXELS", "100000")
    for pairs in ([bank["plain"], bank["dark"], bank["plain2"], bank["pixel"]], [bank["dark"], bank["plain"], bank["pixel32"], bank["plain2"]]):
        for force in (None, "march"):
            if force:
                monkeypatch.setenv("UGSM_MARCH_MIN_PIXELS", "1")
            with lib.Context(levels=LV, slots=2, batch=4, dev=True) as c:
                got, words = _batch(c, pairs)
            _check(f"batch of four, level 0 pair by pair, {force or 'default kernels'}", pairs, got, words)
        monkeypatch.delenv("UGSM_MARCH_MIN_PIXELS")


# ---- the slot is reused ----------------------------------------------------------------------------------------------------------------

def test_slot_reuse_clears_the_words_of_the_next_call(lib, bank):
    """A dark pair, then a plain pair on the same slot WITHOUT a wait in between: the second call's memset is ordered behind the first
    call's last K-cost launch and in front of its own pyramids, on both streams -- the word ends 0, both results exact.  Then a batch of
    two behind a batch of four: the two words of the new call are cleared."""
    dark, plain, plain2, pixel = bank["dark"], bank["plain"], bank["plain2"], bank["pixel"]
    for slots in (1, 2):
        with lib.Context(levels=LV, slots=slots, batch=4, dev=True) as c:
            dev = {k: (c.to_device(bank[k].L), c.to_device(bank[k].R)) for k in ("dark", "plain", "plain2", "pixel")}
            outs = [c.alloc(3 * W * H * 4) for _ in range(6)]
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dev["dark"][0], dev["dark"][1], W, H, 3 * W, outs[0]))
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dev["plain"][0], dev["plain"][1], W, H, 3 * W, outs[1]))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            words = c.range_words(0, 1)
            _report(f"plain behind dark on one slot, slots={slots}", [plain], words)
            assert_bit_equal(c.to_host(outs[0], (3, H, W)), dark.full, "dark pair, a plain pair enqueued behind it")
            assert_bit_equal(c.to_host(outs[1], (3, H, W)), plain.full, "plain pair behind the dark pair")
            assert words == [0], f"the word of the dark pair before it is still set: {words}"
            # ... and the other way round
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dev["plain"][0], dev["plain"][1], W, H, 3 * W, outs[1]))
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dev["dark"][0], dev["dark"][1], W, H, 3 * W, outs[0]))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            assert c.range_words(0, 1) == [1]
            assert_bit_equal(c.to_host(outs[0], (3, H, W)), dark.full, "dark pair behind the plain pair")
            # a batch of four [dark, pixel, dark, plain], a batch of two [plain, dark] behind it
            four, two = [dark, pixel, dark, plain], [plain2, dark]
            name = {id(bank[k]): k for k in dev}
            c.submit_full_batch(0, [dev[name[id(p)]][0] for p in four], [dev[name[id(p)]][1] for p in four], W, H, 3 * W, outs[:4])
            c.submit_full_batch(0, [dev[name[id(p)]][0] for p in two], [dev[name[id(p)]][1] for p in two], W, H, 3 * W, outs[4:])
            c.check(c.lib.ugsm_wait(c.handle, 0))
            words = c.range_words(0, 2)
            _check(f"batch of two behind a batch of four, slots={slots}", two, [c.to_host(o, (3, H, W)) for o in outs[4:]], words)
            for b, p in enumerate(four):
                assert_bit_equal(c.to_host(outs[b], (3, H, W)), p.full, f"batch of four in front, pair {b}")
            for q in [x for pr in dev.values() for x in pr] + outs:
                c.free(q)


# ---- the queue -------------------------------------------------------------------------------------------------------------------------

def test_six_pairs_through_the_queue(lib, bank):
    """Six pairs, plain / dark alternating, through ugsm_enqueue_full on two slots with calls of up to four: every completion exact; the
    words of the last call on each slot are those of its pairs, in order."""
    seq = [bank["plain"], bank["dark"], bank["plain2"], bank["dark"], bank["plain"], bank["dark"]]
    with lib.Context(levels=LV, slots=2, batch=4, dev=True) as c:
        dev = {id(p): (c.to_device(p.L), c.to_device(p.R)) for p in seq}
        outs = [c.alloc(3 * W * H * 4) for _ in seq]
        for k, p in enumerate(seq):
            c.enqueue_full(dev[id(p)][0], dev[id(p)][1], W, H, 3 * W, outs[k], k)
        done = c.drain()
        assert [d.tag for d in done] == list(range(6))
        for k, p in enumerate(seq):
            assert_bit_equal(c.to_host(outs[k], (3, H, W)), p.full, f"queue, pair {k} ({p.name})")
        calls = {}
        for d in done:
            calls.setdefault((d.slot, d.call_index), []).append(int(d.tag))
        print(f"[range word] queue: calls {sorted(calls.items())}")
        for slot in sorted({s for s, _ in calls}):
            tags = calls[max(k for k in calls if k[0] == slot)]
            assert len(tags) == done[tags[0]].call_pairs
            words = c.range_words(slot, len(tags))
            _report(f"queue, last call on slot {slot} (pairs {tags})", [seq[t] for t in tags], words)
            assert words == [seq[t].word for t in tags]
        # one submission from page-locked host memory, one from any memory, of the dark pair
        p = bank["dark"]
        hl, hr, ho = c.host_array((H, W, 3), np.uint8), c.host_array((H, W, 3), np.uint8), c.host_array((3, H, W))
        hl[...], hr[...], ho[...] = p.L, p.R, -1.0
        c.enqueue_full_host(hl, hr, ho, 50)
        d = c.drain()
        assert [x.tag for x in d] == [50]
        assert_bit_equal(ho, p.full, "dark pair from page-locked host memory")
        assert c.range_words(d[0].slot, 1) == [1]
        c.enqueue_full_managed(p.L.copy(), p.R.copy(), 51)
        c.flush()
        d = c.next_done(True)
        assert d.tag == 51
        assert_bit_equal(np.stack(c.managed_planes(d, [(H, W)] * 3)), p.full, "dark pair, managed")
        assert c.range_words(d.slot, 1) == [1]
        c.enqueue_full_managed(bank["plain"].L.copy(), bank["plain"].R.copy(), 52)
        c.flush()
        d = c.next_done(True)
        assert_bit_equal(np.stack(c.managed_planes(d, [(H, W)] * 3)), bank["plain"].full, "plain pair, managed")
        assert c.range_words(d.slot, 1) == [0]
        assert c.next_done(True) is None
        for q in [x for pr in dev.values() for x in pr] + outs:
            c.free(q)


# ---- foveated --------------------------------------------------------------------------------------------------------------------------

F = 7
OFF_DARK, OFF_TEX = (-230, 0), (150, 40)     # the window over the dark third / over the textured part (level-0 pixels from the centre)


def _fovea_word(p):
    """Levels F-1 .. top are matched on the whole frame in foveated mode as well: an out-of-range value there lies inside a view K-cost
    reads whatever the window.  (Values of the fine levels outside the window: the word may be 1 or 0, nothing is asserted.)"""
    return int(sum(p.cl[F - 1:]) + sum(p.cr[F - 1:]) > 0)


def test_foveated_calls(lib, bank):
    dark, plain = bank["dark"], bank["plain"]
    assert _fovea_word(dark) == 1, dark.premise()
    fw, fh = lib.fovea_dims(W, H, LV, F)
    with lib.Context(levels=LV, fovea_levels=F, slots=2, batch=3, dev=True) as c:
        dev = {id(p): (c.to_device(p.L), c.to_device(p.R)) for p in (dark, plain)}
        st = [c.alloc(3 * F * fh * fw * 4) for _ in range(3)]
        for p, off, want in ((dark, OFF_DARK, 1), (dark, OFF_TEX, 1), (plain, OFF_TEX, 0), (dark, (0, 0), 1)):
            c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dev[id(p)][0], dev[id(p)][1], W, H, 3 * W, off[0], off[1], st[0], None, None))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            words = c.range_words(0, 1)
            _report(f"foveated, window at {off}", [p], words)
            assert_bit_equal(c.to_host(st[0], (3, F, fh, fw)), p.fovea(F, off), f"foveated {p.name} pair, window at {off}")
            assert words == [want]
        # a batch with both windows, a plain pair between the dark ones
        pairs, offs = [dark, plain, dark], [OFF_DARK, OFF_TEX, OFF_TEX]
        c.submit_foveated_batch(1, [dev[id(p)][0] for p in pairs], [dev[id(p)][1] for p in pairs], W, H, 3 * W, offs, st)
        c.check(c.lib.ugsm_wait(c.handle, 1))
        words = c.range_words(1, 3)
        _report("foveated batch", pairs, words)
        for b, p in enumerate(pairs):
            assert_bit_equal(c.to_host(st[b], (3, F, fh, fw)), p.fovea(F, offs[b]), f"foveated batch, pair {b} ({p.name}) at {offs[b]}")
        assert words == [1, 0, 1]
        for q in [x for pr in dev.values() for x in pr] + st:
            c.free(q)


def test_fovea_split_phases_keep_the_word(lib, bank):
    """ugsm_submit_pyramids, one ugsm_submit_fovea_coarse, two ugsm_submit_fovea_fine at different offsets, a wait between them: the fine
    phases reuse the pyramids of the first call, so their K-cost launches must still find the word those pyramids set."""
    dark, plain = bank["dark"], bank["plain"]
    fw, fh = lib.fovea_dims(W, H, LV, F)
    for p in (dark, plain):
        with lib.Context(levels=LV, fovea_levels=F, slots=2, dev=True) as c:
            dL, dR = c.to_device(p.L), c.to_device(p.R)
            state, stack = c.alloc(3 * fw * fh * 4), c.alloc(3 * F * fw * fh * 4)
            c.check(c.lib.ugsm_submit_pyramids(c.handle, 1, dL, dR, W, H, 3 * W))
            c.check(c.lib.ugsm_submit_fovea_coarse(c.handle, 1, state))
            for off in (OFF_DARK, OFF_TEX):
                c.check(c.lib.ugsm_submit_fovea_fine(c.handle, 1, state, off[0], off[1], stack))
                c.check(c.lib.ugsm_wait(c.handle, 1))
                words = c.range_words(1, 1)
                _report(f"split phases, fine at {off}", [p], words)
                assert_bit_equal(c.to_host(stack, (3, F, fh, fw)), p.fovea(F, off), f"split phases, {p.name} pair, fine at {off}")
                assert words == [p.word]          # (whole pyramids here: every level was checked, so the zero is asserted too)
            for q in (dL, dR, state, stack):
                c.free(q)


# ---- one other input format ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [en.MONO8, en.BGRA8], ids=["mono8", "bgra8"])
def test_dark_pair_in_another_input_format(lib, orc, bank, fmt):
    """The format-reading instances of k_pyr_base feed the same levels: the dark pair as mono8 and as bgra8, against the rgb8 answer on
    the image's conversion (tests/encode_np.py), whose own premise is asserted."""
    d = bank["dark"]
    iL, iR = en.encode(d.L, fmt), en.encode(d.R, fmt)
    p = Pair(orc, f"dark as {en.NAMES[fmt]}", en.to_rgb8(iL, fmt), en.to_rgb8(iR, fmt))
    assert dk.trips(p.cl) and dk.trips(p.cr), p.premise()
    with lib.Context(levels=LV, slots=1, dev=True) as c:
        c.set_input_format(fmt)
        got, words = _single(c, p, fmt_imgs=(iL, iR))
    _check(f"single call, {en.NAMES[fmt]}", [p], [got], words)


# ---- 16 MP -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dark_16mp(orc, oracle_16mp):
    """bench.py's first 16 MP pair with the dark recipe and the oracle's full-mode answer for it (one more ~3 s oracle run)."""
    g = oracle_16mp
    L, R = dk.dark_pair(g["L"], g["R"], 1601)
    orc.set_num_threads(16)
    try:
        full = orc.match_full(L, R, 14)
        word, cl, cr = dk.pair_word(orc, L, R, 14)
        pword = dk.pair_word(orc, g["L"], g["R"], 14)
    finally:
        orc.set_num_threads(8)
    return dict(L=L, R=R, full=full, word=word, cl=cl, cr=cr, plain_word=pword)


def test_16mp_four_slots_dark_and_plain_in_flight(lib, orc, oracle_16mp, dark_16mp):
    """Full mode at 4928 x 3264, four slots in flight, slots 0 and 2 dark, 1 and 3 plain.  The only place level 0's strip classes of
    k_cost_march and k_blur_decimate2<16> (level 3 = 1741 x 1153 = 2.0 M outputs, levels 4, 5 as well) run with the word set."""
    g, d = oracle_16mp, dark_16mp
    Wb, Hb = g["W"], g["H"]
    assert d["plain_word"][0] == 0 and sum(d["plain_word"][1]) + sum(d["plain_word"][2]) == 0
    assert d["word"] == 1 and dk.trips(d["cl"]) and dk.trips(d["cr"]), (d["cl"], d["cr"])
    w, h = orc.level_dims(Wb, Hb, 14)
    # level 3: above a lone call's streaming threshold as well (slot 0 is submitted onto an empty chip), so strips of 16 on all four slots
    assert d["cl"][3] > 0 and d["cr"][3] > 0 and w[3] * h[3] >= 1500000
    assert np.isfinite(d["full"]).all()
    with lib.Context(levels=14, slots=4, dev=True) as c:
        pl = (c.to_device(g["L"]), c.to_device(g["R"]))
        pd = (c.to_device(d["L"]), c.to_device(d["R"]))
        o = [c.alloc(3 * Wb * Hb * 4) for _ in range(4)]
        for s in range(4):
            src = pd if s % 2 == 0 else pl
            c.check(c.lib.ugsm_submit_full(c.handle, s, src[0], src[1], Wb, Hb, 3 * Wb, o[s]))
        c.check(c.lib.ugsm_wait_all(c.handle))
        words = [c.range_words(s, 1)[0] for s in range(4)]
        print(f"[range word] 16 MP: dark pair out-of-range values per level L {d['cl']} R {d['cr']}; plain pair none; words of slots 0-3 read back {words}")
        for s in range(4):
            assert_bit_equal(c.to_host(o[s], (3, Hb, Wb)), d["full"] if s % 2 == 0 else g["full"], f"16 MP, slot {s} ({'dark' if s % 2 == 0 else 'plain'}) vs oracle")
        assert words == [1, 0, 1, 0]
        for q in list(pl) + list(pd) + o:
            c.free(q)


# ---- degenerate pairs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(160, 120, 8), (333, 251, 10)], ids=["160x120", "333x251"])
def test_degenerate_pairs_on_both_kernel_paths(lib, orc, size):
    """All 0, all 255, constant 7, one image black: every pyramid value is 0 or in range (words 0), every correlation 0 / 0 or 1, and the
    result is exact and finite on the fused path (single call and one batch of all five) and on the one-kernel-per-stage path."""
    from ug_stereomatcher_amd import synth
    w, h, lv = size
    pairs = dk.degenerate_pairs(*synth.make_pair(w, h, synth.BASE_SEED + 612)[:2])
    exp = {}
    for k, (L, R) in pairs.items():
        assert dk.pair_word(orc, L, R, lv)[0] == 0, k
        exp[k] = orc.match_full(L, R, lv)
        assert np.isfinite(exp[k]).all(), k
    for kernel_path in (0, 1):
        with lib.Context(levels=lv, kernel_path=kernel_path, slots=2, batch=5, dev=True) as c:
            dev = {k: (c.to_device(L), c.to_device(R)) for k, (L, R) in pairs.items()}
            outs = [c.alloc(3 * w * h * 4) for _ in pairs]
            for k in pairs:
                c.check(c.lib.ugsm_submit_full(c.handle, 0, dev[k][0], dev[k][1], w, h, 3 * w, outs[0]))
                c.check(c.lib.ugsm_wait(c.handle, 0))
                assert_bit_equal(c.to_host(outs[0], (3, h, w)), exp[k], f"{w}x{h} {k}, kernel_path {kernel_path}")
                if kernel_path == 0:
                    assert c.range_words(0, 1) == [0], k
            c.submit_full_batch(1, [dev[k][0] for k in pairs], [dev[k][1] for k in pairs], w, h, 3 * w, outs)
            c.check(c.lib.ugsm_wait(c.handle, 1))
            for b, k in enumerate(pairs):
                assert_bit_equal(c.to_host(outs[b], (3, h, w)), exp[k], f"{w}x{h} {k}, batch of five, kernel_path {kernel_path}")
            if kernel_path == 0:
                assert c.range_words(1, 5) == [0] * 5
            for q in [x for pr in dev.values() for x in pr] + outs:
                c.free(q)
