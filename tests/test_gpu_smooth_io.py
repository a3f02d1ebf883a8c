"""K-smooth's load and copy-out phases (k_smooth_fused, csrc/ugsm_kernels_smooth.hip) against the CPU oracle, bit for bit, NaNs at the same
places: the tiles inside the image move by quads (16-byte loads and stores, aligned when the width is a multiple of four, at 4-byte
alignment otherwise), the tiles on the frame cell by cell.  Sizes so that every branch runs in each of the three tile classes: widths
with W % 4 = 0, 1, 2, 3; a frame smaller than one tile, exactly one tile, several tiles with interior and frame tiles in both directions;
0..5 passes with and without the box; the 112-column tile at 16, 20 and 36 rows; a batched call whose level 0 is one launch for three
pairs; the last launch writing the caller's buffer directly."""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

BIG = str(1 << 30)
# the tile class by the development thresholds (read at ugsm_create under UGSM_DEV=1); UGSM_SMALL_MASK=1: no k_smooth_small, so
# that every size runs k_smooth_fused
CLASS_ENV = {
    "112": {"UGSM_SMOOTH_BIG_MIN": "1", "UGSM_SMALL_MASK": "1"},
    "64x32": {"UGSM_SMOOTH_BIG_MIN": BIG, "UGSM_SMOOTH_MID_MIN": "1", "UGSM_SMALL_MASK": "1"},
    "32x16": {"UGSM_SMOOTH_BIG_MIN": BIG, "UGSM_SMOOTH_MID_MIN": BIG, "UGSM_SMALL_MASK": "1"},
}
# (smaller than one tile, exactly one tile, several tiles with interior ones; W % 4 = 0, 1, 2, 3 among the multi-tile sizes)
SIZES = {
    "112": [(100, 30), (112, 36), (448, 150), (450, 152), (1233, 300), (1235, 815), (2464, 1632)],
    "64x32": [(50, 20), (64, 32), (448, 150), (450, 152), (617, 409), (903, 577)],   # (below 2^19 pixels: the launcher's own bound of the class)
    "32x16": [(20, 10), (32, 16), (127, 53), (448, 150), (450, 152), (617, 409)],
}
COMBOS = [(p, b) for b in (0, 1) for p in range(6) if p or b]  # (0 passes + box is a launch the stage entry point makes)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def field(W, H, seed):
    """dx, dy, confidence with what the passes treat specially: confidences of 0 (sums of 0: the literal-division redo), negative and
    tiny ones, a NaN; patches at the frame, in the middle and across tile edges."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = np.stack([rng.normal(0, 3, (H, W)), rng.normal(0, 3, (H, W)), 0.1 + 0.9 * rng.random((H, W))]).astype(np.float32)
    d[2, H // 3:H // 3 + 9, W // 4:W // 4 + 40] = 0.0
    d[2, 0:5, 0:7] = 0.0
    d[2, max(H - 6, 0):, max(W - 9, 0):] = 0.0
    d[2, H // 2:H // 2 + 3, W // 2:W // 2 + 30] = -0.25
    d[2, (2 * H) // 3:(2 * H) // 3 + 3, W // 8:W // 8 + 30] = 1e-30
    d[0, H // 2, W // 3] = np.nan
    d[2, (3 * H) // 4, (3 * W) // 4] = np.nan
    return d


def expected(orc, d):
    """{(passes, box): field} for every launch shape of COMBOS."""
    exp = {}
    cur = d
    with np.errstate(all="ignore"):
        for p in range(6):
            if p:
                cur = orc.smooth_pass(cur)
                exp[(p, 0)] = cur
            exp[(p, 1)] = orc.box3(cur)
    return exp


def run_sizes(lib, orc, sizes, what, big=None):
    """big: True / False = the plan must (not) name the 112-column tile for every size (that the environment did set the class)."""
    for k, (W, H) in enumerate(sizes):
        plan = lib.plan_level(W, H, alone=True)
        if big is not None:
            assert plan["smooth_kernel"] == 0 and (plan["smooth_tile_rows"] > 0) == big, f"{what} {W}x{H}: {plan}"
        d = field(W, H, 7000 + k)
        exp = expected(orc, d)
        with lib.Context(levels=1, slots=1) as c:
            for passes, box in COMBOS:
                p = c.to_device(d)
                c.check(c.lib.ugsm_stage_smooth(c.handle, p, W, H, passes, box))
                got = c.to_host(p, d.shape)
                c.free(p)
                assert_bit_equal(got, exp[(passes, box)], f"{what} {W}x{H} passes={passes} box={box}")


@pytest.mark.parametrize("cls", ["112", "64x32", "32x16"])
def test_smooth_io_every_tile_class(lib, orc, monkeypatch, cls):
    for k, v in CLASS_ENV[cls].items():
        monkeypatch.setenv(k, v)
    if cls == "112":
        monkeypatch.setenv("UGSM_SMOOTH_ROWS", "36")  # the fixed-height instance; the other heights below
    run_sizes(lib, orc, SIZES[cls], f"class {cls}", big=cls == "112")


@pytest.mark.parametrize("rows", ["16", "20", "0"])
def test_smooth_io_tile_heights(lib, orc, monkeypatch, rows):
    """The 112-column tile's variable-height instance (UGSM_SMOOTH_ROWS as test_smooth_tile_heights sets it; 0 = the context's policy)."""
    for k, v in CLASS_ENV["112"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("UGSM_SMOOTH_ROWS", rows)
    run_sizes(lib, orc, [(100, 30), (448, 150), (1235, 815), (1234, 301)], f"rows={rows}", big=True)


def test_smooth_io_default_classes(lib, orc):
    """The classes the thresholds pick by themselves."""
    run_sizes(lib, orc, [(127, 53), (617, 409), (1235, 815)], "default")


@pytest.mark.parametrize("cls", ["112", "64x32", "default"])
def test_smooth_io_batch_and_direct_output(lib, orc, monkeypatch, cls):
    """Three pairs in one call whose level 0 is ONE launch for all of them (blockIdx.y picks the pair), every pair's last launch writing
    the caller's buffer; then one pair alone, the same way."""
    from ug_stereomatcher_amd import synth
    for k, v in CLASS_ENV.get(cls, {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("UGSM_BATCH_MAX_PIXELS", "20000000")
    W, H, lv = 450, 302, 6
    pairs = [synth.make_pair(W, H, synth.BASE_SEED + 7100 + j)[:2] for j in range(3)]
    refs = [orc.match_full(L, R, lv) for (L, R) in pairs]
    with lib.Context(levels=lv, batch=3) as c:
        dL, dR = [c.to_device(a) for a, _ in pairs], [c.to_device(b) for _, b in pairs]
        dO = [c.alloc(3 * W * H * 4) for _ in pairs]
        c.submit_full_batch(0, dL, dR, W, H, 3 * W, dO)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        got = [c.to_host(p, (3, H, W)) for p in dO]
        c.submit_full_batch(0, dL[1:2], dR[1:2], W, H, 3 * W, dO[:1])
        c.check(c.lib.ugsm_wait(c.handle, 0))
        alone = c.to_host(dO[0], (3, H, W))
        for p in dL + dR + dO:
            c.free(p)
    for j in range(3):
        assert_bit_equal(got[j], refs[j], f"{cls}: pair {j} of a batch of three, {W}x{H}")
    assert_bit_equal(alone, refs[1], f"{cls}: one pair, {W}x{H}")
