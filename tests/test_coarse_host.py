"""The full-mode call in two halves (ugsm_submit_full_coarse, ugsm_submit_full_fine, ugsm_match_full_coarse, ugsm_match_full_fine,
ugsm_stage_prolong, ugsm_coarse_pixel_iterations) without a GPU: the numpy prolongation against the chain of oracle seed steps; the oracle
composition the GPU tests compare with against orc.match_full; every refusal of the calls, driven through the real csrc/ugsm_coarse.cpp over the
recording stand-in runtime (tests/fake_runtime.cpp, unchanged, plus tests/fake_coarse.cpp); the size identity; the exports, the bindings, the
shims, the documents."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import coarse_np as cn
import seeded_np as sn
from conftest import ROOT, assert_bit_equal
from test_gpu_seeded import _special_field

NAMES = ("ugsm_submit_full_coarse", "ugsm_submit_full_fine", "ugsm_match_full_coarse", "ugsm_match_full_fine", "ugsm_stage_prolong",
         "ugsm_coarse_pixel_iterations")
OK, BAD_ARG, SIZE_MISMATCH, STATE = 0, 1, 2, 7
W, H, LEVELS = 333, 251, 14


def _field(w, h, seed):
    """_special_field of the seeded GPU tests (NaN, +-inf, +-3e38, denormals, -0.0), cropped where a level is smaller than its 3 x 3 corner."""
    return np.ascontiguousarray(_special_field(max(w, 3), max(h, 3), seed)[:, :h, :w])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


# ---- 1. the prolongation in numpy --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,levels", [(333, 251, 14), (231, 211, 14), (67, 49, 9)], ids=["333x251", "231x211", "67x49-nine-levels"])
def test_prolong_np_equals_the_chain_of_oracle_seed_steps(orc, w, h, levels):
    lw, lh = orc.level_dims(w, h, levels)
    for e in range(levels):
        f = _field(lw[e], lh[e], 9300 + 17 * e + w)
        chain = f
        for l in range(e - 1, -1, -1):
            chain = orc.seed(chain, lw[l], lh[l])
        got = cn.prolong_np(f, (lw[:e + 1], lh[:e + 1]))
        assert got.shape == (3, h, w)
        assert_bit_equal(got, chain, f"{w}x{h}, level {e}")
    f0 = _field(w, h, 1)
    assert_bit_equal(cn.prolong_np(f0, (lw[:1], lh[:1])), f0, "level 0 is a copy")


def test_the_per_level_clamp_binds_where_the_header_says():
    """The steps (numbered by the finer level) on which tex's clamp changes a site: no closed form carries them."""
    def binding(n):
        d = [n]
        while len(d) < 14:
            d.append(int(d[-1] / sn.SCALE))
        return [l for l in range(13) if cn.clamp_binds(d[l], d[l + 1])]
    assert binding(333) == [0, 2, 3, 4, 7, 8, 10, 12]
    assert binding(4928) == [0, 1, 2, 4, 6, 7, 8, 9, 10, 11]


# ---- 2. the oracle composition -----------------------------------------------------------------------------------------------------------

def test_coarse_then_fine_is_match_full_and_another_state_moves_the_field(orc):
    from ug_stereomatcher_amd import synth
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 7300)[:2]
    L2, R2 = synth.make_pair(W, H, synth.BASE_SEED + 7301)[:2]
    cold = orc.match_full(L, R, LEVELS)
    pyr, pyr2 = sn.pyramids(orc, L, R, LEVELS), sn.pyramids(orc, L2, R2, LEVELS)
    lw, lh = orc.level_dims(W, H, LEVELS)
    assert_bit_equal(cn.coarse_oracle(orc, L, R, 0, LEVELS, pyr), cold, "coarse_oracle at level 0 is the whole call")
    for e in (1, 2, 5, 13):
        state = cn.coarse_oracle(orc, L, R, e, LEVELS, pyr)
        assert state.shape == (3, lh[e], lw[e])
        assert_bit_equal(cn.fine_oracle(orc, L, R, state, e, LEVELS, pyr), cold, f"fine(coarse({e}))")
        other = cn.fine_oracle(orc, L, R, cn.coarse_oracle(orc, L2, R2, e, LEVELS, pyr2), e, LEVELS, pyr)
        moved = np.abs(other[:2].astype(np.float64) - cold[:2]).mean()
        print(f"state level {e}: mean |fine(another pair's state) - cold| = {moved:.3f} px")
        assert not np.array_equal(other.view(np.uint32), cold.view(np.uint32)), f"premise, level {e}: another pair's state gives the cold field"


# ---- 3. the sizes ------------------------------------------------------------------------------------------------------------------------

def test_coarse_plus_the_rest_is_the_whole_call(lib):
    so = lib.load()
    for (w_, h_) in [(333, 251), (1920, 1080), (4928, 3264)]:
        w, h = lib.level_dims(w_, h_, LEVELS)
        whole = lib.pixel_iterations(w_, h_, LEVELS, 0)
        assert lib.coarse_pixel_iterations(w_, h_, LEVELS, 0) == whole
        for e in range(LEVELS):
            assert lib.coarse_pixel_iterations(w_, h_, LEVELS, e) == sum(w[i] * h[i] * lib.level_iterations(i) for i in range(e, LEVELS)), (w_, h_, e)
            if e >= 1:
                assert lib.coarse_pixel_iterations(w_, h_, LEVELS, e) + lib.seeded_pixel_iterations(w_, h_, LEVELS, e - 1) == whole, (w_, h_, e)
        assert so.ugsm_coarse_pixel_iterations(w_, h_, LEVELS, LEVELS) == -1 and so.ugsm_coarse_pixel_iterations(w_, h_, LEVELS, -1) == -1
    assert so.ugsm_coarse_pixel_iterations(0, 10, 3, 0) == -1 and so.ugsm_coarse_pixel_iterations(64, 48, 14, 0) == -1
    assert so.ugsm_coarse_pixel_iterations(64, 48, 40, 0) == -1


# ---- 4. every refusal, over the stand-in runtime -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fakecoarse") / "libugsm_coarse_fake.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fvisibility=hidden",
           os.path.join(ROOT, "tests", "fake_runtime.cpp"), os.path.join(ROOT, "tests", "fake_coarse.cpp"),
           os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm_coarse.cpp"),
           "-Wl,--version-script=" + os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm.map"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    so = C.CDLL(out, mode=os.RTLD_NOW)
    vp, i, pp = C.c_void_p, C.c_int, C.POINTER(C.c_void_p)
    so.ugsm_fake_create.restype = vp
    so.ugsm_fake_create.argtypes = [i, i, i, i]
    so.ugsm_fake_destroy.argtypes = [vp]
    so.ugsm_fake_destroy.restype = None
    so.ugsm_fake_coarse_lr.argtypes = [C.c_float, i]
    so.ugsm_fake_coarse_early_exit.argtypes = [vp, C.c_float]
    so.ugsm_fake_coarse_queue_busy.argtypes = [vp, i]
    so.ugsm_fake_coarse_input_format.argtypes = [vp, i]
    so.ugsm_fake_coarse_reached.argtypes = [C.POINTER(i * 9)]
    so.ugsm_submit_full_coarse.argtypes = [vp, i, i, pp, pp, i, i, i, i, pp, pp]
    so.ugsm_submit_full_fine.argtypes = [vp, i, i, pp, pp, i, i, i, pp, i, pp]
    so.ugsm_match_full_coarse.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp]
    so.ugsm_match_full_fine.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, i, vp, vp, vp]
    so.ugsm_coarse_pixel_iterations.argtypes = [i, i, i, i]
    so.ugsm_coarse_pixel_iterations.restype = C.c_longlong
    so.ugsm_level_dims.argtypes = [i, i, i, C.POINTER(i), C.POINTER(i)]
    so.ugsm_last_error.argtypes = [vp]
    so.ugsm_last_error.restype = C.c_char_p
    return so


def _reached(fake):
    v = (C.c_int * 9)()
    fake.ugsm_fake_coarse_reached(C.byref(v))
    return list(v)


BASE = 0x7F0000000000
ROOM = 1 << 24          # far more than a 64 x 48 field: the stand-in pointers of one array do not overlap


def _ptrs(n, base=BASE, hole=None):
    return (C.c_void_p * max(n, 1))(*[None if k == hole else base + ROOM * k for k in range(max(n, 1))])


def test_every_status_before_the_runtime_is_reached(fake):
    ctx = fake.ugsm_fake_create(1, 3, 14, 7)
    try:
        fake.ugsm_fake_coarse_lr(0.0, 0)

        def arrays(n, given):
            out = [_ptrs(n, BASE + (j << 36)) if a is None else a for j, a in enumerate(given)]
            return [None if a is False else a for a in out]

        def coarse(n=3, W_=64, H_=48, stride=192, level=5, L=None, R=None, S=None, F=None, c=ctx):
            L, R, S, F = arrays(n, (L, R, S, F))
            return fake.ugsm_submit_full_coarse(c, 0, n, L, R, W_, H_, stride, level, S, F)

        def fine(n=3, W_=64, H_=48, stride=192, level=5, L=None, R=None, S=None, O=None, c=ctx):
            L, R, S, O = arrays(n, (L, R, S, O))
            return fake.ugsm_submit_full_fine(c, 0, n, L, R, W_, H_, stride, S, level, O)

        def mcoarse(W_=64, H_=48, stride=192, level=5, hole=(), c=ctx):
            a = [None if k in hole else BASE + ROOM * k for k in range(8)]
            return fake.ugsm_match_full_coarse(c, a[0], a[1], W_, H_, stride, level, *a[2:8])

        def mfine(W_=64, H_=48, stride=192, level=5, hole=(), c=ctx):
            a = [None if k in hole else BASE + ROOM * k for k in range(8)]
            return fake.ugsm_match_full_fine(c, a[0], a[1], W_, H_, stride, a[2], a[3], a[4], level, a[5], a[6], a[7])

        before = _reached(fake)
        # null context, null arrays, null entries; d_full alone may be null, and so may its entries
        assert coarse(c=None) == BAD_ARG and fine(c=None) == BAD_ARG and mcoarse(c=None) == BAD_ARG and mfine(c=None) == BAD_ARG
        for which in range(3):
            args = [None] * 4
            args[which] = False
            assert coarse(L=args[0], R=args[1], S=args[2]) == BAD_ARG, which
            args[which] = _ptrs(3, hole=1)
            assert coarse(L=args[0], R=args[1], S=args[2]) == BAD_ARG, which
        for which in range(4):
            args = [None] * 4
            args[which] = False
            assert fine(L=args[0], R=args[1], S=args[2], O=args[3]) == BAD_ARG, which
            args[which] = _ptrs(3, hole=1)
            assert fine(L=args[0], R=args[1], S=args[2], O=args[3]) == BAD_ARG, which
        for hole in range(5):
            assert mcoarse(hole=(hole,)) == BAD_ARG, hole
        for hole in ((5,), (6,), (7,), (5, 6), (6, 7)):           # the three full planes, or none
            assert mcoarse(hole=hole) == BAD_ARG, hole
        for hole in range(8):
            assert mfine(hole=(hole,)) == BAD_ARG, hole
        # n and the levels out of range; state_level 0 is no state
        for n in (0, -1, 17):
            assert coarse(n=n) == BAD_ARG and fine(n=n) == BAD_ARG, n
        for level in (-1, 14, 100):
            assert coarse(level=level) == BAD_ARG and mcoarse(level=level) == BAD_ARG, level
        assert b"stop_level" in fake.ugsm_last_error(ctx)
        for level in (-1, 0, 14, 100):
            assert fine(level=level) == BAD_ARG and mfine(level=level) == BAD_ARG, level
        assert b"state_level" in fake.ugsm_last_error(ctx)
        # the early exit
        fake.ugsm_fake_coarse_early_exit(ctx, 0.02)
        assert coarse() == BAD_ARG and fine() == BAD_ARG and mcoarse() == BAD_ARG and mfine() == BAD_ARG
        assert b"early_exit_threshold" in fake.ugsm_last_error(ctx)
        fake.ugsm_fake_coarse_early_exit(ctx, 0.0)
        # a d_full entry over a state of the call -- its own pair's or another's; level 5 of 64 x 48 is 11 x 8: 3 * 88 floats
        lw, lh = (C.c_int * 32)(), (C.c_int * 32)()
        assert fake.ugsm_level_dims(64, 48, 14, lw, lh) == OK
        state_bytes, full_bytes = 3 * lw[5] * lh[5] * 4, 3 * 64 * 48 * 4
        S = _ptrs(3, BASE)
        for k, at in ((0, S[0]), (1, S[2] + state_bytes - 4), (2, S[0] - full_bytes + 4)):
            Fk = (C.c_void_p * 3)(None, None, None)
            Fk[k] = at
            assert coarse(S=S, F=Fk) == BAD_ARG, (k, hex(at))
            assert b"overlaps" in fake.ugsm_last_error(ctx)
        # the full-mode LR check in force: a state, not an argument; the foveated check alone does not matter
        fake.ugsm_fake_coarse_lr(1.0, 1)
        assert coarse() == STATE and fine() == STATE and mcoarse() == STATE and mfine() == STATE
        fake.ugsm_fake_coarse_lr(1.0, 3)
        assert coarse() == STATE
        # pairs outstanding in the queue
        fake.ugsm_fake_coarse_lr(0.0, 0)
        fake.ugsm_fake_coarse_queue_busy(ctx, 1)
        assert coarse() == STATE and fine() == STATE and mcoarse() == STATE and mfine() == STATE
        fake.ugsm_fake_coarse_queue_busy(ctx, 0)
        # size errors, as ugsm_submit_full: no such size, a stride below the format's row
        assert coarse(W_=0) == BAD_ARG and mfine(H_=-4) == BAD_ARG
        assert coarse(stride=191) == SIZE_MISMATCH and fine(stride=191) == SIZE_MISMATCH and mcoarse(stride=191) == SIZE_MISMATCH
        assert _reached(fake) == before, "a refused call reached the runtime"
        # ... and the accepted ones did, with their arguments
        fake.ugsm_fake_coarse_lr(1.0, 2)
        assert coarse() == OK and _reached(fake)[4:] == [0, 3, 64, 5, 3]
        fake.ugsm_fake_coarse_lr(0.0, 1)
        fake.ugsm_fake_coarse_input_format(ctx, 2)          # rgba8: four bytes per pixel
        assert coarse(stride=255) == SIZE_MISMATCH and coarse(stride=256, F=False) == OK and _reached(fake)[4:] == [0, 3, 64, 5, 0]
        fake.ugsm_fake_coarse_input_format(ctx, 0)
        Fk = (C.c_void_p * 3)(None, S[2] + state_bytes, None)       # just behind the last state: no overlap; one entry of three
        assert coarse(S=S, F=Fk, level=5) == OK and _reached(fake)[4:] == [0, 3, 64, 5, 1]
        assert coarse(n=16, level=0, F=False) == OK and _reached(fake)[4:] == [0, 16, 64, 0, 0]
        assert coarse(n=1, level=13) == OK and _reached(fake)[4:] == [0, 1, 64, 13, 1]
        assert fine(n=16, level=1) == OK and _reached(fake)[4:] == [0, 16, 64, 1, 0]
        assert fine(n=1, level=13) == OK and _reached(fake)[4:] == [0, 1, 64, 13, 0]
        assert mcoarse(level=0) == OK and _reached(fake)[4:] == [0, 1, 64, 0, 1]
        assert mcoarse(level=13, hole=(5, 6, 7)) == OK and _reached(fake)[4:] == [0, 1, 64, 13, 0]
        assert mfine(level=13) == OK and _reached(fake)[4:] == [0, 1, 64, 13, 0]
        after = _reached(fake)
        assert [after[k] - before[k] for k in range(4)] == [5, 2, 2, 1]
    finally:
        fake.ugsm_fake_destroy(ctx)


def test_the_size_function_over_the_stand_ins_own_geometry(fake):
    w, h = (C.c_int * 32)(), (C.c_int * 32)()
    assert fake.ugsm_level_dims(640, 480, 9, w, h) == OK
    assert fake.ugsm_coarse_pixel_iterations(640, 480, 9, 4) == sum(w[i] * h[i] * (2 + i) for i in range(4, 9))


# ---- 5. exports, bindings, shims, documents ----------------------------------------------------------------------------------------------

def test_the_header_is_plain_c99_with_the_names(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ugsm.h"
        assert not any(word in name for word in ("seeded", "restrict", "warm")), name
    src = tmp_path / "use.c"
    src.write_text('#include "ugsm.h"\n'
                   "long long use(ugsm_ctx *c, const uint8_t *const *l, const float *const *s, float *const *o, const uint8_t *h, float *f)\n"
                   "{\n"
                   "    return ugsm_submit_full_coarse(c, 0, 1, l, l, 64, 48, 192, 5, o, 0) + ugsm_submit_full_fine(c, 0, 1, l, l, 64, 48, 192, s, 5, o)\n"
                   "           + ugsm_match_full_coarse(c, h, h, 64, 48, 192, 5, f, f, f, 0, 0, 0) + ugsm_match_full_fine(c, h, h, 64, 48, 192, f, f, f, 5, f, f, f)\n"
                   "           + ugsm_stage_prolong(c, f, 64, 48, 5, f) + ugsm_coarse_pixel_iterations(64, 48, 3, 1);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert re.search(r"#define UGSM_ABI_VERSION 6\b", hdr), "additions only: the ABI number stays"
    said = hdr.split("int ugsm_submit_full_coarse(")[0].rsplit("NOT built:", 1)[1]
    for what in ("queue or managed form", "page-locked _host kind", "checked or seeded coarse call", "node's use of it", "clouds straight from a level-sized state"):
        assert what in said, what
    abi = hdr.split("the full-mode call in two halves --", 1)[1].split("6: the kernel choices", 1)[0]
    for name in NAMES:
        assert name in abi, f"{name}: the ABI comment's list of additions"


def test_both_libraries_export_them(lib):
    for name in NAMES:
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(rf" T {name}$", dyn, re.M), f"{name} is not a dynamic symbol of {os.path.basename(path)}"
    so = lib.load()
    assert so.ugsm_abi_version() == 6
    assert len(so.ugsm_submit_full_coarse.argtypes) == 11 and len(so.ugsm_submit_full_fine.argtypes) == 11
    assert len(so.ugsm_match_full_coarse.argtypes) == 13 and len(so.ugsm_match_full_fine.argtypes) == 13 and len(so.ugsm_stage_prolong.argtypes) == 6


def test_a_null_context_is_a_status_code(lib):
    for dev in (False, True):
        so = lib.load(dev)
        ptrs = (C.c_void_p * 1)(None)
        assert so.ugsm_submit_full_coarse(None, 0, 1, ptrs, ptrs, 64, 48, 192, 5, ptrs, None) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_submit_full_fine(None, 0, 1, ptrs, ptrs, 64, 48, 192, ptrs, 5, ptrs) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_match_full_coarse(None, None, None, 64, 48, 192, 5, None, None, None, None, None, None) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_match_full_fine(None, None, None, 64, 48, 192, None, None, None, 5, None, None, None) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_stage_prolong(None, None, 64, 48, 5, None) == lib.UGSM_ERR_BAD_ARG


class _FakeLib:
    """Stands in for the loaded library: records what the Context methods hand to the C calls."""

    def __init__(self):
        self.calls = []

    def _record(self, *args):
        self.calls.append(args)
        return 0

    ugsm_submit_full_coarse = ugsm_submit_full_fine = ugsm_stage_prolong = _record


def test_the_python_binding_marshals_its_lists(lib):
    c = object.__new__(lib.Context)
    c._h, c.lib = 1234, _FakeLib()
    c.submit_full_coarse(1, [10, 20, 30], [11, 21, 31], 64, 48, 192, 5, [12, 22, 32], [13, None, 33])
    c.submit_full_coarse(0, [10], [11], 64, 48, 200, 0, [12])
    (h, slot, n, dl, dr, W_, H_, stride, level, ds, df), second = c.lib.calls
    assert (h, slot, n, W_, H_, stride, level) == (1234, 1, 3, 64, 48, 192, 5)
    assert list(dl) == [10, 20, 30] and list(dr) == [11, 21, 31] and list(ds) == [12, 22, 32] and list(df) == [13, None, 33]
    assert second[2] == 1 and second[7] == 200 and second[8] == 0 and list(second[9]) == [12] and second[10] is None
    c.submit_full_fine(2, [10, 20], [11, 21], 64, 48, 192, [12, 22], 5, [13, 23])
    h, slot, n, dl, dr, W_, H_, stride, ds, level, do = c.lib.calls[-1]
    assert (h, slot, n, level) == (1234, 2, 2, 5) and list(ds) == [12, 22] and list(do) == [13, 23]
    for bad in (([10, 20], [11], [12, 22], [13, 23]), ([10, 20], [11, 21], [12], [13, 23]), ([10, 20], [11, 21], [12, 22], [13])):
        with pytest.raises(lib.UgsmError):
            c.submit_full_coarse(0, bad[0], bad[1], 64, 48, 192, 5, bad[2], bad[3])
        with pytest.raises(lib.UgsmError):
            c.submit_full_fine(0, bad[0], bad[1], 64, 48, 192, bad[2], 5, bad[3])
    assert len(c.lib.calls) == 3
    c.stage_prolong(77, 64, 48, 3, 88)
    assert c.lib.calls[-1] == (1234, 77, 64, 48, 3, 88)


def test_the_python_mirror_and_the_shims_expose_the_calls(lib):
    for method in ("submit_full_coarse", "submit_full_fine", "stage_prolong", "match_full_coarse", "match_full_fine"):
        assert hasattr(lib.Context, method), method
    assert list(inspect.signature(lib.Context.submit_full_coarse).parameters)[-3:] == ["stop_level", "d_state", "d_full"]
    assert list(inspect.signature(lib.Context.submit_full_fine).parameters)[-3:] == ["d_state", "state_level", "d_out"]
    assert callable(lib.coarse_pixel_iterations)
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    assert list(inspect.signature(MatchGPULib.matchCoarse).parameters) == ["self", "cv_ptrL", "cv_ptrR", "stop_level", "want_full"]
    assert inspect.signature(MatchGPULib.matchCoarse).parameters["want_full"].default is False
    assert list(inspect.signature(MatchGPULib.matchFine).parameters) == ["self", "cv_ptrL", "cv_ptrR", "state", "state_level"]
    shim = open(os.path.join(ROOT, "ros", "MatchGPULib_ugsm.hpp")).read()
    assert "float **matchCoarse(ImgPtr L, ImgPtr R, int stop_level, float ***full = nullptr)" in shim and "ugsm_match_full_coarse(ctx_," in shim
    assert "float **matchFine(ImgPtr L, ImgPtr R, float *const *state, int state_level)" in shim and "ugsm_match_full_fine(ctx_," in shim


def test_the_shim_compiles_with_the_two_methods(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "ros", "shim_selftest.cpp"), "-o", str(tmp_path / "shim_selftest.o")])
    assert "m.matchCoarse(L, R, 5" in open(os.path.join(ROOT, "ros", "shim_selftest.cpp")).read()


def test_the_prolongation_is_k_prolong_and_a_class_of_the_statistics():
    """The prolongation is a kernel of its own name, k_prolong (ugsm_kernels_fields.hip), which is also its class in the kernel statistics;
    k_copy_view (ugsm_kernels_aux.hip) is the one operation of that name.  No LDS, no atomics, no preprocessor conditional in the kernel file."""
    csrc = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")
    fields = open(os.path.join(csrc, "ugsm_kernels_fields.hip")).read()
    aux = open(os.path.join(csrc, "ugsm_kernels_aux.hip")).read()
    assert len(re.findall(r"__global__[^\n]*\bvoid k_prolong\(", fields)) == 1
    assert len(re.findall(r"__global__[^\n]*\bvoid k_copy_view\(", aux)) == 1 and aux.count("k_copy_view(") == 1
    assert "ProlongMap pm" in fields and "bool launch_prolong(" in fields
    body = fields.split("void prolong_row(", 1)[1].split("bool launch_prolong(", 1)[0]
    assert "ProlongMap pm" in body and "void k_prolong(" in body
    assert "__shared__" not in body and "atomic" not in body
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", fields + aux, re.M)
    assert '"k_prolong"' in open(os.path.join(csrc, "ugsm_runtime.cpp")).read()
    assert "ugsm_coarse.cpp" in open(os.path.join(csrc, "Makefile")).read()


def test_the_documents_carry_the_calls():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text, what in ((integ, "INTEGRATION.md"), (design, "DESIGN.md"), (readme, "README.md")):
        assert "ugsm_submit_full_coarse" in text and "ugsm_submit_full_fine" in text, what
    assert "The call in two halves" in design and "coarse_bench" in design
