"""The seeded (warm) foveated call (ugsm_submit_foveated_warm, ugsm_submit_foveated_warm_field, ugsm_match_foveated_warm, ugsm_stage_warm_stack,
ugsm_fovea_warm_pixel_iterations) without a GPU: the two numpy statements of the starting fields against each other; the premises of the GPU
tests from the oracle alone; every refusal of the call, driven through the real csrc/ugsm_fovea_seeded.cpp over the recording stand-in runtime
(tests/fake_runtime.cpp, unchanged, plus tests/fake_fovea_seeded.cpp); the size of a warm call; the exports, the bindings, the shims, the documents."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fovea_seeded_np as fs
import launch_census as lc
from conftest import ROOT, assert_bit_equal

NAMES = ("ugsm_submit_foveated_warm", "ugsm_submit_foveated_warm_field", "ugsm_match_foveated_warm", "ugsm_stage_warm_stack",
         "ugsm_fovea_warm_pixel_iterations")
OK, BAD_ARG, SIZE_MISMATCH, STATE = 0, 1, 2, 7
W, H, LEVELS, F = lc.W, lc.H, lc.LEVELS, lc.F


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


# ---- 1. the starting fields: two statements ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(333, 251), (231, 211)])
@pytest.mark.parametrize("F_", [7, 2, LEVELS], ids=["F7", "F2", "F-is-levels"])
def test_the_pointwise_recursion_is_reconstruct_restrict_crop(orc, w, h, F_):
    fw, fh = orc.fovea_geometry(w, h, LEVELS, F_)[:2]
    prior = fs.special_stack(F_, fh, fw, 4100 + w + F_)
    offs = lc.OFFS3
    cases = [(p, n) for p in offs for n in offs]            # equal offsets, moved windows, and both clamped into a corner
    assert ((5000, -5000), (5000, -5000)) in cases and ((0, 0), (0, 0)) in cases
    for poff, off in cases:
        want = fs.start_fields(orc, prior, w, h, LEVELS, poff, off, 0)
        got = fs.pointwise(orc, prior, w, h, LEVELS, poff, off, 0)
        assert sorted(want) == sorted(got) == list(range(F_))
        for k in range(F_):
            assert_bit_equal(got[k], want[k], f"{w}x{h}, F = {F_}, prior at {poff}, window at {off}, level {k}")


def test_a_field_prior_is_restrict_crop_and_level_0_is_a_crop(orc):
    rng = np.random.default_rng(77)
    field = rng.normal(0, 30, (3, H, W)).astype(np.float32)
    fw, fh, ox, oy, _, _ = fs.origins(orc, W, H, LEVELS, F, lc.OFF_CENTRE)
    got = fs.start_fields_field(orc, field, W, H, LEVELS, F, lc.OFF_CENTRE, 0)
    assert_bit_equal(got[0], field[:, oy[0]:oy[0] + fh, ox[0]:ox[0] + fw], "level 0 of a field prior: the window itself")
    assert got[F - 1].shape == (3, fh, fw)


# ---- 2. the premises of the GPU tests, from the oracle alone ----------------------------------------------------------------------------------

def test_premises_a_warm_start_moves_the_stack_and_the_priors_offsets_matter(orc):
    L, R = lc.pairs()[0]
    cold, _, _ = orc.match_foveated(L, R, LEVELS, F, 0, 0)
    warm = fs.warm_oracle(orc, L, R, cold, LEVELS, (0, 0), (0, 0), F - 1)
    assert warm.shape == cold.shape
    assert not np.array_equal(warm.view(np.uint32), cold.view(np.uint32)), "from its own cold stack at level F-1 the call must still differ"
    a = fs.start_fields(orc, cold, W, H, LEVELS, (0, 0), lc.OFF_CENTRE, 0)
    b = fs.start_fields(orc, cold, W, H, LEVELS, (5000, -5000), lc.OFF_CENTRE, 0)
    for k in range(F):          # (level F-1 too: inside a finer window of the prior the finer level's value is taken)
        assert not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"level {k}: the prior's offsets do not matter"


# ---- 3. every refusal, over the stand-in runtime -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fakewarm") / "libugsm_warm_fake.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fvisibility=hidden",
           os.path.join(ROOT, "tests", "fake_runtime.cpp"), os.path.join(ROOT, "tests", "fake_fovea_seeded.cpp"),
           os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm_fovea_seeded.cpp"),
           "-Wl,--version-script=" + os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm.map"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    so = C.CDLL(out, mode=os.RTLD_NOW)
    vp, i, pp, ip = C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)
    so.ugsm_fake_create.restype = vp
    so.ugsm_fake_create.argtypes = [i, i, i, i]
    so.ugsm_fake_destroy.argtypes = [vp]
    so.ugsm_fake_destroy.restype = None
    so.ugsm_fake_warm_lr.argtypes = [C.c_float, i]
    so.ugsm_fake_warm_early_exit.argtypes = [vp, C.c_float]
    so.ugsm_fake_warm_fovea_levels.argtypes = [vp, i]
    so.ugsm_fake_warm_queue_busy.argtypes = [vp, i]
    so.ugsm_fake_warm_input_format.argtypes = [vp, i]
    so.ugsm_fake_warm_reached.argtypes = [C.POINTER(i * 7)]
    so.ugsm_submit_foveated_warm.argtypes = [vp, i, i, pp, pp, i, i, i, ip, ip, pp, ip, ip, i, pp]
    so.ugsm_submit_foveated_warm_field.argtypes = [vp, i, i, pp, pp, i, i, i, ip, ip, pp, i, pp]
    so.ugsm_match_foveated_warm.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, i, i, i, vp, vp, vp]
    so.ugsm_fovea_warm_pixel_iterations.argtypes = [i, i, i, i, i]
    so.ugsm_fovea_warm_pixel_iterations.restype = C.c_longlong
    so.ugsm_fovea_dims.argtypes = [i, i, i, i, ip, ip]
    so.ugsm_last_error.argtypes = [vp]
    so.ugsm_last_error.restype = C.c_char_p
    return so


def _reached(fake):
    v = (C.c_int * 7)()
    fake.ugsm_fake_warm_reached(C.byref(v))
    return list(v)


def _ptrs(n, base, hole=None, step=1 << 24):
    return (C.c_void_p * max(n, 1))(*[None if k == hole else base + step * k for k in range(max(n, 1))])


def test_every_status_before_the_runtime_is_reached(fake):
    ctx = fake.ugsm_fake_create(1, 3, 14, 7)
    try:
        fake.ugsm_fake_warm_lr(0.0, 0)

        def submit(n=3, W_=64, H_=48, stride=192, level=5, L=None, R=None, P=None, O=None, c=ctx, field=False):
            L, R, P, O = [_ptrs(n, 0x7F0000000000 + (j << 32)) if a is None else a for j, a in enumerate((L, R, P, O))]
            L, R, P, O = [None if a is False else a for a in (L, R, P, O)]
            if field:
                return fake.ugsm_submit_foveated_warm_field(c, 0, n, L, R, W_, H_, stride, None, None, P, level, O)
            return fake.ugsm_submit_foveated_warm(c, 0, n, L, R, W_, H_, stride, None, None, P, None, None, level, O)

        def match(W_=64, H_=48, stride=192, level=5, ptr=0x7F0000000000, hole=None, c=ctx):
            a = [None if k == hole else ptr + (1 << 24) * k for k in range(8)]
            return fake.ugsm_match_foveated_warm(c, a[0], a[1], W_, H_, stride, 3, -4, a[2], a[3], a[4], 0, 0, level, a[5], a[6], a[7])

        before = _reached(fake)
        # null context, null arrays, null entries
        assert submit(c=None) == BAD_ARG and submit(c=None, field=True) == BAD_ARG and match(c=None) == BAD_ARG
        for field in (False, True):
            for which in range(4):
                args = [None] * 4
                args[which] = False
                assert submit(L=args[0], R=args[1], P=args[2], O=args[3], field=field) == BAD_ARG, which
                args[which] = _ptrs(3, 0x7F0000000000 + (which << 32), hole=1)
                assert submit(L=args[0], R=args[1], P=args[2], O=args[3], field=field) == BAD_ARG, which
        for hole in range(8):
            assert match(hole=hole) == BAD_ARG, hole
        # n and start_level out of range: the levels are the FOVEA levels 0 .. F-1
        for n in (0, -1, 17):
            assert submit(n=n) == BAD_ARG, n
        for level in (-1, 7, 13, 100):
            assert submit(level=level) == BAD_ARG and submit(level=level, field=True) == BAD_ARG and match(level=level) == BAD_ARG, level
        assert b"start_level" in fake.ugsm_last_error(ctx)
        # fovea_levels < 2
        for F_ in (1, 0):
            fake.ugsm_fake_warm_fovea_levels(ctx, F_)
            assert submit(level=0) == BAD_ARG and match(level=0) == BAD_ARG
            assert b"fovea_levels" in fake.ugsm_last_error(ctx)
        fake.ugsm_fake_warm_fovea_levels(ctx, 7)
        # the early exit
        fake.ugsm_fake_warm_early_exit(ctx, 0.02)
        assert submit() == BAD_ARG and match() == BAD_ARG
        assert b"early_exit_threshold" in fake.ugsm_last_error(ctx)
        fake.ugsm_fake_warm_early_exit(ctx, 0.0)
        # not in place: a prior that is (or overlaps) any of the call's d_stack buffers
        O = _ptrs(3, 0x7F0300000000)
        for k in range(3):
            P = _ptrs(3, 0x7F0200000000)
            P[k] = O[(k + 1) % 3]
            assert submit(P=P, O=O) == BAD_ARG and submit(P=P, O=O, field=True) == BAD_ARG, k
            assert b"not in place" in fake.ugsm_last_error(ctx)
            P[k] = O[k] + 64                                  # inside the stack, not at its start
            assert submit(P=P, O=O) == BAD_ARG, k
        # the foveated LR check in force: a state, not an argument; the full-mode check alone does not matter
        fake.ugsm_fake_warm_lr(1.0, 2)
        assert submit() == STATE and submit(field=True) == STATE and match() == STATE
        fake.ugsm_fake_warm_lr(1.0, 3)
        assert submit() == STATE
        accepted = 0
        fake.ugsm_fake_warm_lr(1.0, 1)
        assert submit() == OK
        fake.ugsm_fake_warm_lr(0.0, 2)
        assert submit() == OK
        accepted += 2
        # pairs outstanding in the queue
        fake.ugsm_fake_warm_queue_busy(ctx, 1)
        assert submit() == STATE and match() == STATE
        fake.ugsm_fake_warm_queue_busy(ctx, 0)
        # size errors, as ugsm_submit_foveated: no such size, a stride below the format's row
        assert submit(W_=0) == BAD_ARG and match(H_=-4) == BAD_ARG
        assert submit(stride=191) == SIZE_MISMATCH and match(stride=191) == SIZE_MISMATCH
        fake.ugsm_fake_warm_input_format(ctx, 2)          # rgba8: four bytes per pixel
        assert submit(stride=255) == SIZE_MISMATCH and submit(stride=256) == OK
        accepted += 1
        fake.ugsm_fake_warm_input_format(ctx, 0)
        # ... and none of the refused calls reached the runtime; the accepted ones did, with their arguments
        after = _reached(fake)
        assert after[0] - before[0] == accepted and after[1] == before[1]
        assert submit(n=16, level=0) == OK and _reached(fake)[2:] == [0, 16, 64, 0, 0]
        assert submit(n=1, level=6, field=True) == OK and _reached(fake)[2:] == [0, 1, 64, 6, 1]
        assert match(level=6) == OK and _reached(fake)[1] == before[1] + 1 and _reached(fake)[2:] == [0, 1, 64, 6, 0]
    finally:
        fake.ugsm_fake_destroy(ctx)


def test_warm_pixel_iterations_is_the_fovea_times_the_iterations(lib, fake):
    so = lib.load()
    for (w_, h_, lv, F_) in [(4928, 3264, 14, 7), (1920, 1080, 14, 7), (333, 251, 14, 7), (67, 49, 9, 2), (333, 251, 14, 14)]:
        fw, fh = lib.fovea_dims(w_, h_, lv, F_)
        for s in range(F_):
            want = fw * fh * sum(lib.level_iterations(i) for i in range(s + 1))
            assert lib.fovea_warm_pixel_iterations(w_, h_, lv, F_, s) == want, (w_, h_, lv, F_, s)
        assert so.ugsm_fovea_warm_pixel_iterations(w_, h_, lv, F_, F_) == -1 and so.ugsm_fovea_warm_pixel_iterations(w_, h_, lv, F_, -1) == -1
    assert lib.fovea_warm_pixel_iterations(333, 251, 14, 7, 6) == lib.pixel_iterations(333, 251, 14, 7) - sum(
        w * h * lib.level_iterations(i) for i, (w, h) in enumerate(zip(*lib.level_dims(333, 251, 14))) if i >= 7)
    for bad in [(0, 10, 3, 2, 0), (64, 48, 14, 7, 0), (640, 480, 40, 7, 0), (640, 480, 9, 1, 0), (640, 480, 9, 10, 0)]:
        assert so.ugsm_fovea_warm_pixel_iterations(*bad) == -1, bad
    # the same source over the stand-in's own geometry and counts
    fw, fh = C.c_int(), C.c_int()
    assert fake.ugsm_fovea_dims(640, 480, 9, 5, C.byref(fw), C.byref(fh)) == OK
    assert fake.ugsm_fovea_warm_pixel_iterations(640, 480, 9, 5, 3) == fw.value * fh.value * sum(2 + i for i in range(4))


# ---- 4. exports, bindings, shims, documents ------------------------------------------------------------------------------------------------------

def test_the_header_is_plain_c99_with_the_five_names(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ugsm.h"
    src = tmp_path / "use.c"
    src.write_text('#include "ugsm.h"\n'
                   "long long use(ugsm_ctx *c, const uint8_t *const *l, const float *const *p, float *const *o, const uint8_t *h, float *f, const int *at)\n"
                   "{\n"
                   "    return ugsm_submit_foveated_warm(c, 0, 1, l, l, 64, 48, 192, at, at, p, at, at, 5, o)\n"
                   "           + ugsm_submit_foveated_warm_field(c, 0, 1, l, l, 64, 48, 192, at, at, p, 5, o)\n"
                   "           + ugsm_match_foveated_warm(c, h, h, 64, 48, 192, 0, 0, f, f, f, 0, 0, 5, f, f, f)\n"
                   "           + ugsm_stage_warm_stack(c, f, 64, 48, 0, 0, 3, 4, 5, f) + ugsm_fovea_warm_pixel_iterations(64, 48, 3, 2, 1);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert re.search(r"#define UGSM_ABI_VERSION 6\b", hdr), "additions only: the ABI number stays"
    spec = hdr.split("int ugsm_submit_foveated_warm(")[0].rsplit("The seeded FOVEATED call", 1)[1]
    assert "WARNING" in spec and "never refreshes the levels above start_level" in spec
    said = spec.rsplit("NOT built:", 1)[1]
    for what in ("pyramid stacks", "queue or managed form", "page-locked", "checked call", "multi-window call", "start levels above F-1"):
        assert what in said, what
    abi = hdr.split("the seeded (warm) foveated call --", 1)[1].split("6: the kernel choices", 1)[0]
    for name in NAMES:
        assert name in abi, f"{name}: the ABI comment's list of additions"


def test_both_libraries_export_them_and_nothing_else_new(lib):
    for name in NAMES:
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for path, extra in ((lib.LIB_PATH, []), (lib.DEV_LIB_PATH, lib.DEV_EXPORTS)):
        dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
        for name in NAMES:
            assert re.search(rf" T {name}$", dyn, re.M), f"{name} is not a dynamic symbol of {os.path.basename(path)}"
        assert names == declared | set(extra), sorted(names ^ (declared | set(extra)))
        assert {n for n in names if "warm" in n} == set(NAMES)
    so = lib.load()
    assert so.ugsm_abi_version() == 6
    assert [len(getattr(so, n).argtypes) for n in NAMES] == [15, 13, 17, 10, 5]


def test_a_null_context_is_a_status_code(lib):
    for dev in (False, True):
        so = lib.load(dev)
        ptrs = (C.c_void_p * 1)(None)
        assert so.ugsm_submit_foveated_warm(None, 0, 1, ptrs, ptrs, 64, 48, 192, None, None, ptrs, None, None, 5, ptrs) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_submit_foveated_warm_field(None, 0, 1, ptrs, ptrs, 64, 48, 192, None, None, ptrs, 5, ptrs) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_match_foveated_warm(None, None, None, 64, 48, 192, 0, 0, None, None, None, 0, 0, 5, None, None, None) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_stage_warm_stack(None, None, 64, 48, 0, 0, 0, 0, 5, None) == lib.UGSM_ERR_BAD_ARG


class _FakeLib:
    """Stands in for the loaded library: records what the Context methods hand to the C calls."""

    def __init__(self):
        self.calls = []

    def _record(self, *args):
        self.calls.append(args)
        return 0

    ugsm_submit_foveated_warm = ugsm_submit_foveated_warm_field = ugsm_stage_warm_stack = _record


def test_the_python_binding_marshals_its_lists(lib):
    c = object.__new__(lib.Context)
    c._h, c.lib = 1234, _FakeLib()
    c.submit_foveated_warm(1, [10, 20, 30], [11, 21, 31], 64, 48, 192, [(1, 2), (3, 4), (5, 6)], [12, 22, 32], [(7, 8), (9, 10), (11, 12)], 5, [13, 23, 33])
    c.submit_foveated_warm(0, [10], [11], 64, 48, 200, None, [12], None, 0, [14])
    (h, slot, n, dl, dr, W_, H_, stride, ox, oy, dp, px, py, level, do), second = c.lib.calls
    assert (h, slot, n, W_, H_, stride, level) == (1234, 1, 3, 64, 48, 192, 5)
    assert list(dl) == [10, 20, 30] and list(dr) == [11, 21, 31] and list(dp) == [12, 22, 32] and list(do) == [13, 23, 33]
    assert (list(ox), list(oy), list(px), list(py)) == ([1, 3, 5], [2, 4, 6], [7, 9, 11], [8, 10, 12])
    assert second[2] == 1 and second[7] == 200 and second[8] is second[9] is second[11] is second[12] is None and second[13] == 0
    c.submit_foveated_warm_field(2, [10, 20], [11, 21], 64, 48, 192, [(1, 2), (3, 4)], [12, 22], 4, [13, 23])
    assert c.lib.calls[-1][1:3] == (2, 2) and list(c.lib.calls[-1][10]) == [12, 22] and c.lib.calls[-1][11] == 4
    for bad in (([10, 20], [11], [12, 22], [13, 23]), ([10, 20], [11, 21], [12], [13, 23]), ([10, 20], [11, 21], [12, 22], [13])):
        with pytest.raises(lib.UgsmError):
            c.submit_foveated_warm(0, bad[0], bad[1], 64, 48, 192, None, bad[2], None, 5, bad[3])
    with pytest.raises(lib.UgsmError):
        c.submit_foveated_warm(0, [10, 20], [11, 21], 64, 48, 192, [(0, 0)], [12, 22], None, 5, [13, 23])
    assert len(c.lib.calls) == 3
    c.stage_warm_stack(77, 64, 48, (1, 2), (3, 4), 3, 88)
    assert c.lib.calls[-1] == (1234, 77, 64, 48, 1, 2, 3, 4, 3, 88)


def test_the_python_mirror_and_the_shims_expose_the_call(lib):
    for method in ("submit_foveated_warm", "submit_foveated_warm_field", "match_foveated_warm", "stage_warm_stack"):
        assert hasattr(lib.Context, method), method
    assert list(inspect.signature(lib.Context.submit_foveated_warm).parameters)[-4:] == ["d_prior_stack", "prior_offsets", "start_level", "d_stack"]
    assert callable(lib.fovea_warm_pixel_iterations)
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    assert list(inspect.signature(MatchGPULib.matchStackSeeded).parameters) == ["self", "cv_ptrL", "cv_ptrR", "prior_stack", "prior_off", "off", "start_level"]
    shim = open(os.path.join(ROOT, "ros", "MatchGPULib_ugsm.hpp")).read()
    assert "float ***matchStackSeeded(ImgPtr L, ImgPtr R, float **const *prior_stack, const int *prior_off, const int *off, int start_level)" in shim
    assert "ugsm_match_foveated_warm(ctx_," in shim
    assert "m.matchStackSeeded(L, R, st, at0, at1, sl)" in open(os.path.join(ROOT, "ros", "shim_selftest.cpp")).read()


def test_the_shim_selftest_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "ros", "shim_selftest.cpp"),
                           "-o", str(tmp_path / "shim_selftest.o")])


def test_the_starting_fields_are_k_restrict_stack_and_a_class_of_the_statistics():
    """The starting-field kernel is a kernel of its own name, k_restrict_stack, beside k_upsample_paste (ugsm_kernels_fields.hip), whose rule it
    descends; the name is also its class in the kernel statistics, and k_upsample_paste is the one operation of that name.  No atomics in it."""
    csrc = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")
    fields = open(os.path.join(csrc, "ugsm_kernels_fields.hip")).read()
    assert len(re.findall(r"__global__[^\n]*\bvoid k_restrict_stack\(", fields)) == 1
    assert len(re.findall(r"__global__[^\n]*\bvoid k_upsample_paste\(", fields)) == 1 and fields.count("k_upsample_paste(") == 1
    body = fields.split("RestrictStack rs)\n{", 1)[1].split("\n}\n", 1)[0]
    assert "restrict_site(" in body and "tex_index(" in body and "atomic" not in body
    assert "bool launch_restrict_stack(" in fields
    assert '"k_restrict_stack"' in open(os.path.join(csrc, "ugsm_runtime.cpp")).read()


def test_the_documents_carry_the_call():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text, what in ((integ, "INTEGRATION.md"), (design, "DESIGN.md"), (readme, "README.md")):
        assert "ugsm_submit_foveated_warm" in text, what
    for name in NAMES:
        assert name in design, name
    assert "fovea_seeded_bench" in design and "matchStackSeeded" in integ
