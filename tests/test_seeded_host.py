"""The seeded full-mode call (ugsm_submit_full_seeded, ugsm_match_full_seeded, ugsm_stage_restrict, ugsm_seeded_pixel_iterations) without a
GPU: the numpy restriction's closed-form sites against the pyramid's own sampling chain; the oracle composition the GPU tests compare with
against orc.match_full; every refusal of the call, driven through the real csrc/ugsm_seeded.cpp over the recording stand-in runtime
(tests/fake_runtime.cpp, unchanged, plus tests/fake_seeded.cpp); the size of a seeded call; the exports, the bindings, the shims, the documents."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import seeded_np as sn
from conftest import ROOT, assert_bit_equal

NAMES = ("ugsm_submit_full_seeded", "ugsm_match_full_seeded", "ugsm_stage_restrict", "ugsm_seeded_pixel_iterations")
OK, BAD_ARG, SIZE_MISMATCH, STATE = 0, 1, 2, 7
W, H, LEVELS = 333, 251, 14


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


# ---- 1. the restriction in numpy ---------------------------------------------------------------------------------------------------------

def _axis_dims(n, levels=14):
    d = [n]
    while len(d) < levels and int(d[-1] / sn.SCALE) >= 1:
        d.append(int(d[-1] / sn.SCALE))            # MatchGPULib.cpp:1224-1228
    return d


def test_level_dims_of_the_sweep_are_the_oracles(orc):
    for n in (40, 333, 700, 1080, 4928):
        assert _axis_dims(n) == orc.level_dims(n, n, len(_axis_dims(n)))[0]


def test_closed_form_sites_equal_the_pyramid_chain_and_no_clamp_binds():
    for n in list(range(40, 701)) + [1080, 1920, 3264, 4928]:
        dims = _axis_dims(n)
        for s in range(len(dims)):
            closed, walked = sn.sites_closed(dims[s], s, n), sn.sites_stepwise(s, dims)
            assert np.array_equal(closed, walked), (n, s)
            k = s // 2
            if s % 2 == 0:                          # the issue's closed form, without any clamp
                assert np.array_equal(closed, ((np.arange(dims[s]) + 1) << k) - 1), (n, s)
            assert closed[-1] <= n - 1 and np.all(np.diff(closed) > 0), (n, s)


def test_restriction_values():
    rng = np.random.default_rng(5)
    f = rng.normal(0, 30, (3, 97, 131)).astype(np.float32)
    f[0, 0, 0], f[1, 0, 0], f[0, 1, 1], f[1, 1, 1] = np.float32(-0.0), np.inf, np.float32(3e38), np.float32(1e-44)
    assert_bit_equal(sn.restrict_np(f, 0, 131, 97), f, "level 0 is a copy")
    dw, dh = _axis_dims(131), _axis_dims(97)
    for s in range(1, 8):
        r = sn.restrict_np(f, s, dw[s], dh[s])
        k = s // 2
        sx, sy = sn.sites_closed(dw[s], s, 131), sn.sites_closed(dh[s], s, 97)
        assert r.shape == (3, dh[s], dw[s])
        assert_bit_equal(r[2], f[2][sy][:, sx], f"level {s}: the confidence is copied")
        src = f[0][sy][:, sx]
        want = (src.astype(np.float64) / 1.41421356).astype(np.float32) * np.float32(2.0 ** -k) if s % 2 else src * np.float32(2.0 ** -k)
        assert_bit_equal(r[0], want, f"level {s}: dx")
    r2 = sn.restrict_np(f, 2, dw[2], dh[2])         # site (0, 0) of level 2 is (1, 1) of level 0
    assert r2[0, 0, 0] == np.float32(1.5e38) and r2[1, 0, 0] == np.float32(1e-44) * np.float32(0.5)


# ---- 2. the oracle composition -----------------------------------------------------------------------------------------------------------

def test_the_composition_reproduces_match_full_and_a_prior_moves_the_field(orc):
    from ug_stereomatcher_amd import synth
    L, R = synth.make_pair(W, H, synth.BASE_SEED + 7300)[:2]
    cold = orc.match_full(L, R, LEVELS)
    assert_bit_equal(sn.cold_by_stages(orc, L, R, LEVELS), cold, "the stages composed, from the zero seed with is_top at the top level")
    pyr = sn.pyramids(orc, L, R, LEVELS)
    for s in (13, 9, 5, 3, 0):
        seeded = sn.seeded_oracle(orc, L, R, cold, s, LEVELS, pyr)
        moved = np.abs(seeded[:2].astype(np.float64) - cold[:2]).mean()
        print(f"start level {s}: mean |seeded - cold| = {moved:.3f} px")
        assert seeded.shape == cold.shape and not np.array_equal(seeded.view(np.uint32), cold.view(np.uint32)), s


# ---- 3. every refusal, over the stand-in runtime -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fakeseeded") / "libugsm_seeded_fake.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fvisibility=hidden",
           os.path.join(ROOT, "tests", "fake_runtime.cpp"), os.path.join(ROOT, "tests", "fake_seeded.cpp"),
           os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm_seeded.cpp"),
           "-Wl,--version-script=" + os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm.map"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    so = C.CDLL(out, mode=os.RTLD_NOW)
    vp, i, pp = C.c_void_p, C.c_int, C.POINTER(C.c_void_p)
    so.ugsm_fake_create.restype = vp
    so.ugsm_fake_create.argtypes = [i, i, i, i]
    so.ugsm_fake_destroy.argtypes = [vp]
    so.ugsm_fake_destroy.restype = None
    so.ugsm_fake_seeded_lr.argtypes = [C.c_float, i]
    so.ugsm_fake_seeded_early_exit.argtypes = [vp, C.c_float]
    so.ugsm_fake_seeded_queue_busy.argtypes = [vp, i]
    so.ugsm_fake_seeded_input_format.argtypes = [vp, i]
    so.ugsm_fake_seeded_reached.argtypes = [C.POINTER(i * 6)]
    so.ugsm_submit_full_seeded.argtypes = [vp, i, i, pp, pp, i, i, i, pp, i, pp]
    so.ugsm_match_full_seeded.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, i, vp, vp, vp]
    so.ugsm_seeded_pixel_iterations.argtypes = [i, i, i, i]
    so.ugsm_seeded_pixel_iterations.restype = C.c_longlong
    so.ugsm_level_dims.argtypes = [i, i, i, C.POINTER(i), C.POINTER(i)]
    so.ugsm_last_error.argtypes = [vp]
    so.ugsm_last_error.restype = C.c_char_p
    return so


def _reached(fake):
    v = (C.c_int * 6)()
    fake.ugsm_fake_seeded_reached(C.byref(v))
    return list(v)


def _ptrs(n, base=0x7F0000000000, hole=None):
    return (C.c_void_p * max(n, 1))(*[None if k == hole else base + 4096 * k for k in range(max(n, 1))])


def test_every_status_before_the_runtime_is_reached(fake):
    ctx = fake.ugsm_fake_create(1, 3, 14, 7)
    try:
        fake.ugsm_fake_seeded_lr(0.0, 0)

        def submit(n=3, W_=64, H_=48, stride=192, level=5, L=None, R=None, P=None, O=None, c=ctx):
            L, R, P, O = [_ptrs(n, 0x7F0000000000 + (j << 32)) if a is None else a for j, a in enumerate((L, R, P, O))]
            L, R, P, O = [None if a is False else a for a in (L, R, P, O)]
            return fake.ugsm_submit_full_seeded(c, 0, n, L, R, W_, H_, stride, P, level, O)

        def match(W_=64, H_=48, stride=192, level=5, ptr=0x7F0000000000, hole=None, c=ctx):
            a = [None if k == hole else ptr + 4096 * k for k in range(8)]
            return fake.ugsm_match_full_seeded(c, a[0], a[1], W_, H_, stride, a[2], a[3], a[4], level, a[5], a[6], a[7])

        before = _reached(fake)
        # null context, null arrays, null entries
        assert submit(c=None) == BAD_ARG and match(c=None) == BAD_ARG
        for which in range(4):
            args = [None] * 4
            args[which] = False
            assert submit(L=args[0], R=args[1], P=args[2], O=args[3]) == BAD_ARG, which
            args[which] = _ptrs(3, hole=1)
            assert submit(L=args[0], R=args[1], P=args[2], O=args[3]) == BAD_ARG, which
        for hole in range(8):
            assert match(hole=hole) == BAD_ARG, hole
        # n and start_level out of range
        for n in (0, -1, 17):
            assert submit(n=n) == BAD_ARG, n
        for level in (-1, 14, 100):
            assert submit(level=level) == BAD_ARG and match(level=level) == BAD_ARG, level
        assert b"start_level" in fake.ugsm_last_error(ctx)
        # the early exit
        fake.ugsm_fake_seeded_early_exit(ctx, 0.02)
        assert submit() == BAD_ARG and match() == BAD_ARG
        assert b"early_exit_threshold" in fake.ugsm_last_error(ctx)
        fake.ugsm_fake_seeded_early_exit(ctx, 0.0)
        # the full-mode LR check in force: a state, not an argument; the foveated check alone does not matter
        fake.ugsm_fake_seeded_lr(1.0, 1)
        assert submit() == STATE and match() == STATE
        fake.ugsm_fake_seeded_lr(1.0, 3)
        assert submit() == STATE
        fake.ugsm_fake_seeded_lr(1.0, 2)
        assert submit() == OK
        fake.ugsm_fake_seeded_lr(0.0, 1)
        assert submit() == OK
        # pairs outstanding in the queue
        fake.ugsm_fake_seeded_queue_busy(ctx, 1)
        assert submit() == STATE and match() == STATE
        fake.ugsm_fake_seeded_queue_busy(ctx, 0)
        # size errors, as ugsm_submit_full: no such size, a stride below the format's row
        assert submit(W_=0) == BAD_ARG and match(H_=-4) == BAD_ARG
        assert submit(stride=191) == SIZE_MISMATCH and match(stride=191) == SIZE_MISMATCH
        fake.ugsm_fake_seeded_input_format(ctx, 2)          # rgba8: four bytes per pixel
        assert submit(stride=255) == SIZE_MISMATCH and submit(stride=256) == OK
        fake.ugsm_fake_seeded_input_format(ctx, 0)
        # ... and none of the refused calls reached the runtime; the accepted ones did, with their arguments
        after = _reached(fake)
        assert after[0] - before[0] == 3 and after[1] == before[1]
        assert submit(n=16, level=0) == OK and _reached(fake)[2:] == [0, 16, 64, 0]
        assert submit(n=1, level=13) == OK and _reached(fake)[2:] == [0, 1, 64, 13]
        assert match(level=13) == OK and _reached(fake)[1] == before[1] + 1 and _reached(fake)[2:] == [0, 1, 64, 13]
    finally:
        fake.ugsm_fake_destroy(ctx)


def test_seeded_pixel_iterations_is_the_sum_over_the_levels(lib, fake):
    so = lib.load()
    for (w_, h_, lv) in [(4928, 3264, 14), (1920, 1080, 14), (333, 251, 14), (67, 49, 9), (640, 480, 3)]:
        w, h = lib.level_dims(w_, h_, lv)
        for s in range(lv):
            want = sum(w[i] * h[i] * lib.level_iterations(i) for i in range(s + 1))
            assert lib.seeded_pixel_iterations(w_, h_, lv, s) == want, (w_, h_, lv, s)
        assert lib.seeded_pixel_iterations(w_, h_, lv, lv - 1) == lib.pixel_iterations(w_, h_, lv, 0)
        assert so.ugsm_seeded_pixel_iterations(w_, h_, lv, lv) == -1 and so.ugsm_seeded_pixel_iterations(w_, h_, lv, -1) == -1
    assert so.ugsm_seeded_pixel_iterations(0, 10, 3, 0) == -1 and so.ugsm_seeded_pixel_iterations(64, 48, 14, 0) == -1
    assert so.ugsm_seeded_pixel_iterations(64, 48, 40, 0) == -1
    # the same source over the stand-in's own geometry and counts
    w, h = (C.c_int * 32)(), (C.c_int * 32)()
    assert fake.ugsm_level_dims(640, 480, 9, w, h) == OK
    assert fake.ugsm_seeded_pixel_iterations(640, 480, 9, 4) == sum(w[i] * h[i] * (2 + i) for i in range(5))


# ---- 4. exports, bindings, shims, documents ----------------------------------------------------------------------------------------------

def test_the_header_is_plain_c99_with_the_four_names(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ugsm.h"
    src = tmp_path / "use.c"
    src.write_text('#include "ugsm.h"\n'
                   "long long use(ugsm_ctx *c, const uint8_t *const *l, const float *const *p, float *const *o, const uint8_t *h, float *f)\n"
                   "{\n"
                   "    return ugsm_submit_full_seeded(c, 0, 1, l, l, 64, 48, 192, p, 5, o) + ugsm_match_full_seeded(c, h, h, 64, 48, 192, f, f, f, 5, f, f, f)\n"
                   "           + ugsm_stage_restrict(c, f, 64, 48, 5, f) + ugsm_seeded_pixel_iterations(64, 48, 3, 1);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])
    assert re.search(r"#define UGSM_ABI_VERSION 6\b", hdr), "additions only: the ABI number stays"
    said = hdr.split("int ugsm_submit_full_seeded(")[0].rsplit("NOT built:", 1)[1]
    assert "queue form" in said and "page-locked _host kind" in said and "seeded checked or foveated call" in said


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
        assert {n for n in names if "seeded" in n or "restrict" in n} == set(NAMES)
    so = lib.load()
    assert so.ugsm_abi_version() == 6
    assert len(so.ugsm_submit_full_seeded.argtypes) == 11 and len(so.ugsm_match_full_seeded.argtypes) == 13 and len(so.ugsm_stage_restrict.argtypes) == 6


def test_a_null_context_is_a_status_code(lib):
    for dev in (False, True):
        so = lib.load(dev)
        ptrs = (C.c_void_p * 1)(None)
        assert so.ugsm_submit_full_seeded(None, 0, 1, ptrs, ptrs, 64, 48, 192, ptrs, 5, ptrs) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_match_full_seeded(None, None, None, 64, 48, 192, None, None, None, 5, None, None, None) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_stage_restrict(None, None, 64, 48, 5, None) == lib.UGSM_ERR_BAD_ARG


class _FakeLib:
    """Stands in for the loaded library: records what the Context methods hand to the C calls."""

    def __init__(self):
        self.calls = []

    def ugsm_submit_full_seeded(self, *args):
        self.calls.append(args)
        return 0

    def ugsm_stage_restrict(self, *args):
        self.calls.append(args)
        return 0


def test_the_python_binding_marshals_its_lists(lib):
    c = object.__new__(lib.Context)
    c._h, c.lib = 1234, _FakeLib()
    c.submit_full_seeded(1, [10, 20, 30], [11, 21, 31], 64, 48, 192, [12, 22, 32], 5, [13, 23, 33])
    c.submit_full_seeded(0, [10], [11], 64, 48, 200, [12], 0, [12])
    (h, slot, n, dl, dr, W_, H_, stride, dp, level, do), second = c.lib.calls
    assert (h, slot, n, W_, H_, stride, level) == (1234, 1, 3, 64, 48, 192, 5)
    assert list(dl) == [10, 20, 30] and list(dr) == [11, 21, 31] and list(dp) == [12, 22, 32] and list(do) == [13, 23, 33]
    assert second[2] == 1 and second[7] == 200 and second[9] == 0 and list(second[8]) == list(second[10]) == [12]
    for bad in (([10, 20], [11], [12, 22], [13, 23]), ([10, 20], [11, 21], [12], [13, 23]), ([10, 20], [11, 21], [12, 22], [13])):
        with pytest.raises(lib.UgsmError):
            c.submit_full_seeded(0, bad[0], bad[1], 64, 48, 192, bad[2], 5, bad[3])
    assert len(c.lib.calls) == 2
    c.stage_restrict(77, 64, 48, 3, 88)
    assert c.lib.calls[-1] == (1234, 77, 64, 48, 3, 88)


def test_the_python_mirror_and_the_shims_expose_the_call(lib):
    for method in ("submit_full_seeded", "match_full_seeded", "stage_restrict"):
        assert hasattr(lib.Context, method), method
    assert list(inspect.signature(lib.Context.submit_full_seeded).parameters)[-3:] == ["d_prior", "start_level", "d_out"]
    assert callable(lib.seeded_pixel_iterations)
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    assert list(inspect.signature(MatchGPULib.matchSeeded).parameters) == ["self", "cv_ptrL", "cv_ptrR", "prior", "start_level"]
    shim = open(os.path.join(ROOT, "ros", "MatchGPULib_ugsm.hpp")).read()
    assert "float **matchSeeded(ImgPtr L, ImgPtr R, float *const *prior, int start_level)" in shim and "ugsm_match_full_seeded(ctx_," in shim
    node = open(os.path.join(ROOT, "ros", "UG_GPU_matcher_ugsm.cpp")).read()
    assert 'nh_.getParam("seed_level", s)' in node and "mgpu_->matchSeeded(L, R, last_, sl)" in node
    assert "int s = -1;" in node.split("int seed_level()")[1].split("}")[0], "seed_level is off by default"
    assert "m.matchSeeded(L, R, cold, 5)" in open(os.path.join(ROOT, "ros", "shim_selftest.cpp")).read()


def test_the_shim_selftest_and_the_node_compile(lib, tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "ros", "shim_selftest.cpp"),
                           "-o", str(tmp_path / "shim_selftest.o")])
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Itests/ros_stubs", "-Iros", "-Iinclude", "ros/UG_GPU_matcher_ugsm.cpp"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_restriction_is_k_restrict_and_a_class_of_the_statistics():
    """The restriction is a kernel of its own name, k_restrict (ugsm_kernels_fields.hip), which is also its class in the kernel statistics;
    k_seed (ugsm_kernels_aux.hip) is the one operation of that name."""
    csrc = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")
    fields = open(os.path.join(csrc, "ugsm_kernels_fields.hip")).read()
    aux = open(os.path.join(csrc, "ugsm_kernels_aux.hip")).read()
    assert len(re.findall(r"__global__[^\n]*\bvoid k_restrict\(", fields)) == 1
    assert len(re.findall(r"__global__[^\n]*\bvoid k_seed\(", aux)) == 1 and aux.count("k_seed(") == 1
    assert "RestrictMap rm" in fields and "void launch_restrict(" in fields
    assert '"k_restrict"' in open(os.path.join(csrc, "ugsm_runtime.cpp")).read()


def test_the_documents_carry_the_call():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text, what in ((integ, "INTEGRATION.md"), (design, "DESIGN.md"), (readme, "README.md")):
        assert "ugsm_submit_full_seeded" in text, what
    assert "The seeded call" in design and "seeded_bench" in design
    assert "seed_level" in integ
