"""The float input formats (include/ugsm.h UGSM_INPUT_RGB32F, UGSM_INPUT_MONO32F) without a GPU: the tables, the header as C99, the
bindings' constants, the yardstick of the GPU tests (tests/float_np.py cold_float) proved against the oracle's own full-mode match, the
colour-word rule, and the alignment and stride refusals of the queue's entry points through the recording stand-in runtime."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import float_np as fl
from conftest import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, SIZE_MISMATCH = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_status_numbers_are_the_librarys(lib):
    assert (lib.UGSM_OK, lib.UGSM_ERR_BAD_ARG, lib.UGSM_ERR_SIZE_MISMATCH) == (OK, BAD_ARG, SIZE_MISMATCH)


def test_bytes_per_pixel_and_encoding_tables(lib):
    assert lib.input_bytes_per_pixel(fl.RGB32F) == 12 and lib.input_bytes_per_pixel(fl.MONO32F) == 4
    for unknown in (5, 6, 7, 10, 99, -1):
        assert lib.input_bytes_per_pixel(unknown) == -1, unknown
    assert lib.input_format_from_encoding("32FC3") == fl.RGB32F and lib.input_format_from_encoding("32FC1") == fl.MONO32F
    for bad in ("32fc3", "32FC2", "32FC4", "64FC1", "16UC1", "mono16", "rgb16", "32FC1 ", "32SC1"):
        assert lib.input_format_from_encoding(bad) == -1, bad
    so = C.CDLL(lib.DEV_LIB_PATH)
    assert so.ugsm_input_bytes_per_pixel(8) == 12 and so.ugsm_input_bytes_per_pixel(9) == 4 and so.ugsm_input_bytes_per_pixel(7) == -1


def test_bindings_constants_and_tables(lib):
    assert (lib.UGSM_INPUT_RGB32F, lib.UGSM_INPUT_MONO32F) == (8, 9) == fl.FORMATS
    for f in fl.FORMATS:
        assert lib.INPUT_BYTES_PER_PIXEL[f] == fl.BPP[f] == lib.input_bytes_per_pixel(f)
        assert lib.INPUT_ENCODINGS[fl.ENCODINGS[f]] == f
    for name, f in lib.INPUT_ENCODINGS.items():
        assert lib.input_format_from_encoding(name) == f and lib.INPUT_BYTES_PER_PIXEL[f] == lib.input_bytes_per_pixel(f)
    assert "ugsm_set_input_format" in lib.EXPORTS


def test_header_declares_the_two_macros_and_is_c99(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    assert re.search(r"#define UGSM_INPUT_RGB32F\s+8\b", hdr) and re.search(r"#define UGSM_INPUT_MONO32F\s+9\b", hdr)
    assert re.search(r"#define UGSM_ABI_VERSION 6\b", hdr)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "macros.c"
    src.write_text('#include "ugsm.h"\n'
                   "typedef char rgb32f_is_8[UGSM_INPUT_RGB32F == 8 ? 1 : -1];\n"
                   "typedef char mono32f_is_9[UGSM_INPUT_MONO32F == 9 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_encode_and_planes():
    rng = np.random.Generator(np.random.PCG64(8))
    rgb = rng.uniform(0, 256, (5, 7, 3)).astype(np.float32)
    a, m = fl.encode(rgb, fl.RGB32F), fl.encode(rgb, fl.MONO32F)
    assert a.dtype == np.float32 and a.shape == (5, 7, 3) and m.dtype == np.float32 and m.shape == (5, 7)
    p = fl.planes(a, fl.RGB32F)
    assert p.shape == (3, 5, 7) and all(np.array_equal(p[k], rgb[..., k]) for k in range(3))
    q = fl.planes(m, fl.MONO32F)
    assert q.shape == (3, 5, 7) and all(np.array_equal(q[k], rgb[..., 0]) for k in range(3))
    buf = fl.rows(a, 8)
    assert buf.shape == (5, 7 * 12 + 8) and np.array_equal(buf[:, :84].reshape(-1).view(np.float32).reshape(5, 7, 3), a)


def test_cold_float_on_integer_samples_is_the_oracles_full_match(orc):
    """The yardstick: from the float planes of an 8-bit pair, the stages give orc.match_full of the bytes, bit for bit (64 x 48, 5 levels)."""
    from ug_stereomatcher_amd import synth
    L, R = synth.make_pair(64, 48, synth.BASE_SEED + 71)[:2]
    want = orc.match_full(L, R, 5)
    for fmt in fl.FORMATS:
        eight = L if fmt == fl.RGB32F else np.ascontiguousarray(np.repeat(L[..., :1], 3, axis=2)), \
                R if fmt == fl.RGB32F else np.ascontiguousarray(np.repeat(R[..., :1], 3, axis=2))
        pl, pr = fl.planes(fl.encode(L, fmt), fmt), fl.planes(fl.encode(R, fmt), fmt)
        assert np.array_equal(pl, orc.rgb_to_planes(eight[0]))
        got = fl.cold_float(orc, pl, pr, 5)
        assert_bit_equal(got, want if fmt == fl.RGB32F else orc.match_full(eight[0], eight[1], 5), fl.NAMES[fmt])


def test_colour_byte_rule():
    v = np.array([0, 0.49, 0.5, 254.5, 255, 300, -1, np.nan, 1, 127.49, 127.5, 254.49, -0.0, np.inf, -np.inf], np.float32)
    assert fl.colour_byte(v).tolist() == [0, 0, 1, 255, 255, 255, 0, 0, 1, 127, 128, 254, 0, 255, 0]
    ints = np.arange(256, dtype=np.float32)
    assert np.array_equal(fl.colour_byte(ints), np.arange(256, dtype=np.uint32))  # integer samples: the 8-bit image's byte
    img = np.array([[[1, 2, 3], [255, 0, 300]]], np.float32)
    assert fl.colour_word(img, fl.RGB32F).tolist() == [[0x010203, 0xFF00FF]]
    assert fl.colour_word(img[..., 0], fl.MONO32F).tolist() == [[0x010101, 0xFFFFFF]]


# ---- the queue's refusals, through the recording stand-in runtime (tests/fake_runtime.cpp) ------------------------------------------------

@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fakeq_float") / "libugsm_queue_fake.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fvisibility=hidden",
           os.path.join(ROOT, "tests", "fake_runtime.cpp"), os.path.join(ROOT, "tests", "fake_input_format.cpp"),
           os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm_queue.cpp"),
           "-Wl,--version-script=" + os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm.map"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    so = C.CDLL(out)
    vp, i, u64 = C.c_void_p, C.c_int, C.c_uint64
    so.ugsm_fake_create.restype = vp
    so.ugsm_fake_create.argtypes = [i, i, i, i]
    so.ugsm_fake_destroy.argtypes = [vp]
    so.ugsm_fake_destroy.restype = None
    so.ugsm_fake_set_input_format.argtypes = [vp, i]
    so.ugsm_fake_get_input_format.argtypes = [vp]
    so.ugsm_fake_calls.argtypes = [vp]
    so.ugsm_fake_calls.restype = C.c_longlong
    so.ugsm_enqueue_full.argtypes = [vp, vp, vp, i, i, i, vp, u64]
    so.ugsm_enqueue_foveated.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, u64]
    so.ugsm_enqueue_full_managed.argtypes = [vp, vp, vp, i, i, i, u64]
    so.ugsm_queue_depth.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    return so


BASE = 0x7F0000000000  # made-up "device" addresses: the queue hands them on and never looks behind them


@pytest.mark.parametrize("fmt", fl.FORMATS, ids=[fl.NAMES[f] for f in fl.FORMATS])
def test_queue_refuses_misaligned_float_images_and_enqueues_nothing(fq, fmt):
    W, H = 64, 32
    row = fl.BPP[fmt] * W
    ctx = fq.ugsm_fake_create(2, 3, 8, 4)
    try:
        assert fq.ugsm_fake_set_input_format(ctx, fmt) == OK
        L, R, o = BASE, BASE + 65536, BASE + 131072
        cases = [(L + 1, R, row, BAD_ARG), (L + 2, R, row, BAD_ARG), (L, R + 1, row, BAD_ARG), (L, R + 2, row + 8, BAD_ARG),
                 (L, R, row + 2, BAD_ARG), (L, R, row + 1, BAD_ARG), (L, R, row - 4, SIZE_MISMATCH), (L, R, row - 1, SIZE_MISMATCH)]
        for l, r, stride, want in cases:
            assert fq.ugsm_enqueue_full(ctx, l, r, W, H, stride, o, 1) == want, (hex(l), hex(r), stride)
            assert fq.ugsm_enqueue_foveated(ctx, l, r, W, H, stride, 0, 0, o, None, None, 2) == want, (hex(l), hex(r), stride)
            assert fq.ugsm_fake_get_input_format(ctx) == fmt
        # a managed pair's host images: the pointer is looked at before anything is copied
        host = np.zeros(2 * row * H + 8, np.uint8)
        p = host.ctypes.data + (-host.ctypes.data % 4)
        assert fq.ugsm_enqueue_full_managed(ctx, p + 1, p + row * H, W, H, row, 3) == BAD_ARG
        assert fq.ugsm_enqueue_full_managed(ctx, p, p + row * H, W, H, row + 2, 3) == BAD_ARG
        w, f, u = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert fq.ugsm_queue_depth(ctx, C.byref(w), C.byref(f), C.byref(u)) == OK
        assert (w.value, f.value, u.value) == (0, 0, 0) and fq.ugsm_fake_calls(ctx) == 0
        # aligned at + 4, + 8, + 12 with a padded stride: accepted
        for k, shift in enumerate((4, 8, 12)):
            assert fq.ugsm_enqueue_full(ctx, L + shift, R + shift, W, H, row + 8, o, 10 + k) == OK
        # the 8-bit formats keep their freedom: any pointer, any stride that is large enough
        assert fq.ugsm_fake_set_input_format(ctx, 0) == OK
        assert fq.ugsm_enqueue_full(ctx, L + 1, R + 3, W, H, 3 * W + 1, o, 20) == OK
    finally:
        fq.ugsm_fake_destroy(ctx)


def test_fake_setter_knows_the_float_formats_and_no_others(fq):
    ctx = fq.ugsm_fake_create(1, 1, 8, 4)
    try:
        for f in (5, 6, 7, 10, 99):
            assert fq.ugsm_fake_set_input_format(ctx, f) == BAD_ARG
        for f in fl.FORMATS:
            assert fq.ugsm_fake_set_input_format(ctx, f) == OK and fq.ugsm_fake_get_input_format(ctx) == f
    finally:
        fq.ugsm_fake_destroy(ctx)
