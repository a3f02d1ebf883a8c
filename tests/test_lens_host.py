"""Lens distortion (ugsm_set_lens, ugsm_get_lens, ugsm_undistort_points; include/ugsm.h, "lens distortion") without a GPU: the numpy
restatement of the closed form against the oracle, the host statement of the definition against the numpy one, the zero-D identity, the
round trip, the purpose on synthetic ground truth, and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lens_np as ln
from conftest import ROOT

NEW = ["ugsm_set_lens", "ugsm_get_lens", "ugsm_undistort_points"]
WILD = (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40)   # tests/test_gpu_depth.py's
W, H = 97, 131
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def rigs():
    return ln.rigs()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def frame_points(rig, n=100000, seed=5):
    """Corners, edge midpoints and centre of the frame, n random float32 coordinates reaching 300 px outside it, NaN and +-inf."""
    w, h = rig["width"], rig["height"]
    xs, ys = (0, (w - 1) / 2, w - 1), (0, (h - 1) / 2, h - 1)
    fixed = [(x, y) for y in ys for x in xs]
    rng = np.random.Generator(np.random.PCG64(seed))
    rnd = np.stack([rng.uniform(-300, w + 300, n), rng.uniform(-300, h + 300, n)], axis=1)
    odd = [(np.nan, 10.0), (10.0, np.nan), (np.inf, 5.0), (5.0, -np.inf), (-np.inf, np.inf), (np.nan, np.nan)]
    return np.concatenate([np.array(fixed), rnd, np.array(odd)]).astype(F32)


def test_lens_symbols_are_declared_and_exported_by_both_libraries(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().ugsm_abi_version() == 6
    assert "lens distortion" in hdr and "not pinned against OpenCV" in hdr


def test_tri_point_restatement_is_the_oracle_without_a_lens(orc, rigs):
    """1. lens_np.tri_point with no lens equals oracle.triangulate and oracle.triangulate_fovea bit for bit (a NaN equals any NaN): the new
    yardstick is pinned to the old one."""
    rng = np.random.Generator(np.random.PCG64(11))
    dx = rng.normal(-40, 12, (H, W)).astype(F32)
    dy = rng.normal(0, 2, (H, W)).astype(F32)
    for a in (dx, dy):
        for v in WILD:
            a.flat[rng.integers(0, a.size, a.size // 80)] = v
    for rig in rigs.values():
        exp, got = orc.triangulate(dx, dy, rig["P1"], rig["P2"]), ln.triangulate(dx, dy, rig["P1"], rig["P2"])
        assert same_bits(got, exp).all()
        assert np.isnan(exp).any() and np.isfinite(exp).mean() > 0.5
    sx = rng.normal(-12, 4, (4, H, W)).astype(F32)      # (the fovea form truncates to int: finite and far inside its range)
    sy = rng.normal(0, 1.5, (4, H, W)).astype(F32)
    for level, (left, upper, scale) in enumerate([(10, 7, 1.0), (-3, 5, F32(1.41421356)), (40, -20, F32(2.0)), (0, 0, F32(2.8284271))]):
        for rig in rigs.values():
            exp = orc.triangulate_fovea(sx, sy, level, left, upper, scale, rig["P1"], rig["P2"])
            got = ln.triangulate_fovea(sx, sy, level, left, upper, scale, rig["P1"], rig["P2"])
            assert same_bits(got, exp).all(), level


@pytest.mark.parametrize("iterations", [1, 5, 12])
def test_undistort_points_is_the_numpy_definition(lib, rigs, iterations):
    """2. ugsm_undistort_points equals lens_np.undistort bit for bit (NaN equals NaN) for both rigs and both cameras."""
    for name, rig in rigs.items():
        uv = frame_points(rig)
        for K, D in ((rig["K1"], rig["D1"]), (rig["K2"], rig["D2"])):
            got = lib.undistort_points(K, D, uv, iterations)
            eu, ev = ln.undistort(K, D, uv[:, 0], uv[:, 1], iterations)
            assert same_bits(got[:, 0], eu).all() and same_bits(got[:, 1], ev).all(), name
            moved = np.hypot(got[:9, 0] - uv[:9, 0], got[:9, 1] - uv[:9, 1])
            assert moved[[0, 2, 6, 8]].min() > 1.0 and moved[4] < 1.0, moved     # the corners move, the centre hardly
    assert lib.undistort_points(rig["K1"], rig["D1"], uv, 0).tobytes() == lib.undistort_points(rig["K1"], rig["D1"], uv, 5).tobytes()   # 0: the default


def test_zero_distortion_is_the_identity_byte_for_byte(lib, rigs):
    """3. With all five coefficients zero the output bytes are the input bytes on the coordinates of test 2 -- with two exceptions that follow
    from the definition itself, which the library must not special-case:
      - a coordinate of magnitude below 2^-10 px, the frame's exact 0 among them: the float64 round trip ((u - cx) / fx) * fx + cx errs by up
        to four roundings of values below 2^13, 2^-38 px, which only exceeds half a float32 ulp for |u| < 2^-14.  There the result is held to
        within 2^-36 px of the input (column 0 comes back as some 1e-13, not 0);
      - a point with a NaN or an infinite coordinate: r2 is NaN or inf and 0 * inf is NaN, so both coordinates come back NaN.
    Both are held to the numpy definition bit for bit as well."""
    for rig in rigs.values():
        uv = frame_points(rig)
        finite = np.isfinite(uv).all(axis=1)
        strict = finite & (np.abs(uv) >= 2.0 ** -10).all(axis=1)
        assert strict.sum() >= 100000 and (~finite).sum() == 6 and (finite & ~strict).sum() >= 5      # (the five frame points in row or column 0)
        for K in (rig["K1"], rig["K2"]):
            for it in (1, 5, 12):
                got = lib.undistort_points(K, np.zeros(5), uv, it)
                assert got[strict].tobytes() == uv[strict].tobytes()
                assert np.abs(got[finite].astype(F64) - uv[finite].astype(F64)).max() <= 2.0 ** -36
                eu, ev = ln.undistort(K, np.zeros(5), uv[:, 0], uv[:, 1], it)
                assert np.isnan(got[~finite]).all() and same_bits(got[:, 0], eu).all() and same_bits(got[:, 1], ev).all()


def round_trip(lib, rig, K, D, iterations):
    """max distance, in pixels, between (u, v) and the forward-distorted ugsm_undistort_points(u, v) over the frame."""
    w, h = rig["width"], rig["height"]
    rng = np.random.Generator(np.random.PCG64(21))
    uv = np.stack([rng.uniform(0, w - 1, 50000), rng.uniform(0, h - 1, 50000)], axis=1).astype(F32)
    und = lib.undistort_points(K, D, uv, iterations).astype(F64)
    bu, bv = ln.distort64(K, D, und[:, 0], und[:, 1])
    return float(np.hypot(bu - uv[:, 0].astype(F64), bv - uv[:, 1].astype(F64)).max())


def test_round_trip(lib, rigs):
    """4. 16 MP rig, 5 iterations: forward-distorting (u', v') in float64 comes back to (u, v) within 2^-11 px, one float32 ulp of a coordinate in
    [4096, 8192) -- twice the rounding floor of u' itself (2.5e-4 px).  Small rig: 12 iterations are no worse than 5."""
    rig = rigs["rig16mp"]
    for K, D in ((rig["K1"], rig["D1"]), (rig["K2"], rig["D2"])):
        e5 = round_trip(lib, rig, K, D, 5)
        print(f"round trip, 16 MP rig, 5 iterations: {e5:.3e} px; 8: {round_trip(lib, rig, K, D, 8):.3e}; 20: {round_trip(lib, rig, K, D, 20):.3e}")
        assert e5 <= 2.0 ** -11
    rig = rigs["small"]
    for K, D in ((rig["K1"], rig["D1"]), (rig["K2"], rig["D2"])):
        e5, e12 = round_trip(lib, rig, K, D, 5), round_trip(lib, rig, K, D, 12)
        print(f"round trip, small rig: 5 iterations {e5:.3e} px, 12 iterations {e12:.3e} px")
        assert e12 <= e5


def purpose_errors(rig, iterations, visible_only=False):
    """max |Z - Z_true| / Z_true over a 17 x 13 grid of integer left pixels at Z in {0.8, 1.5, 3}: with the lens, without it, and for points built
    with D = 0 and triangulated without a lens (the closed form's own float32 error).  visible_only: only the correspondences whose right
    position lies inside the right camera's frame."""
    w, h = rig["width"], rig["height"]
    P1, P2 = rig["P1"], rig["P2"]
    gx, gy = np.meshgrid(np.linspace(0, w - 1, 17).round(), np.linspace(0, h - 1, 13).round())
    u1, v1 = gx.reshape(-1).astype(F64), gy.reshape(-1).astype(F64)
    zero = np.zeros(5)

    def build(D1, D2, Z):
        """dx, dy (float32) of the points on the left pixels' rays at depth Z, as cameras with D1, D2 see them, and which of them the right
        camera's frame holds."""
        iu, iv = ln.undistort64(rig["K1"], D1, u1, v1, 30)                  # the ideal left pixel
        ray = np.stack([(iu - P1[0, 2]) / P1[0, 0], (iv - P1[1, 2]) / P1[1, 1], np.ones_like(iu)]) * Z   # P1 = K1 [I | 0]
        q = P2 @ np.vstack([ray, np.ones_like(iu)[None]])
        u2, v2 = ln.distort64(rig["K2"], D2, q[0] / q[2], q[1] / q[2])
        seen = (u2 >= 0) & (u2 <= w - 1) & (v2 >= 0) & (v2 <= h - 1) if visible_only else np.ones(u2.shape, bool)
        return (u2 - u1).astype(F32), (v2 - v1).astype(F32), seen

    def err(dx, dy, seen, Z, lens):
        x1, y1 = u1.astype(F32), v1.astype(F32)
        z = ln.tri_lens(x1, y1, x1 + dx, y1 + dy, P1, P2, lens)[2].astype(F64)
        return float(np.abs(z - Z)[seen].max() / Z)

    with_lens = without = ref = 0.0
    for Z in (0.8, 1.5, 3.0):
        dx, dy, seen = build(rig["D1"], rig["D2"], Z)
        assert seen.sum() >= 100
        with_lens = max(with_lens, err(dx, dy, seen, Z, ln.lens_of(rig, iterations)))
        without = max(without, err(dx, dy, seen, Z, None))
        dx0, dy0, seen0 = build(zero, zero, Z)
        ref = max(ref, err(dx0, dy0, seen0, Z, None))
    return with_lens, without, ref


def test_the_lens_corrects_the_range_on_synthetic_ground_truth(rigs):
    """5. At 16 MP with the rig's calibration: the range error with the lens is within twice the closed form's own float32 error (the margin is
    for the float32 rounding of the four undistorted coordinates), and the error without the lens is larger.

    The grid's rays at Z = 0.8 meet the right image up to 1437 px LEFT of its frame, where no camera sees them and the fixed-point iteration
    converges more slowly than anywhere inside a frame.  So the bound is asserted twice: over the whole grid with 12 iterations, and with the
    default 5 over the correspondences both cameras can see (at least 152 of the 221 at every Z).  Measured here: 12 iterations, whole grid
    1.27e-6 with the lens, 8.0e-2 without, 1.75e-6 the closed form's own; 5 iterations, visible correspondences 1.27e-6, 1.76e-2, 1.75e-6;
    5 iterations over the whole grid 1.2e-4 (8 iterations: 2.1e-6) -- a point outside the right frame, not a correspondence."""
    rig = rigs["rig16mp"]
    assert np.array_equal(rig["P1"][:, :3], rig["K1"]) and not rig["P1"][:, 3].any()
    for iterations, visible_only in ((12, False), (5, True)):
        with_lens, without, ref = purpose_errors(rig, iterations, visible_only)
        print(f"relative range error at 16 MP, {iterations} iterations, {'visible correspondences' if visible_only else 'whole grid'}: "
              f"with the lens {with_lens:.3e}, without it {without:.3e}, the closed form's own {ref:.3e}")
        assert with_lens <= 2 * ref
        assert without > with_lens
    print(f"5 iterations over the whole grid: {purpose_errors(rig, 5)[0]:.3e}; 8: {purpose_errors(rig, 8)[0]:.3e}")


def test_undistort_points_refuses_bad_arguments(lib, rigs):
    """6. NULL, n < 0, non-finite K or D, fx <= 0, iterations 33 and -1."""
    so, BAD = lib.load(), lib.UGSM_ERR_BAD_ARG
    rig = rigs["small"]
    dbl = lambda a: (C.c_double * len(a))(*a)                                        # noqa: E731
    K, D = list(rig["K1"].reshape(-1)), list(rig["D1"])
    uv = np.array([[1.0, 2.0], [3.0, 4.0]], F32)
    out = np.full_like(uv, -7.0)
    call = lambda k, d, it, n=2, i=uv.ctypes.data, o=None: so.ugsm_undistort_points(k, d, it, i, out.ctypes.data if o is None else o, n)   # noqa: E731
    assert call(dbl(K), dbl(D), 5) == lib.UGSM_OK and (out != -7.0).all()
    assert call(dbl(K), dbl(D), 5, n=0, i=None, o=0) == lib.UGSM_OK                     # (nothing to do)
    out[:] = -7.0
    assert call(None, dbl(D), 5) == BAD and call(dbl(K), None, 5) == BAD
    assert call(dbl(K), dbl(D), 5, i=None) == BAD and call(dbl(K), dbl(D), 5, o=0) == BAD
    assert call(dbl(K), dbl(D), 5, n=-1) == BAD
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 2, 8):
            assert call(dbl(K[:k] + [bad] + K[k + 1:]), dbl(D), 5) == BAD
        for k in (0, 4):
            assert call(dbl(K), dbl(D[:k] + [bad] + D[k + 1:]), 5) == BAD
    for fx in (0.0, -150.0):
        assert call(dbl([fx] + K[1:]), dbl(D), 5) == BAD
        assert call(dbl(K[:4] + [fx] + K[5:]), dbl(D), 5) == BAD
    assert call(dbl(K), dbl(D), 33) == BAD and call(dbl(K), dbl(D), -1) == BAD
    assert call(dbl(K), dbl(D), 32) == lib.UGSM_OK and call(dbl(K), dbl(D), 1) == lib.UGSM_OK
    out[:] = -7.0
    assert call(dbl(K), dbl(D), 33) == BAD and (out == -7.0).all()                      # (a refused call writes nothing)
    with pytest.raises(lib.UgsmError):
        lib.undistort_points(rig["K1"], rig["D1"], uv, 40)
    so.ugsm_get_lens.restype = C.c_int
    assert so.ugsm_set_lens(None, None, None, None, None, 0) == BAD and so.ugsm_get_lens(None, None, None, None, None, None, None) == BAD
