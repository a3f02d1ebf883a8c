"""The resized cloud (ugsm_point_cloud_resized / ugsm_point_cloud_resized_fovea) without a GPU: the C-ABI's declarations and exports, the
host-only size rule, argument refusals, and the CPU restatement of INTER_CUBIC (tests/resize_np.py) against an independent float64
evaluation of the same kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resize_np as rn
from conftest import ROOT
from test_cloud_host import bad_argument_cases

NEW = ["ugsm_resized_cloud_points", "ugsm_point_cloud_resized", "ugsm_point_cloud_resized_fovea"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_resized_symbols_are_declared_and_exported_by_both_libraries(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
    for path in (lib.LIB_PATH, lib.DEV_LIB_PATH):
        so = C.CDLL(path)
        for name in NEW:
            assert hasattr(so, name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().ugsm_abi_version() == 6


def test_resized_cloud_points(lib):
    f = lambda W, H, k: lib.load().ugsm_resized_cloud_points(W, H, C.c_float(k))
    assert f(4928, 3264, 0.2) == 985 * 652 == lib.resized_cloud_points(4928, 3264, 0.2)
    assert f(615, 407, 0.2) == 123 * 81
    assert f(1920, 1080, 0.2) == 384 * 216
    assert f(7, 5, 0.2) == 1 and f(3, 3, 1.0) == 9
    for (W, H, k) in [(4928, 3264, 0.5), (317, 203, 0.3), (317, 203, 0.7), (33, 7, 1 / 3), (1000, 31, 1.0), (9, 9, 0.99)]:
        dw, dh = rn.resized_size(W, H, k)
        assert f(W, H, k) == dw * dh, (W, H, k)
    for bad in [(64, 32, 0.0), (64, 32, -0.2), (64, 32, 1.5), (64, 32, float("nan")), (64, 32, float("inf")), (4, 32, 0.2), (64, 4, 0.2),
                (0, 32, 0.5), (64, 0, 0.5), (-5, 32, 0.5)]:
        assert f(*bad) == -1, bad


def _call(lib, fovea=False, factor=0.2, colour_mapped=0, **over):
    """One ugsm_point_cloud_resized[_fovea] call with no context and plausible (fake, never dereferenced) device pointers."""
    P = (C.c_double * 12)(*range(12))
    a = dict(dx=0x10000, dy=0x20000, conf=0x30000, rgb=0x40000, W=64, H=32, stride=192, P1=P, P2=P,
             p=lib.cloud_params(), points=0x50000, cap=100, count=0x60000)
    a.update(over)
    p = C.byref(a["p"]) if a["p"] is not None else None
    so = lib.load()
    if fovea:
        return so.ugsm_point_cloud_resized_fovea(None, 0, a["dx"], a["dy"], a["conf"], 40, 20, 0, 8, 6, C.c_float(1.0), a["rgb"], a["W"],
                                                 a["H"], a["stride"], a["P1"], a["P2"], C.c_float(factor), colour_mapped, p, a["points"],
                                                 a["cap"], a["count"])
    return so.ugsm_point_cloud_resized(None, 0, a["dx"], a["dy"], a["conf"], a["rgb"], a["W"], a["H"], a["stride"], a["P1"], a["P2"],
                                       C.c_float(factor), p, a["points"], a["cap"], a["count"])


def resized_bad_argument_cases(lib):
    """The refusals the resized forms add to the cloud's (name, overrides): sampling, the factor, colour_mapped."""
    nan = float("nan")
    return [("sampling 2", dict(p=lib.cloud_params(sampling=2))), ("factor 0", dict(factor=0.0)), ("factor < 0", dict(factor=-0.5)),
            ("factor > 1", dict(factor=1.25)), ("factor NaN", dict(factor=nan)), ("factor inf", dict(factor=float("inf"))),
            ("a side truncates to 0", dict(factor=0.01)), ("colour_mapped 2", dict(colour_mapped=2))]


def test_bad_arguments_are_refused_without_a_device(lib):
    for fovea in (False, True):
        for name, over in bad_argument_cases(lib) + resized_bad_argument_cases(lib):
            if name == "colour_mapped 2" and not fovea:
                continue
            assert _call(lib, fovea=fovea, **over) == lib.UGSM_ERR_BAD_ARG, (name, fovea)
        assert _call(lib, fovea=fovea) == lib.UGSM_ERR_BAD_ARG      # (good arguments, no context)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def _keys64(plane, dw, dh):
    """Keys' cubic (a = -0.75) in float64 at OpenCV's sample positions ((d + 0.5) * scale - 0.5, rounded to float as resize.cpp
    stores them), replicate border: an evaluation independent of the restatement's float order, coefficients and tap tables."""
    def w(t):
        t = np.abs(t)
        a = -0.75
        return np.where(t <= 1, (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1, np.where(t < 2, a * t ** 3 - 5 * a * t ** 2 + 8 * a * t - 4 * a, 0.0))

    def matrix(n, m):
        u = ((np.arange(m) + 0.5) * (1.0 / (m / n)) - 0.5).astype(np.float32).astype(np.float64)
        M = np.zeros((m, n))
        for d in range(m):
            b = int(np.floor(u[d]))
            for k in range(b - 1, b + 3):
                M[d, min(max(k, 0), n - 1)] += w(u[d] - k)
        return M
    ph, pw = plane.shape
    return matrix(ph, dh) @ plane.astype(np.float64) @ matrix(pw, dw).T


@pytest.mark.parametrize("W,H,f", [(317, 203, 0.2), (317, 203, 0.3), (100, 64, 1 / 3), (50, 37, 0.5), (41, 29, 0.7), (3, 3, 0.7),
                                   (7, 5, 0.2), (64, 48, 0.99)])
def test_restatement_matches_float64_keys(W, H, f):
    """Within 4e-6 of the plane's largest magnitude: float32 rounding of a 4 x 4 weighted sum whose weights' magnitudes sum below 1.6."""
    rng = np.random.Generator(np.random.PCG64(W * 31 + H))
    plane = rng.uniform(-3, 5, (H, W)).astype(np.float32)
    dw, dh = rn.resized_size(W, H, f)
    got = rn.resize_cubic(plane, dw, dh)
    assert got.dtype == np.float32 and got.shape == (dh, dw)
    ref = _keys64(plane, dw, dh)
    err = np.abs(got - ref).max()
    assert err <= 4e-6 * np.abs(plane).max(), err
    # a constant plane stays constant to rounding (the weights sum to 1)
    c = rn.resize_cubic(np.full((H, W), 2.5, np.float32), dw, dh)
    assert np.abs(c - 2.5).max() <= 4e-6


def test_taps_at_f_0_2_are_disjoint():
    """At f = 0.2 on 16 MP neighbouring output columns share no tap (sx steps by at least 4), and no column is a border column."""
    for n in (4928, 3264):
        s, c, border = rn.tap_table(n, rn.resized_size(n, n, 0.2)[0])
        assert (np.diff(s) >= 4).all() and s[0] >= 1 and s[-1] + 2 < n
        assert not border.any()
    s, c, border = rn.tap_table(3, 2)                          # 3 -> 2: fx 0.25 and 1.75, both clamped
    assert s.tolist() == [0, 1] and border.tolist() == [True, True]


def test_border_columns_start_from_plus_zero():
    """15 x 9 -> 5 x 3 (scale 3, fraction 0: coefficients +0, 1, +0, +0): every product of a -0.0 plane is -0.0, so the interior sums
    are -0.0f; the border column (sx + 2 >= 15) starts from +0.0f and reads +0.0f."""
    plane = np.full((9, 15), -0.0, np.float32)
    s, c, border = rn.tap_table(15, 5)
    assert s.tolist() == [1, 4, 7, 10, 13] and border.tolist() == [False, False, False, False, True]
    assert c[0].tolist() == [0.0, 1.0, 0.0, 0.0]
    out = rn.resize_cubic(plane, 5, 3)
    assert (out == 0).all() and (np.signbit(out) == ~border[None, :]).all()


def test_nan_and_inf_propagate_through_zero_coefficients():
    plane = np.ones((10, 10), np.float32)
    plane[4, 4] = np.inf
    out = rn.resize_cubic(plane, 5, 5)        # f = 0.5: fx 0.5, every coefficient nonzero
    assert np.isinf(out).any() or np.isnan(out).any()
    plane[4, 4] = np.nan
    assert np.isnan(rn.resize_cubic(plane, 5, 5)).sum() >= 1


def test_factor_one_is_an_identity():
    """cv::resize copies when the size does not change: at f = 1 the resized plane is the plane, on finite planes and non-finite ones
    alike; and the full generic path at a factor just under 1 stays within rounding of a finite plane."""
    rng = np.random.Generator(np.random.PCG64(3))
    plane = rng.normal(0, 4, (37, 53)).astype(np.float32)
    assert rn.resized_size(53, 37, 1.0) == (53, 37)
    assert np.array_equal(rn.resize_cubic(plane, 53, 37).view(np.uint32), plane.view(np.uint32))
    plane[3, 7], plane[10, 0], plane[0, 52] = np.inf, np.nan, -np.inf
    got = rn.resize_cubic(plane, 53, 37)
    assert np.array_equal(got.view(np.uint32), plane.view(np.uint32))


def test_sample_positions_pin_the_float_division():
    """xx = (int)((float)ii / f) in float32.  At f = 0.2 that is 5 ii exactly, where binary64 division by the same float would give
    5 ii - 1; at 0.3 it rounds 3 / 0.3f up to 10; neither is round(ii / f)."""
    x = rn.sample_at(40, 0.2)
    assert x.tolist() == list(range(0, 40, 5))
    d64 = (np.arange(8) / np.float64(np.float32(0.2))).astype(int)
    assert d64.tolist() == [0, 4, 9, 14, 19, 24, 29, 34]
    x = rn.sample_at(40, 0.3)
    assert x.tolist() == [0, 3, 6, 10, 13, 16, 20, 23, 26, 29, 33, 36]
    assert np.nonzero(x != np.round(np.arange(12) / 0.3).astype(int))[0].tolist() == [2, 5, 8, 9, 11]
    assert np.nonzero(x != (np.arange(12) / np.float64(np.float32(0.3))).astype(int))[0].tolist() == [3, 6]
    x = rn.sample_at(40, 0.7)
    assert x[:10].tolist() == [0, 1, 2, 4, 5, 7, 8, 10, 11, 12]
    assert np.nonzero(x != np.round(np.arange(28) / 0.7).astype(int))[0].tolist() == [2, 4, 6, 9, 11, 13, 16, 18, 20, 23, 25, 27]
    assert rn.sample_at(4928, 0.2)[-1] == 4920 and rn.sample_at(3264, 0.2)[-1] == 3255


def test_restatement_cloud_on_hand_planes():
    """The cloud's order and contents on a plane whose X names the pixel: X of point (ii, jj) is the pixel (xx, yy)'s, Z the resized
    map's, the colour the pixel's."""
    H, W = 15, 20
    y, x = np.mgrid[0:H, 0:W]
    xyz = np.stack([(100 * x + y), -x, (1 + x + y)]).astype(np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = x, y, 7
    r = rn._resized_records(xyz, rn.colour_word(rgb), None, 0.2)
    assert r.size == 4 * 3
    exp_x = [100 * (5 * i) + 5 * j for i in range(4) for j in range(3)]
    assert r["x"].tolist() == exp_x
    assert r["rgb"].tolist() == [(5 * i) << 16 | (5 * j) << 8 | 7 for i in range(4) for j in range(3)]
    Z = rn.resize_cubic(xyz[2], 4, 3)
    assert r["z"].tolist() == Z.T.reshape(-1).tolist()
    # Z = 1 + x + y is linear, and the cubic reproduces it at the taps' centre: sx + 0.5 = 5 ii + 2 (the registration quirk)
    assert np.allclose(Z[1:2, 1:3], 1 + (5 * np.arange(1, 3) + 2) + (5 * 1 + 2), atol=1e-5)
