"""The HIP kernels against what the REFERENCE'S OWN stage code gave, bit for bit.

tests/golden/ref_stages.npz holds uint8 images, float seed fields and the outputs of the reference's MatchLib.cu, compiled for the CPU
(oracle/ref_cpu/, tests/golden/make_golden.py) and composed in the order of MatchGPULib.cpp by tests/ref_stages.py: two iterations of a
level (mi = 4, S = 5, with and without is_top) at 37 x 29, 61 x 45 and 130 x 75, pyramid levels 1 to 3, seeds, one to five smoothing passes.
Only that file is read here.  Every K-cost and K-smooth form is driven over the iterate cases, with the kernel that ran asserted from
kernel_stats(); tests/test_ref_pin_host.py holds the oracle and the numpy restatement to the same file on the CPU.
"""
import numpy as np
import pytest

from conftest import assert_bit_equal, load_golden
from test_gpu_march import iterate, run_smooth
from test_gpu_small import stats_names

pytestmark = pytest.mark.gpu

MI, S = 4, 5

# (context arguments, development overrides, kernels that must have run, kernels that must not)
FORMS = {
    "default": (dict(), {}, {"k_cost_small", "k_smooth_small"}, set()),
    "lds_tiled": (dict(small_max_pixels=-1), {}, {"k_smooth_fused"}, {"k_cost_small", "k_smooth_small"}),
    "march": (dict(), {"UGSM_MARCH_MIN_PIXELS": "1"}, {"k_cost_march"}, {"k_cost_small", "k_cost_march4"}),
    "march4": (dict(), {"UGSM_MARCH4": "1,2000000000"}, {"k_cost_march4"}, {"k_cost_small", "k_cost_march"}),
    "small_mask_1": (dict(), {"UGSM_SMALL_MASK": "1"}, {"k_cost_small", "k_smooth_fused"}, {"k_smooth_small"}),
    "kernel_path_1": (dict(kernel_path=1), {}, {"k_cost_ref", "k_smooth_pass", "k_box"}, {"k_cost_small", "k_smooth_small", "k_smooth_fused"}),
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_stages.npz")


def planes(rgb):
    return np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(np.float32)


@pytest.mark.parametrize("form", list(FORMS))
def test_iterate_every_kernel_form(lib, gold, monkeypatch, form):
    """ugsm_stage_iterate, two iterations, 61 x 45 and 130 x 75, is_top 0 and 1, on one K-cost / K-smooth form."""
    kw, env, must, must_not = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with lib.Context(levels=1, profile_events=2, **kw) as c:
        for case in ("61x45", "130x75"):
            pl, pr, d0 = planes(gold[case + "_L"]), planes(gold[case + "_R"]), gold[case + "_d0"]
            for top in (0, 1):
                assert_bit_equal(iterate(c, pl, pr, d0, MI, S, top, 1, 2), gold[f"{case}_top{top}"], f"{form} {case} is_top={top}")
        names = stats_names(c)
    print(form, sorted(names))
    assert must <= names and not (must_not & names), f"{form}: ran {sorted(names)}"


def test_iterate_correlation_planes_and_update(lib, gold):
    """The five Q planes and (dx', dy', kappa) of the second iteration at 37 x 29 (the one-kernel-per-stage path writes them out)."""
    from test_gpu_parity import run_iterate
    pl, pr, d0 = planes(gold["37x29_L"]), planes(gold["37x29_R"]), gold["37x29_d0"]
    with lib.Context(levels=1, kernel_path=1) as c:
        for top in (0, 1):
            out, dbg = run_iterate(c, pl, pr, d0, MI, S, top, 1, 2, want_dbg=True)
            assert_bit_equal(dbg[:5], gold[f"37x29_Q_top{top}"], f"Q is_top={top}")
            assert_bit_equal(dbg[5:], gold[f"37x29_nd_top{top}"], f"(dx', dy', kappa) is_top={top}")
            assert_bit_equal(out, gold[f"37x29_top{top}"], f"field is_top={top}")
    with lib.Context(levels=1) as c:
        for top in (0, 1):
            assert_bit_equal(iterate(c, pl, pr, d0, MI, S, top, 1, 2), gold[f"37x29_top{top}"], f"default form, field is_top={top}")


def test_iterate_rgb8_level0_form(lib, gold, monkeypatch):
    """ugsm_stage_iterate_rgb8 (libugsm_dev.so): the 8-bit instances of K-cost and of A = G * L^2 read the images themselves, 130 x 75."""
    monkeypatch.setenv("UGSM_MARCH4", "0,0")  # every level to k_cost_march, whose 8-bit instance this entry point runs
    L, R, d0 = gold["130x75_L"], gold["130x75_R"], gold["130x75_d0"]
    H, W, _ = L.shape
    with lib.Context(levels=1, march_min_pixels=1, profile_events=2, dev=True) as c:
        dl, dr = c.to_device(L), c.to_device(R)
        try:
            for top in (0, 1):
                pd = c.to_device(d0)
                try:
                    c.check(c.lib.ugsm_stage_iterate_rgb8(c.handle, dl, dr, 3 * W, pd, W, H, MI, S, top, 1, 2))
                    assert_bit_equal(c.to_host(pd, (3, H, W)), gold[f"130x75_top{top}"], f"rgb8 is_top={top}")
                finally:
                    c.free(pd)
        finally:
            c.free(dl)
            c.free(dr)
        assert "k_cost_march" in stats_names(c), stats_names(c)


@pytest.mark.parametrize("form", ["default", "lds_tiled", "kernel_path_1"])
def test_smooth_one_to_five_passes_with_and_without_the_box(lib, gold, form):
    """ugsm_stage_smooth on a field with zero, negative and 1e-30 confidences (0/0 spreads as NaN, as in the reference's smoothKernel)."""
    kw, _, _, _ = FORMS[form]
    src = gold["smooth_src"]
    with lib.Context(levels=1, profile_events=2, **kw) as c:
        for passes in range(1, 6):
            for box in (0, 1):
                assert_bit_equal(run_smooth(c, src, passes, box), gold[f"smooth_p{passes}_b{box}"], f"{form} passes={passes} box={box}")
        names = stats_names(c)
    want = {"default": "k_smooth_small", "lds_tiled": "k_smooth_fused", "kernel_path_1": "k_smooth_pass"}[form]
    assert want in names, f"{form}: ran {sorted(names)}"


@pytest.mark.parametrize("path", [0, 1])
def test_pyramid_levels_one_to_three(lib, gold, path):
    img = gold["130x75_L"]
    H, W, _ = img.shape
    with lib.Context(levels=4, kernel_path=path) as c:
        p = c.to_device(img)
        try:
            for lev in (1, 2, 3):
                exp = gold[f"pyr{lev}"]
                out = c.alloc(exp.nbytes)
                try:
                    c.check(c.lib.ugsm_stage_pyramid(c.handle, p, W, H, img.strides[0], lev, out))
                    assert_bit_equal(c.to_host(out, exp.shape), exp, f"path {path} level {lev}")
                finally:
                    c.free(out)
        finally:
            c.free(p)


@pytest.mark.parametrize("path", [0, 1])
def test_seed(lib, gold, path):
    """ugsm_stage_seed against subsampleDispGPU: to the next level's size, to an odd size, and upsampled then cropped as a fovea level is."""
    src = gold["37x29_d0"]
    with lib.Context(levels=2, fovea_levels=2, kernel_path=path) as c:
        p = c.to_device(src)
        try:
            for key in ("seed_53x42", "seed_52x41"):
                exp = gold[key]
                _, H2, W2 = exp.shape
                q = c.alloc(exp.nbytes)
                try:
                    c.check(c.lib.ugsm_stage_seed(c.handle, p, 37, 29, q, W2, H2, 0, 0, 0, 0))
                    assert_bit_equal(c.to_host(q, exp.shape), exp, f"path {path} {key}")
                finally:
                    c.free(q)
            q = c.alloc(src.nbytes)
            try:
                c.check(c.lib.ugsm_stage_seed(c.handle, p, 37, 29, q, 37, 29, 53, 42, 8, 7))
                assert_bit_equal(c.to_host(q, src.shape), gold["seed_53x42"][:, 7:7 + 29, 8:8 + 37], f"path {path} fovea seed")
            finally:
                c.free(q)
        finally:
            c.free(p)
