"""The C-ABI library without a GPU: it loads, exports every symbol include/ugsm.h declares, and
its pure-host geometry agrees with the oracle.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

# the k_* symbol set of the shipped library and the shipped .hip files, exactly
PRODUCT_KERNELS = {"k_cost_march", "k_cost_march4", "k_cost_small", "k_smooth_small", "k_smooth_fused", "k_pyr_base", "k_pyr_base_march", "k_blur_decimate2",
                   "k_blur_decimate_tiled", "k_sqblur_tiled", "k_range_scan", "k_seed", "k_copy_view", "k_lr_check", "k_rgb_planes", "k_triangulate",
                   "k_triangulate_fovea", "k_upsample_paste", "k_wdiff_rows", "k_wdiff_total",
                   "k_restrict", "k_prolong", "k_level0_windows", "k_warp_right", "k_residual_rows", "k_residual_total", "k_upsample_paste_multi",
                   "k_restrict_stack", "k_cloud", "k_cloud_fovea", "k_cloud_stack", "k_cloud_pairs", "k_cloud_stack_pairs", "k_cloud_multi"}
SHIPPED_HIP = ["ugsm_kernels_aux.hip", "ugsm_kernels_cloud.hip", "ugsm_kernels_depth.hip", "ugsm_kernels_fields.hip", "ugsm_kernels_march.hip", "ugsm_kernels_march4.hip",
               "ugsm_kernels_pyr.hip", "ugsm_kernels_small.hip", "ugsm_kernels_smooth.hip", "ugsm_kernels_warp.hip"]


def library_kernels(path):   # the kernels' mangled names: _ZN4ugsm<len>k_name...
    blob = open(path, "rb").read()
    return set(name[:int(n)].decode() for n, name in re.findall(rb"_ZN4ugsm(\d+)(k_[a-z_0-9]+)", blob))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ugsm.h")).read()
    declared = sorted(set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 30
    assert sorted(lib.EXPORTS) == declared, "ug_stereomatcher_amd/_lib.py EXPORTS out of date with include/ugsm.h"
    so = C.CDLL(lib.LIB_PATH)
    for name in declared:
        assert hasattr(so, name), f"{name} declared in ugsm.h but not exported by libugsm.so"
    assert lib.load().ugsm_abi_version() == 6
    assert lib.load().ugsm_is_dev_library() == 0
    # ... and NOTHING else (-fvisibility=hidden + csrc/ugsm.map): no ugsm::launch_*, no __device_stub__*, no kernel handles
    import shutil
    import subprocess
    nm = shutil.which("nm")
    if nm:
        for path, extra in ((lib.LIB_PATH, []), (lib.DEV_LIB_PATH, lib.DEV_EXPORTS)):
            out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            names = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
            assert names == sorted(declared + extra), sorted(set(names) ^ set(declared + extra))


def test_dev_header_symbols_are_exported_by_the_dev_library_only(lib):
    """include/ugsm_dev.h: libugsm_dev.so = everything ugsm.h declares + the probe entry points; libugsm.so has none of those."""
    hdr = open(os.path.join(ROOT, "include", "ugsm_dev.h")).read()
    declared = sorted(set(re.findall(r"\b(ugsm_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == sorted(lib.DEV_EXPORTS)
    dev, prod = C.CDLL(lib.DEV_LIB_PATH), C.CDLL(lib.LIB_PATH)
    for name in declared:
        assert hasattr(dev, name), f"{name} declared in ugsm_dev.h but not exported by libugsm_dev.so"
        assert not hasattr(prod, name), f"{name} is a development entry point but libugsm.so exports it"
    for name in lib.EXPORTS:
        assert hasattr(dev, name)
    assert lib.load(dev=True).ugsm_is_dev_library() == 1 and lib.load(dev=True).ugsm_abi_version() == 6


def test_product_library_holds_no_development_kernel(lib):
    """the one-kernel-per-stage path, round 1's LDS-tiled K-cost and the probe kernels are csrc/dev/ and in
    libugsm_dev.so only; the library a maintainer links carries only kernels a configuration of include/ugsm.h can launch, and the measured
    negatives of rounds 2-5 (k_smooth_march, k_smooth_pipe, k_iter_small, the one-thread-per-quad k_cost_fused) are in neither."""
    prod, dev = library_kernels(lib.LIB_PATH), library_kernels(lib.DEV_LIB_PATH)
    banned = {"k_cost_split", "k_poly_probe", "k_div3_probe", "k_div_probe", "k_cost_ref", "k_warp", "k_smooth_pass", "k_box", "k_sqblur_clamp", "k_blur_decimate"}
    gone = {"k_smooth_march", "k_smooth_pipe", "k_iter_small", "k_cost_fused"}
    assert not (prod & (banned | gone)), sorted(prod & (banned | gone))
    assert banned <= dev, sorted(banned - dev)
    assert not (dev & gone), sorted(dev & gone)
    assert prod == PRODUCT_KERNELS, sorted(prod ^ PRODUCT_KERNELS)          # the k_* symbol set of the shipped library, exactly
    assert dev == PRODUCT_KERNELS | banned, sorted(dev ^ (PRODUCT_KERNELS | banned))


def test_a_kernel_name_is_one_operation(lib):
    """The pins above keep development kernels out of the product; they do not ban a new name or a new file.  A new operation gets a kernel
    of its own name -- equal to its class in the kernel statistics where it has one -- not an overload of a kernel that does something else:
    over the shipped .hip files every __global__ name is defined in one file, and once, but for k_lr_check's two forms (one operation on a
    field and on a stack, tests/test_lr_fovea_host.py); and every kernel class of the statistics names a kernel of the library."""
    csrc = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")
    where = {}
    for f in SHIPPED_HIP:
        for name in re.findall(r"__global__[^\n]*\bvoid (k_[a-z_0-9]+)\(", open(os.path.join(csrc, f)).read()):
            where.setdefault(name, []).append(f)
    assert set(where) == PRODUCT_KERNELS, sorted(set(where) ^ PRODUCT_KERNELS)
    assert all(len(set(fs)) == 1 for fs in where.values()), {k: fs for k, fs in where.items() if len(set(fs)) > 1}
    assert {k: len(fs) for k, fs in where.items() if len(fs) > 1} == {"k_lr_check": 2}
    runtime = open(os.path.join(csrc, "ugsm_runtime.cpp")).read()
    classes = re.findall(r'"([^"]+)"', re.search(r"kClassName\[2\]\[KC_COUNT\] = \{\s*\{(.*?)\}", runtime, re.S).group(1))
    named = [c for c in classes if c.startswith("k_") and c != "k_cost_split"]   # (k_cost_split: libugsm_dev.so's, banned above)
    assert len(named) >= 12 and "k_restrict_stack" in named
    prod = library_kernels(lib.LIB_PATH)
    for c in named:
        assert any(k.startswith(c) for k in prod), c


def test_product_kernel_sources_hold_no_development_switch():
    """the shipped .hip files compile with no -D probe macro recognised -- no preprocessor conditional at all -- and libugsm_dev.so
    is those same files plus csrc/dev/.  The same OBJECTS: what make would run (a dry run: nothing is compiled) compiles every source once,
    with no -D, and the two libraries are two links that differ only in the objects they name."""
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert files == SHIPPED_HIP
    for f in files:
        src = open(os.path.join(csrc, f)).read()
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", src, re.M), f
    every = [os.path.join(d, f) for d in (csrc, os.path.join(csrc, "dev")) for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))]
    assert len(every) > 30
    for f in every:
        src = open(f).read()
        assert not re.search(r"UGSM_DEV_(LIB|KERNELS)", src), f   # (the two macros that once told the libraries apart)
    make = shutil.which("make")
    assert make, "make: the build's own tool"
    plan = subprocess.run([make, "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout
    cmds = [line.split() for line in plan.splitlines() if "hipcc" in line.split(" ")[0]]
    compiles, links = [c for c in cmds if "-c" in c], [c for c in cmds if "-shared" in c]
    assert len(compiles) + len(links) == len(cmds) and not [c for c in compiles if "-shared" in c]
    assert not [a for c in cmds for a in c if a.startswith("-D")]
    srcs = lambda c: [os.path.relpath(a, csrc) for a in c if a.endswith((".hip", ".cpp"))]
    assert all(len(srcs(c)) == 1 for c in compiles)
    compiled = sorted(srcs(c)[0] for c in compiles)
    # every source file of csrc/ and csrc/dev/ is compiled, and exactly once
    assert compiled == sorted(os.path.relpath(f, csrc) for f in every if f.endswith((".hip", ".cpp"))), compiled
    shared = [s for s in compiled if not s.startswith("dev" + os.sep) and s != "ugsm_no_dev.cpp"]
    assert set(SHIPPED_HIP) <= set(shared) and len(shared) >= 24
    obj_of = {s: os.path.join("build", os.path.splitext(s)[0] + ".o") for s in compiled}
    for c in compiles:   # ... into the object the links name
        assert os.path.relpath(c[c.index("-o") + 1], csrc) == obj_of[srcs(c)[0]], c
    objs = lambda c: sorted(os.path.relpath(a, csrc) for a in c if a.endswith(".o"))
    out = lambda c: os.path.basename(c[c.index("-o") + 1])
    by_out = {out(c): c for c in links}
    assert sorted(by_out) == ["libugsm.so", "libugsm_dev.so"] and len(links) == 2
    assert not srcs(by_out["libugsm.so"]) and not srcs(by_out["libugsm_dev.so"]) and "hip" not in by_out["libugsm.so"] + by_out["libugsm_dev.so"]  # (-x hip)
    # libugsm.so: the shared objects + ugsm_no_dev, nothing from dev/; libugsm_dev.so: the shared objects + dev/, not ugsm_no_dev
    assert objs(by_out["libugsm.so"]) == sorted(obj_of[s] for s in shared + ["ugsm_no_dev.cpp"])
    assert objs(by_out["libugsm_dev.so"]) == sorted(obj_of[s] for s in compiled if s != "ugsm_no_dev.cpp")
    assert len([s for s in compiled if s.startswith("dev" + os.sep)]) >= 4


def test_product_refuses_the_configurations_of_the_development_library(lib):
    cfg = lib.Config()
    lib.load().ugsm_default_config(C.byref(cfg))
    cfg.kernel_path = 1
    hnd = C.c_void_p()
    assert lib.load().ugsm_create(C.byref(cfg), C.byref(hnd)) == lib.UGSM_ERR_BAD_ARG
    cfg.kernel_path, cfg.march_min_pixels = 0, -1       # round 1's LDS-tiled K-cost: libugsm_dev.so only since ABI 6
    assert lib.load().ugsm_create(C.byref(cfg), C.byref(hnd)) == lib.UGSM_ERR_BAD_ARG


def test_status_strings(lib):
    for st in range(0, 8):
        assert lib.status_string(st) != "unknown status"
    assert lib.status_string(99) == "unknown status"


def test_geometry_matches_oracle(lib, orc):
    for (W, H, lv) in [(4928, 3264, 14), (1920, 1080, 14), (640, 480, 14), (640, 480, 3), (160, 120, 8), (97, 61, 5)]:
        assert lib.level_dims(W, H, lv) == orc.level_dims(W, H, lv)
    for i in range(20):
        assert lib.level_iterations(i) == orc.iterations_for_level(i)
        assert lib.level_smooth_passes(i) == orc.smooth_passes_for_level(i)
    for mi in (2, 4, 6, 8, 10, 12, 22):
        assert lib.threshold_schedule(mi).tobytes() == orc.threshold_schedule(mi).tobytes()
    assert lib.fovea_dims(4928, 3264, 14, 7) == (615, 407)
    assert lib.fovea_dims(1920, 1080, 14, 7) == (239, 134)


def test_pixel_iterations_match_survey(lib):
    # SURVEY.md Appendix B / BASELINE.md section 2
    assert lib.pixel_iterations(4928, 3264, 14, 0) == 131429636
    assert lib.pixel_iterations(4928, 3264, 14, 7) == 21414118
    assert lib.pixel_iterations(1920, 1080, 14, 0) == 16897288
    assert lib.pixel_iterations(1920, 1080, 14, 7) == 2726516
    assert lib.pixel_iterations(640, 480, 14, 0) == 2480040
    assert lib.pixel_iterations(640, 480, 3, 0) == 1684758


def test_bad_arguments_are_status_codes_not_exits(lib):
    so = lib.load()
    w = (C.c_int * 32)()
    h = (C.c_int * 32)()
    assert so.ugsm_level_dims(0, 10, 3, w, h) == lib.UGSM_ERR_BAD_ARG
    assert so.ugsm_level_dims(10, 10, 40, w, h) == lib.UGSM_ERR_BAD_ARG
    assert so.ugsm_level_dims(64, 48, 14, w, h) == lib.UGSM_ERR_TOO_SMALL  # reference: zero-size mallocs
    assert so.ugsm_level_dims(64, 48, 3, None, h) == lib.UGSM_ERR_BAD_ARG
    assert so.ugsm_create(None, None) == lib.UGSM_ERR_BAD_ARG
    cfg = lib.Config()
    so.ugsm_default_config(C.byref(cfg))
    assert (cfg.levels, cfg.fovea_levels, cfg.slots, cfg.device) == (14, 7, 1, 0)
    cfg.levels = 0
    hnd = C.c_void_p()
    assert so.ugsm_create(C.byref(cfg), C.byref(hnd)) == lib.UGSM_ERR_BAD_ARG


def test_no_device_fails_loudly(lib):
    """On a box without a GPU the product must refuse, not fall back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(lib.UgsmError) as e:
        lib.Context()
    assert e.value.status == lib.UGSM_ERR_NO_DEVICE


def test_product_does_not_import_the_oracle():
    """Only tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke() may touch oracle/."""
    pkg = os.path.join(ROOT, "ug_stereomatcher_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp", ".h")) or f == "Makefile":
                text = open(os.path.join(dirpath, f)).read()
                assert "ugsm_oracle" not in text and "from oracle" not in text and "import oracle" not in text, f
    for f in os.listdir(os.path.join(ROOT, "include")):
        assert "oracle" not in open(os.path.join(ROOT, "include", f)).read()


def test_fovea_mapping_matches_oracle(orc):
    from ug_stereomatcher_amd import _lib
    for (W, H) in [(4928, 3264), (1920, 1080), (640, 480), (333, 217)]:
        for src in range(0, 7):
            assert _lib.fovea_mapping(W, H, src) == orc.fovea_mapping(W, H, src)
        for dest in (1, 3):
            assert _lib.fovea_mapping(W, H, 0, dest) == orc.fovea_mapping(W, H, 0, dest)


def test_ros_node_source_compiles_against_declaration_stubs():
    """ros/UG_GPU_matcher_ugsm.cpp (the catkin node over the shim) has never met ROS in this image.  This is a SYNTAX /
    INTERFACE check only: g++ -fsyntax-only against declaration-only stand-ins (tests/ros_stubs/, see its README) for the ROS,
    cv_bridge, image_transport, message_filters, OpenCV and boost headers it includes -- it catches typos, wrong member names
    and drift against ros/MatchGPULib_ugsm.hpp and include/ugsm.h; it does not build, link or run a node."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if not gxx:
        import pytest
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([gxx, "-std=c++14", "-fsyntax-only", "-Itests/ros_stubs", "-Iros", "-Iinclude", "ros/UG_GPU_matcher_ugsm.cpp"],
                       cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_torch_hip_runtime_is_shared_only_when_the_abi_matches(lib, tmp_path, monkeypatch):
    """the package preloads PyTorch's bundled libamdhip64 (so that `import torch` after it still sees the GPU) only if that
    file's SONAME is the one libugsm.so was linked against; a mismatch -- mocked here by offering another library, and a file that is no
    ELF at all -- is skipped with a warning instead of binding libugsm.so's HIP calls to another runtime ABI.  The opt-out stays."""
    import warnings
    soname, needed = lib._elf_dynamic(lib.LIB_PATH)
    hip = [n for n in needed if n.startswith("libamdhip64.so")]
    assert len(hip) == 1 and soname is None
    other = "/lib/x86_64-linux-gnu/libm.so.6"
    assert lib._elf_dynamic(other)[0] == "libm.so.6"
    junk = tmp_path / "libamdhip64.so"
    junk.write_bytes(b"not an ELF file")
    monkeypatch.delenv("UGSM_NO_TORCH_RUNTIME", raising=False)
    for offered in (other, str(junk)):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert lib._share_torch_hip_runtime(lib.LIB_PATH, torch_hip=offered) == "mismatch"
        assert len(w) == 1 and "not sharing it" in str(w[0].message) and hip[0] in str(w[0].message)
    real = lib._torch_hip_runtime_path()
    if real is not None and lib._elf_dynamic(real)[0] == hip[0]:
        assert lib._share_torch_hip_runtime(lib.LIB_PATH) == "preloaded"
    monkeypatch.setenv("UGSM_NO_TORCH_RUNTIME", "1")
    assert lib._share_torch_hip_runtime(lib.LIB_PATH, torch_hip=other) == "off"


def test_header_is_plain_c99(lib):
    """include/ugsm.h is the boundary a C / C++ / cgo / JNI host binds: it must compile as C99 by itself, and ros/queue_example.c (the
    queue from plain C) must compile against it."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "ugsm.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "ros", "queue_example.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
